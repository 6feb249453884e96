// clrs_mw_types.h -- the plain records of the multi-word path that host and device share: no HIP here, so that the host-only table builder
// (clrs_mw_tables.h) and its CPU tests include them with a plain C++ compiler.  The layouts are what the kernels read (MwDev::blk, MwDev::clu).
#ifndef CLRS_MW_TYPES_H
#define CLRS_MW_TYPES_H

typedef long long mwi64;

struct MwBlk {               // one PSD block (j, l)
    int j, n, kind, delta, U, cnt, P, inv;   // chol(X_b)^-1 is formed beside the factor (Xi): 1 = in LDS, 2 = in place in memory (the block fits in LDS once, not twice), 0 = not
    mwi64 xyoff;             // offset in the xy layout
    mwi64 rd_off;            // offset of its reciprocal Cholesky diagonal in xrd (sum of n over earlier blocks)
    mwi64 v_off;             // low rank: V, n x U column-major fp64 (expanded unique vectors)
    mwi64 vrow_off;          // low rank: first nonzero row of each unique vector [U]
    mwi64 z_off;             // Z / T scratch, n x U
    mwi64 g_off;             // GX / GY scratch, U x U
    mwi64 tptr_off;          // CSR over the cluster's constraints into the sorted term arrays [P+1]
    mwi64 a_off;             // dense: stack of A_e, cnt matrices n x n fp64
    mwi64 sd_off;            // dense: contribution table cnt x cnt
    mwi64 w_off;             // dense: T_e = X^-1 A_e Y, cnt matrices n x n
    mwi64 dmap_off;          // dense: constraint -> entry (or -1) [P]
    mwi64 d0;                // dense: first entry in dense_p
    mwi64 t0;                // low rank: first term (sorted arrays and original order share the range)
    int m, pad2;
};
struct MwClu {               // one cluster j
    int P, b0, b1, lds;      // constraints; block range; 1 = S_j and the inverse of its factor fit in LDS side by side (k_mw_factor), 0 = blocked path
    mwi64 coff, Soff;
    int one_term, pad;       // 1 = at most four PSD blocks and at most one low-rank term per (constraint, block): S_j by k_mw_saccum_one
};

#endif

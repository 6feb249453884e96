// clrs_mw_kernel_vectors.hip.h -- kernel vectors of the PSD blocks of a solution, step 1 of the reference's exact_solution ("Finding the kernel",
// detecteigenvectors, src/rounding.jl:575-642), in multi-word fp64: DESIGN.md section 12.
//
// At an optimum X_b Y_b = 0 and rank X_b + rank Y_b = n_b: the row space of X_b is the kernel of Y_b.  The reference reads a basis of it off the reduced
// row-echelon form of a column-pivoted QR of X_b; for a symmetric PSD block that form is [I W] over the pivot columns of the diagonally pivoted elimination
// of k_mw_rank_reveal (clrs_mw_rank.hip.h), W = G11^-1 G12.  Per block one of two branches, chosen on the host:
//     dual   (MW_KV_DUAL):   X_b is eliminated, rank r:    r vectors,        vector c:  v[perm[c]] = 1,        v[perm[r + a]] = W[c, a],  0 at the other pivots;
//     primal (MW_KV_PRIMAL): Y_b is eliminated, rank r:    n - r vectors,    vector a:  v[perm[r + a]] = 1,    v[perm[c]] = -W[c, a],     0 at the other non-pivots
// (Y v = Y[:, rest_a] - Y[:, piv] W[:, a] = 0: the relations of the dependent columns of Y ARE its kernel).
//
// Two kernels here; the elimination is k_mw_rank_reveal and the residual R_b = Y_b V_b is k_mw_gemm (clrs_mw_gemm.hip.h), both as they are.
//   k_mw_kv_scatter: one workgroup per block writes the vectors from (perm, rank, W) into the pool V -- block b at its offset, column-major n_b x count_b,
//     original index order.  Which number goes where is kv_entry below, host and device (tests/mw_host/mw_kv_host.cpp compiles it with g++).  Every position
//     of the permutation is visited once per vector and perm is a permutation, so every entry of n_b x count_b is stored exactly once and nothing else is.
//   k_mw_kv_colmax: per vector max_i |head R[i, v]| (what the reference asserts on, src/rounding.jl:608, 631-638) and max_i |head V[i, v]| (what it prints).
//     One workgroup per block, 16 vectors at a time with 16 lanes each; the 16 partial maxima of a vector meet in LDS.  A maximum does not depend on the
//     order it is taken in, so the result is reproducible; a NaN is kept, not dropped (fmax would drop it and a broken residual would pass for small).
#ifndef CLRS_MW_KERNEL_VECTORS_HIP_H
#define CLRS_MW_KERNEL_VECTORS_HIP_H

#include "clrs_mw_arith.h"

#define MW_KV_PRIMAL 0
#define MW_KV_DUAL 1

struct MwKvBlk {             // one block of the batch
    int n, branch, rank, count;  // rows; MW_KV_*; rank of the eliminated matrix; vectors (dual: rank, primal: n - rank)
    long long off;           // offset of the block (n x n column-major) in the X / Y / W / V / R planes
    long long xoff;          // offset of its n entries in the perm / maxima arrays
};

namespace mwa {

// Entry of vector v at POSITION j of the permutation (so at original index row = perm[j]) of a block with rank r.  Returns the factor f in {0, +1, -1};
// widx < 0: the entry is f itself; otherwise it is f * W[widx], W the r x (n - r) relations, column-major with leading dimension r.
template <class PP>
MWF int kv_entry(int branch, PP perm, int r, int v, int j, int &row, long &widx) {
    row = perm[j];
    widx = -1;
    if (branch == MW_KV_DUAL) {                     // vector c = v: row c of [I W]
        if (j < r) return j == v ? 1 : 0;
        widx = v + (long)(j - r) * r;
        return 1;
    }
    if (j >= r) return j - r == v ? 1 : 0;          // vector a = v: column a of [-W; I]
    widx = j + (long)v * r;
    return -1;
}

// max that keeps a NaN
MWF double kv_max(double m, double x) { return (x > m || x != x) ? x : m; }

}  // namespace mwa

#if defined(__HIPCC__) || defined(__HIP__)
#include "clrs_mw_kernels.hip.h"

// grid: one workgroup per block.  perm: the permutations of k_mw_rank_reveal; W: its relations (planar, plane `plane`, at the block's offset); V: planar, the same plane.
template <int K>
__global__ __launch_bounds__(MW_NT) void k_mw_kv_scatter(const MwKvBlk *__restrict__ blks, const int *__restrict__ perm, const double *__restrict__ W,
                                                        double *__restrict__ V, mwi64 plane) {
    const MwKvBlk q = blks[blockIdx.x];
    const int n = q.n;
    const long total = (long)n * q.count;
    for (long e = threadIdx.x; e < total; e += MW_NT) {
        const int j = (int)(e % n), v = (int)(e / n);
        int row;
        long widx;
        const int f = mwa::kv_entry(q.branch, perm + q.xoff, q.rank, v, j, row, widx);
        if ((unsigned)row >= (unsigned)n) continue;                    // (a permutation never does this: nothing is stored outside the block)
        const mwi64 o = q.off + row + (mwi64)v * n;
#pragma unroll
        for (int l = 0; l < K; l++) {
            double x;
            if (widx < 0) x = l == 0 ? (double)f : 0.0;
            else { const double w = W[l * plane + q.off + widx]; x = f < 0 ? -w : w; }
            V[l * plane + o] = x;
        }
    }
}

// grid: one workgroup per block; R, V: limb plane 0 of the pools.  rmax / vmax: entry xoff + v for vector v < count.  Not a template (the heads do not depend on the limb
// count): static, launched from the one unit that includes this header and calls it.
static __global__ __launch_bounds__(MW_NT) void k_mw_kv_colmax(const MwKvBlk *__restrict__ blks, const double *__restrict__ R, const double *__restrict__ V,
                                                              double *__restrict__ rmax, double *__restrict__ vmax) {
    __shared__ double red[2][16][17];
    const MwKvBlk q = blks[blockIdx.x];
    const int lo = threadIdx.x & 15, hi = threadIdx.x >> 4;
    for (int v0 = 0; v0 < q.count; v0 += 16) {                         // (uniform over the workgroup)
        const int v = v0 + hi;
        double mr = 0.0, mv = 0.0;
        if (v < q.count)
            for (int i = lo; i < q.n; i += 16) {
                const mwi64 o = q.off + i + (mwi64)v * q.n;
                mr = mwa::kv_max(mr, fabs(R[o]));
                mv = mwa::kv_max(mv, fabs(V[o]));
            }
        red[0][hi][lo] = mr;
        red[1][hi][lo] = mv;
        __syncthreads();
        for (int s = 8; s > 0; s >>= 1) {
            if (lo < s) {
                red[0][hi][lo] = mwa::kv_max(red[0][hi][lo], red[0][hi][lo + s]);
                red[1][hi][lo] = mwa::kv_max(red[1][hi][lo], red[1][hi][lo + s]);
            }
            __syncthreads();
        }
        if (lo == 0 && v < q.count) {
            rmax[q.xoff + v] = red[0][hi][0];
            vmax[q.xoff + v] = red[1][hi][0];
        }
        __syncthreads();
    }
}
#endif

#endif

// clrs_mw_posv.hip.h -- a dense symmetric positive definite solve in multi-word fp64 outside a context: A X = B by a left-looking blocked
// Cholesky with panels of MW_POSV_T = MW_GEMM_T columns.  Everything but the diagonal blocks is a product and goes
// through k_mw_gemm (clrs_mw_gemm.hip.h); this file holds
//   * mw_posv_diag_block<K>: the elimination of one nb x nb diagonal block, nb <= 16, which leaves L11 = chol(S11) and W = L11^-1 -- ONE text for
//     the kernel k_mw_posv_diag<K> and for a g++ build (tests/mw_host/mw_posv_host.cpp), where the lanes become loops;
//   * mw_posv_plan: the launches of a whole solve with their job and tile tables, built once on the host -- the entry clrs_mw_posv
//     (clrs_mw.hip) uploads the tables once and walks the launches, the host restatement walks the same list.
//
// The device pool (one plane per limb; offsets in MwPosvPlan):  S, the working copy of A (n x n, column-major, only the lower triangle is read);
// L, the factor (n x n); Wp, the inverse of every diagonal block (16 x 16 per panel, leading dimension 16, strict upper triangle zero); b, the
// right-hand sides as they are updated; y = L^-1 b; x.  Per panel p (columns c0 .. c0 + nb), forward:
//     update   S[c0:, p] -= L[c0:, :c0] L[p, :c0]^T   and   b[p] -= L[p, :c0] y[:c0]                 one k_mw_gemm launch (none for c0 = 0)
//     diag     L[p, p], Wp[p] = mw_posv_diag_block(S[p, p])                                           k_mw_posv_diag, one workgroup
//     apply    L[c0 + nb:, p] = S[c0 + nb:, p] Wp[p]^T   and   y[p] = Wp[p] b[p]                    one k_mw_gemm launch
// and backward, from the last panel:  y[p] -= L[c0 + nb:, p]^T x[c0 + nb:]  (none for the last panel),  x[p] = Wp[p]^T y[p].
// Every dependency is a launch boundary on one stream: no workgroup waits for another, no atomics, plain vector stores only.
//
// The diagonal block.  One workgroup of MW_NT = 256 lanes holds S11 and W in LDS, planar over the limbs.  The elimination is the fraction-free
// [M | I] form of wg_potrf (clrs_mw_kernels.hip.h): with s_k the product of the scaled pivots so far, step k replaces every entry (i, c) of
// rows i > k by (d~_k a~_ic - a~_ik a~_ck) 2^-ex_k -- columns c > k of M (c <= i) and columns c <= k of W alike -- so a pivot step has no
// reciprocal and no square root on its chain, and what was taken out (1 / sqrt(s_k d~_k) per pivot, one product per entry) happens once after
// the loop for all pivots side by side.  Step k has (nb - k - 1) nb <= 240 entries (nb - k - 1 rows, nb columns: k + 1 of W, the rest of M of
// which those with c > i are idle): ONE entry per lane in every step, so a step lasts as long as one entry's two products and one
// renormalisation, and there is one barrier per pivot.  Lane e of a step owns row k + 1 + e % m, column e / m: a wave reads the pivot column
// a~_ik from consecutive words.  More lanes per entry would split a multi-word product whose carries run through every bin; fewer lanes would
// put several entries on one lane's chain.  A K-limb entry costs about 2 K^2 two_prods against 3 K LDS reads, so LDS banking is not what
// the step waits for and the block is stored with leading dimension 16.
//
// A pivot that is not positive or not finite ends the elimination: the launch records 1 + column in the status word (only when the word is
// still 0) and writes zeros for L11 and W, and so does every later diagonal launch: the launches behind it multiply finite numbers by zeros.
#ifndef CLRS_MW_POSV_HIP_H
#define CLRS_MW_POSV_HIP_H

#include <vector>

#include "clrs_mw_gemm.hip.h"

#define MW_POSV_T MW_GEMM_T                          // columns of a panel: the tile of k_mw_gemm
#define MW_POSV_PL (MW_POSV_T * MW_POSV_T)           // doubles per limb of a block in LDS and of a panel's W in the pool
#define MW_POSV_LDS(K) ((2 * (K) * MW_POSV_PL + 2 * (K) * MW_POSV_T) * sizeof(double))   // M, W and two vectors per pivot; 43.5 KB at 10 limbs

#if defined(__HIP_DEVICE_COMPILE__)
#define MW_POSV_BARRIER() __syncthreads()
#else
#define MW_POSV_BARRIER() ((void)0)                  // the host build runs the lanes of a step one after the other
#endif

namespace mwa {

// Exact scaling of one elimination step: ex even with d 2^-ex in [1/2, 2); p1 = 2^-ex, ph = 2^(-ex/2)  (pivot_scale of clrs_mw_kernels.hip.h
// without device intrinsics; the exponent is kept inside the normal range)
MWF void posv_pivot_scale(double head, double &p1, double &ph) {
    long long u;
    __builtin_memcpy(&u, &head, sizeof u);
    int ex = (int)((u >> 52) & 0x7ff) - 1023;
    ex += ex & 1;
    ex = ex < -1020 ? -1020 : (ex > 1020 ? 1020 : ex);
    const long long a = (long long)(1023 - ex) << 52, b = (long long)(1023 - ex / 2) << 52;
    __builtin_memcpy(&p1, &a, sizeof a);
    __builtin_memcpy(&ph, &b, sizeof b);
}

template <int K, class P>
MWF mw<K> posv_ld(P p, int plane, int i) {
    mw<K> r;
#pragma unroll
    for (int l = 0; l < K; l++) r.l[l] = p[l * plane + i];
    return r;
}
template <int K, class P>
MWF void posv_st(P p, int plane, int i, const mw<K> &v) {
#pragma unroll
    for (int l = 0; l < K; l++) p[l * plane + i] = v.l[l];
}

// The nb x nb block M (planar [K][MW_POSV_PL], column-major with leading dimension MW_POSV_T; the lower triangle is read) -> L11 in its lower
// triangle and W = L11^-1 (same layout), strict upper triangles zero.  `scr`: [2 K][MW_POSV_T].  Lane `tid` of `nt` (the host: 0 of 1).
// Returns 0, or 1 + k at the first pivot that is not positive or not finite (the same value in every lane; M and W are then unfinished).
template <int K, class P>
MWF int mw_posv_diag_block(P M, P W, P scr, int nb, int tid, int nt) {
    constexpr int T = MW_POSV_T, PL = MW_POSV_PL;
#if defined(__HIPCC__) || defined(__HIP__)
    static_assert(MW_POSV_T * (MW_POSV_T - 1) < MW_NT, "one entry per lane in every step, and the last lane, which carries s_k, owns none");
#endif
    P fs = scr, us = scr + K * T;                                       // f_k; s_k until the pivot's post-processing replaces it by 1 / sqrt(d_k)
    for (int e = tid; e < nb * nb; e += nt) {
        const int i = e % nb, c = e / nb;
        posv_st<K>(W, PL, i + c * T, i == c ? from_double<K>(1.0) : zero<K>());
    }
    mw<K> srun = from_double<K>(1.0);                                   // s_k, carried by the last lane (idle in every step)
    if (tid == nt - 1) posv_st<K>(us, T, 0, srun);
    MW_POSV_BARRIER();
    int fail = 0;
    for (int k = 0; k < nb; k++) {
        const mw<K> d = posv_ld<K>(M, PL, k + k * T);
        if (!(d.l[0] > 0.0 && d.l[0] < __builtin_inf())) { fail = 1 + k; break; }      // every lane reads the same pivot: uniform exit
        if (k + 1 < nb) {
            double p1, ph;
            posv_pivot_scale(d.l[0], p1, ph);
            const mw<K> dh = mul_pow2<K>(d, p1);
            const int m = nb - k - 1;
            for (int e = tid; e < m * nb; e += nt) {
                const int i = k + 1 + e % m, c = e / m;
                const bool tr = c > k;                                  // an entry of the trailing matrix (c <= i) or of rows k + 1 .. of W (c <= k)
                if (tr && c > i) continue;
                const mw<K> ci = mul_pow2<K>(posv_ld<K>(M, PL, i + k * T), ph);
                const mw<K> cj = mul_pow2<K>(tr ? posv_ld<K>(M, PL, c + k * T) : posv_ld<K>(W, PL, k + c * T), ph);
                const mw<K> v = tr ? posv_ld<K>(M, PL, i + c * T) : posv_ld<K>(W, PL, i + c * T);
                acc<K> s;
                acc_zero<K>(s);
                acc_fma<K, K, K>(s, dh, v);
                acc_fma<K, K, K>(s, ci, cj, -1.0);
                const mw<K> r = acc_result<K>(s);
                if (tr) posv_st<K>(M, PL, i + c * T, r);
                else posv_st<K>(W, PL, i + c * T, r);
            }
            if (tid == nt - 1) {
                srun = mul<K>(srun, dh);
                posv_st<K>(us, T, k + 1, srun);
                posv_st<K>(W, PL, (k + 1) + (k + 1) * T, srun);
            }
        }
        MW_POSV_BARRIER();
    }
    if (fail) return fail;
    // per pivot, side by side: f_k = 1 / sqrt(s_k d~_k) = 1 / (s_k sqrt(d_k)), then 1 / sqrt(d_k) = f_k s_k and sqrt(d_k) = d~_k f_k
    for (int k = tid; k < nb; k += nt) {
        const mw<K> sk = posv_ld<K>(us, T, k), dt = posv_ld<K>(M, PL, k + k * T);
        const mw<K> f = rsqrt<K>(mul<K>(sk, dt));
        posv_st<K>(us, T, k, mul<K>(f, sk));
        posv_st<K>(M, PL, k + k * T, mul<K>(dt, f));
        posv_st<K>(fs, T, k, f);
    }
    MW_POSV_BARRIER();
    // one product per entry: L_ic = a~_ic f_c, (L^-1)_ic = W_ic f_i; the diagonal of W is 1 / sqrt(d_i)
    for (int e = tid; e < nb * nb; e += nt) {
        const int i = e % nb, c = e / nb, o = i + c * T;
        if (i > c) {
            posv_st<K>(M, PL, o, mul<K>(posv_ld<K>(M, PL, o), posv_ld<K>(fs, T, c)));
            posv_st<K>(W, PL, o, mul<K>(posv_ld<K>(W, PL, o), posv_ld<K>(fs, T, i)));
        } else if (i == c) {
            posv_st<K>(W, PL, o, posv_ld<K>(us, T, i));
        } else {
            posv_st<K>(M, PL, o, zero<K>());
            posv_st<K>(W, PL, o, zero<K>());
        }
    }
    MW_POSV_BARRIER();
    return 0;
}

}  // namespace mwa

// ---- the launches of one solve (host) ----
struct MwPosvLaunch {
    int diag;                // 1: k_mw_posv_diag of panel `panel`; 0: k_mw_gemm over rows tile0 .. tile0 + ntiles of the tile table
    int panel, tile0, ntiles;
};
struct MwPosvPlan {
    int n = 0, nrhs = 0, npanels = 0;
    long long s_off = 0, l_off = 0, w_off = 0, b_off = 0, y_off = 0, x_off = 0, plane = 0;      // the pool
    std::vector<MwGemmJob> jobs;
    std::vector<int> tiles;              // (job, tile row, tile column) per 16 x 16 tile, the launches one after the other
    std::vector<MwPosvLaunch> launches;
};

static inline void mw_posv_plan_gemm(MwPosvPlan &q, const MwGemmJob *jobs, int njobs) {
    const int first = (int)(q.tiles.size() / 3);
    for (int t = 0; t < njobs; t++) {
        const MwGemmJob &j = jobs[t];
        if (j.m <= 0 || j.n <= 0) continue;
        const int id = (int)q.jobs.size();
        q.jobs.push_back(j);
        for (int tj = 0; tj < (j.n + MW_GEMM_T - 1) / MW_GEMM_T; tj++)
            for (int ti = 0; ti < (j.m + MW_GEMM_T - 1) / MW_GEMM_T; ti++) { q.tiles.push_back(id); q.tiles.push_back(ti); q.tiles.push_back(tj); }
    }
    const int count = (int)(q.tiles.size() / 3) - first;
    if (count > 0) q.launches.push_back(MwPosvLaunch{0, 0, first, count});
}

static inline MwPosvPlan mw_posv_plan(int n, int nrhs) {
    constexpr int T = MW_POSV_T;
    MwPosvPlan q;
    q.n = n;
    q.nrhs = nrhs;
    q.npanels = (n + T - 1) / T;
    const long long nn = (long long)n * n, nr = (long long)n * nrhs;
    q.s_off = 0;
    q.l_off = nn;
    q.w_off = 2 * nn;
    q.b_off = q.w_off + (long long)q.npanels * MW_POSV_PL;
    q.y_off = q.b_off + nr;
    q.x_off = q.y_off + nr;
    q.plane = q.x_off + nr;
    for (int p = 0; p < q.npanels; p++) {
        const int c0 = p * T, nb = n - c0 < T ? n - c0 : T, below = n - c0 - nb;
        const long long w = q.w_off + (long long)p * MW_POSV_PL;
        if (c0 > 0) {
            const MwGemmJob up[2] = {
                {n - c0, nb, c0, 0, 1, -1, 1, n, n, n, q.l_off + c0, q.l_off + c0, q.s_off + c0 + (long long)c0 * n},
                {nb, nrhs, c0, 0, 0, -1, 1, n, n, n, q.l_off + c0, q.y_off, q.b_off + c0}};
            mw_posv_plan_gemm(q, up, 2);
        }
        q.launches.push_back(MwPosvLaunch{1, p, 0, 0});
        const MwGemmJob ap[2] = {
            {below, nb, nb, 0, 1, 1, 0, n, T, n, q.s_off + c0 + nb + (long long)c0 * n, w, q.l_off + c0 + nb + (long long)c0 * n},
            {nb, nrhs, nb, 0, 0, 1, 0, T, n, n, w, q.b_off + c0, q.y_off + c0}};
        mw_posv_plan_gemm(q, ap, 2);
    }
    for (int p = q.npanels - 1; p >= 0; p--) {
        const int c0 = p * T, nb = n - c0 < T ? n - c0 : T, below = n - c0 - nb;
        const long long w = q.w_off + (long long)p * MW_POSV_PL;
        if (below > 0) {
            const MwGemmJob dn = {nb, nrhs, below, 1, 0, -1, 1, n, n, n, q.l_off + c0 + nb + (long long)c0 * n, q.x_off + c0 + nb, q.y_off + c0};
            mw_posv_plan_gemm(q, &dn, 1);
        }
        const MwGemmJob xs = {nb, nrhs, nb, 1, 0, 1, 0, T, n, n, w, q.y_off + c0, q.x_off + c0};
        mw_posv_plan_gemm(q, &xs, 1);
    }
    return q;
}

#if defined(__HIPCC__) || defined(__HIP__)
// One workgroup of MW_NT lanes; dynamic LDS: MW_POSV_LDS(K) bytes.  The nb x nb block of S at s_off (leading dimension ld) -> its factor at l_off
// (lower triangle; the entries above it are not written) and the inverse of the factor at w_off (nb x nb, leading dimension MW_POSV_T, all of it).
// *status: 0, or 1 + the column of the first failed pivot of this solve.
template <int K>
__global__ __launch_bounds__(MW_NT) void k_mw_posv_diag(double *pool, mwi64 plane, mwi64 s_off, mwi64 l_off, int ld, mwi64 w_off, int nb, int col0, int *status) {
    using namespace mwk;
    constexpr int T = MW_POSV_T, PL = MW_POSV_PL;
    const int tid = threadIdx.x;
    lds_d *M = MW_LDS, *W = M + K * PL, *scr = W + K * PL;
    const int before = *status;
    for (int e = tid; e < nb * nb; e += MW_NT) {
        const int i = e % nb, c = e / nb;
#pragma unroll
        for (int l = 0; l < K; l++) M[l * PL + i + c * T] = i >= c ? pool[l * plane + s_off + i + (mwi64)c * ld] : 0.0;
    }
    __syncthreads();                                                    // (also: every lane has read the status word before lane 0 writes it)
    int fail = 0;
    if (before == 0) {
        fail = mw_posv_diag_block<K>(M, W, scr, nb, tid, MW_NT);
        if (fail && tid == 0) *status = col0 + fail;
    }
    const bool dead = before != 0 || fail != 0;
    for (int e = tid; e < nb * nb; e += MW_NT) {
        const int i = e % nb, c = e / nb;
#pragma unroll
        for (int l = 0; l < K; l++) {
            if (i >= c) pool[l * plane + l_off + i + (mwi64)c * ld] = dead ? 0.0 : M[l * PL + i + c * T];
            pool[l * plane + w_off + i + c * T] = dead ? 0.0 : W[l * PL + i + c * T];
        }
    }
}
#endif

#endif

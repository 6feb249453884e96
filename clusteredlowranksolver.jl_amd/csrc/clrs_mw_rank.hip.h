// clrs_mw_rank.hip.h -- rank-revealing (diagonally pivoted) Cholesky of symmetric positive semidefinite matrices in multi-word fp64:
// the device side of the linear-dependency detection (the reference's preprocess!, src/pre_postprocessing.jl).
//
// The reference factors (all PSD entries) x (all constraints) by a column-pivoted QR.  The Gram matrix of the constraint matrices of a
// cluster is S_j(X = I, Y = I), which the assembly kernels already produce, and R_ii^2 of that QR is pivot i of the diagonally pivoted
// Cholesky of the Gram matrix (column-norm pivoting = diagonal pivoting), so the rank, the dependent set and the relation coefficients are
// those of this factorisation.
//
// One workgroup per matrix, a batch of matrices of different sizes.  The elimination is the fraction-free one of wg_potrf
// (clrs_mw_kernels.hip.h): with a~ = s_k a,
//     a~_ij  <-  (d~_k a~_ij - a~_ik a~_jk) 2^-ex_k ,      s_(k+1) = s_k d~_k 2^-ex_k ,
// no division on the pivot chain and an exact power of two that keeps s_k near 1 -- here with the pivot CHOSEN at every step: the largest
// remaining diagonal among the candidates (indices < ncand), ties to the smallest original index.  All scaled entries of a step share the
// factor s_k, so the choice compares the fp64 heads of the scaled diagonal.  Rows and columns are never moved: a permutation in LDS (pivots
// first, in pivot order, then the rest in original order) names the remaining indices, and because the rest stays in original order, entry
// (i, c) of two remaining indices is always read from the lower triangle as stored.
//
// The same elimination runs on the rows of a unit matrix beside M ([M | I]).  After r steps the row of a NON-pivot index i holds, in the
// columns of the pivots, -s_r G_(i,piv) G_11^-1: the coefficients that express constraint i by the pivots, W = G_11^-1 G_12, are read off
// with one multi-word reciprocal (of s_r) and one product per entry -- no substitution, no second pass over the factor.  The unscaled
// residual diagonal a~_ii / s_r of the non-pivots comes from the same reciprocal.
//
// One barrier per pivot: the diagonal entries written during a step ARE the published heads (limb plane 0 of the diagonal), and after the
// step's barrier every wave finds the next pivot from them redundantly (n / 64 loads per lane and six shuffle rounds), so no second
// barrier and no broadcast sit on the chain.  The new permutation is written to the other of two buffers during the step.
// A pivot step with m remaining indices and k pivots behind it is m (m + 1) / 2 + m (k + 1) two-product updates over the workgroup.
//
// Residence: M and the unit part side by side in LDS while 2 K n^2 doubles (plus the s_k and the permutation) fit in the workgroup's
// budget; otherwise the SAME body on planes in global memory (the accessors are template parameters, as in wg_potrf) -- slow, one-off.
#ifndef CLRS_MW_RANK_HIP_H
#define CLRS_MW_RANK_HIP_H

#include "clrs_mw_kernels.hip.h"

struct MwRankMat {           // one matrix of the batch
    int n, ncand, lds, pad;  // rows; indices < ncand may become pivots; 1 = M and the unit part fit in LDS
    mwi64 goff;              // offset of the matrix (n x n column-major) in the G / workspace / W planes
    mwi64 xoff;              // offset of its n entries in the perm / residual arrays
    double tau;              // stop when the largest remaining candidate diagonal, unscaled, is <= tau
};
// doubles of LDS beside the matrices: s_0 .. s_n (K limbs each) and two permutations of n ints
#define MW_RANK_SCR(K, n) ((long)(K) * ((n) + 1) + (n) + 2)
#define MW_RANK_LDS(K, n) ((MW_RANK_SCR(K, n) + 2l * (K) * (n) * (n)) * 8)      // bytes of the LDS-resident form

namespace mwk {

// M: n x n, leading dimension n, lower triangle used (and overwritten); Wm: n x n workspace (row = original index, column = pivot number).
// Outputs to global memory: perm[n], *rank, resid (n - r entries, planar with plane xplane), Wout (r x (n - r) column-major with leading
// dimension r, planar with plane gplane).
template <int K, class PM, class PW>
__device__ __forceinline__ void wg_rank_reveal(PM M, long plane, PW Wm, long wplane, int n, int ncand, double tau, lds_d *scr, int tid, int *__restrict__ perm,
                                               int *__restrict__ rank, double *__restrict__ resid, long xplane, double *__restrict__ Wout, long gplane) {
    constexpr int NT = MW_PT;
    lds_d *us = scr;                                                     // s_k, planar with plane n + 1
    typedef __attribute__((address_space(3))) int lds_i;
    lds_i *pb = (lds_i *)(scr + (long)K * (n + 1));                     // two permutations of n entries
    for (int e = tid; e < n * n; e += NT) stx<K>(Wm, wplane, e, zero<K>());
    for (int i = tid; i < n; i += NT) pb[i] = i;
    mw<K> srun = from_double<K>(1.0);                                    // s_k, carried by the last thread
    if (tid == NT - 1) stx<K>(us, n + 1, 0, srun);
    __syncthreads();
    const int lane = tid & 63;
    int k = 0;
    for (; k < n; k++) {
        lds_i *pc = pb + (k & 1) * n, *pn = pb + ((k + 1) & 1) * n;
        // the next pivot: largest head of the remaining candidates' diagonal, ties to the smallest index; the same in every wave
        double bv = -__builtin_inf();
        int bi = 0x7fffffff, bt = -1;
        for (int j = k + lane; j < n; j += 64) {
            const int i = pc[j];
            if (i < ncand) {
                const double v = M[i + (long)i * n];
                if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; bt = j; }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64), ot = __shfl_xor(bt, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; bt = ot; }
        }
        if (bt < 0 || !(bv > tau * us[k])) break;                       // (us[k]: the head of s_k; uniform over the workgroup)
        const int p = bi, t = bt;
        const mw<K> d = ldx<K>(M, plane, p + (long)p * n);
        double p1, ph;
        pivot_scale(d.l[0], p1, ph);
        const mw<K> dh = mul_pow2<K>(d, p1);
        // the permutation after this step: the pivot moves to position k, positions k .. t - 1 shift up by one, the rest stays
        for (int j = tid; j < n; j += NT) pn[j] = j < k || j > t ? pc[j] : j == k ? p : pc[j - 1];
        const int m = n - k - 1, trail = m * (m + 1) / 2, total = trail + m * (k + 1);
        for (int e = tid; e < total; e += NT) {
            int a, b;
            const bool tr = e < trail;
            if (tr) tri_index(e, a, b);
            else { a = (e - trail) % m; b = (e - trail) / m; }
            const int ja = k + 1 + a, i = ja <= t ? pc[ja - 1] : pc[ja];               // remaining index number a (original order: i > c below)
            const mw<K> ci = mul_pow2<K>(ldx<K>(M, plane, i > p ? i + (long)p * n : p + (long)i * n), ph);
            mw<K> cj, v;
            long idx;
            if (tr) {
                const int jb = k + 1 + b, c = jb <= t ? pc[jb - 1] : pc[jb];
                cj = mul_pow2<K>(ldx<K>(M, plane, c > p ? c + (long)p * n : p + (long)c * n), ph);
                idx = i + (long)c * n;
                v = ldx<K>(M, plane, idx);
            } else {
                idx = i + (long)b * n;                                                   // column b <= k of the unit part
                if (b == k) { cj = mul_pow2<K>(ldx<K>(us, n + 1, k), ph); v = zero<K>(); }      // the unit entry of the pivot's row: s_k
                else { cj = mul_pow2<K>(ldx<K>(Wm, wplane, p + (long)b * n), ph); v = ldx<K>(Wm, wplane, idx); }
            }
            acc<K> s;
            acc_zero<K>(s);
            acc_fma<K, K, K>(s, dh, v);
            acc_fma<K, K, K>(s, ci, cj, -1.0);
            const mw<K> r = acc_result<K>(s);
            if (tr) stx<K>(M, plane, idx, r);
            else stx<K>(Wm, wplane, idx, r);
        }
        if (tid == NT - 1) {
            srun = mul<K>(srun, dh);
            stx<K>(us, n + 1, k + 1, srun);
        }
        __syncthreads();
    }
    // k pivots; the permutation is in buffer k & 1
    const int r = k;
    lds_i *pc = pb + (r & 1) * n;
    if (tid == 0) *rank = r;
    for (int j = tid; j < n; j += NT) perm[j] = pc[j];
    const int nd = n - r;
    if (nd == 0) return;
    const mw<K> rs = recip<K>(ldx<K>(us, n + 1, r));                     // 1 / s_r, by every thread
    for (int e = tid; e < nd * (r + 1); e += NT) {
        const int a = e / (r + 1), c = e % (r + 1), i = pc[r + a];
        if (c == r) stx<K>(resid, xplane, a, mul<K>(ldx<K>(M, plane, i + (long)i * n), rs));
        else stx<K>(Wout, gplane, c + (long)a * r, neg<K>(mul<K>(ldx<K>(Wm, wplane, i + (long)c * n), rs)));
    }
}

}  // namespace mwk

// grid: one workgroup per matrix.  G (planar, plane gplane) is overwritten where a matrix is not LDS-resident; Wk: workspace of the same shape for those
// matrices (may be null when every matrix is LDS-resident).
template <int K>
__global__ __launch_bounds__(MW_PT) void k_mw_rank_reveal(const MwRankMat *__restrict__ mats, double *__restrict__ G, double *__restrict__ Wk, mwi64 gplane,
                                                         double *__restrict__ Wout, int *__restrict__ perm, int *__restrict__ rank, double *__restrict__ resid,
                                                         mwi64 xplane) {
    using namespace mwk;
    const MwRankMat q = mats[blockIdx.x];
    const int n = q.n, tid = threadIdx.x;
    if (n <= 0) { if (tid == 0) rank[blockIdx.x] = 0; return; }
    lds_d *scr = MW_LDS;
    if (q.lds) {
        lds_d *M = MW_LDS + MW_RANK_SCR(K, n), *Wm = M + (long)K * n * n;
        wg_copy<K, MW_PT>(M, (long)n * n, n, G + q.goff, gplane, n, n, n, tid);
        __syncthreads();
        wg_rank_reveal<K>(M, (long)n * n, Wm, (long)n * n, n, q.ncand, q.tau, scr, tid, perm + q.xoff, rank + blockIdx.x, resid + q.xoff, xplane, Wout + q.goff, gplane);
    } else {
        wg_rank_reveal<K>(G + q.goff, gplane, Wk + q.goff, gplane, n, q.ncand, q.tau, scr, tid, perm + q.xoff, rank + blockIdx.x, resid + q.xoff, xplane, Wout + q.goff, gplane);
    }
}

#endif

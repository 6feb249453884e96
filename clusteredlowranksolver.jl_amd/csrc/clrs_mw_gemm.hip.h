// clrs_mw_gemm.hip.h -- a general batched matrix product in multi-word fp64: C <- beta C + alpha op(A) op(B) on planar limb arrays, the
// building block of everything that multiplies matrices OUTSIDE a context (the substitution of preprocess: DESIGN.md section 11).
//
// A job is one product: column-major matrices with leading dimensions inside three planar pools (limb l of element o of a pool is
// pool[l * plane + o]), op = identity or transpose, alpha in {-1, +1}, beta in {-1, 0, +1} -- both scalings are exact.  One launch takes a batch
// of jobs of different shapes through a table with one row (job, tile row, tile column) per 16 x 16 tile of some C.
//
// One workgroup of 256 threads per tile, one entry of C per thread in one accumulator (mwk::acc<K + 1>).  The contraction is walked in chunks of
// MW_GEMM_KC: a 16 x KC panel of op(A) and a KC x 16 panel of op(B) are staged in LDS, planar over the limbs, with op applied while staging, so
// that the inner loop reads A_s[l][r][i] (contiguous over i, broadcast over j) and B_s[l][r][j] (broadcast over i) whatever the job's op; the staged rows are
// padded to 17 doubles so that the staging writes of a transposed operand spread over the banks too.
//
// Order of operations of one entry -- the whole definition of the result, shared word for word by the device and by a host loop
// (gemm_entry_accum / gemm_entry_finish below are MWF: tests/mw_host/mw_gemm_host.cpp compiles them with g++):
//     s = 0;  for r = 0 .. k - 1 ascending:  s += alpha a_ir b_rj  (acc_fma<K + 1, K, K>, the larger factor first, the sign on its limbs: exact);
//     v = acc_result(s) cut to K limbs;  beta != 0:  v = v + beta c_ij  (one multi-word add);  c_ij = v.
// The accumulator carries ONE BIN MORE than the numbers have limbs.  Only the last bin of an accumulator rounds, but the remainders of every push cascade
// upwards, so the bins do not fall off by 2^-53 per order: measured on the host with 64 full-limb terms, acc<K> ends up to 2^-(53 K - 12) of sum |a b| off at 5
// limbs and 2^-(53 K - 24) at 10, beyond (k + 2) 2^-(52 K - 2); with the guard bin the rounding sits one order lower and the bound holds at every limb count.
// No atomics, no split of k over lanes, nothing that depends on the grid: every result is reproducible bit for bit.  beta = 0 never reads C.
// Lanes outside m x n compute nothing and store nothing; rows m .. ldc - 1 of C are never written.
#ifndef CLRS_MW_GEMM_HIP_H
#define CLRS_MW_GEMM_HIP_H

#include "clrs_mw_arith.h"

#define MW_GEMM_T 16         // side of a tile of C
#define MW_GEMM_KC 16        // contraction steps per staged chunk
#define MW_GEMM_LD 17        // doubles per staged row (T + 1: a transposed operand is staged with the row index running over the lanes -- a stride of 16 doubles would
                             // put the ds_write on two banks); 2 K KC 17 doubles of LDS, 43.5 KB at 10 limbs: three workgroups per compute unit
#define MW_GEMM_LDS(K) (2 * (K) * MW_GEMM_KC * MW_GEMM_LD * sizeof(double))

struct MwGemmJob {           // the layout of clrs_mw_gemm_job (include/clrs_hip.h)
    int m, n, k, transa, transb, alpha, beta, lda, ldb, ldc;
    long long a_off, b_off, c_off;
};

namespace mwa {

// s += sgn * sum_{r < kc} a_r b_r, r ascending: limb l of a_r is a[l * aplane + r * astride] (PA / PB: pointers to global memory, LDS or host memory)
template <int K, class PA, class PB>
MWF void gemm_entry_accum(acc<K + 1> &s, int kc, PA a, long aplane, long astride, PB b, long bplane, long bstride, double sgn) {
    for (int r = 0; r < kc; r++) {
        mw<K> x, y;
#pragma unroll
        for (int l = 0; l < K; l++) {
            x.l[l] = a[(long)l * aplane + (long)r * astride];
            y.l[l] = b[(long)l * bplane + (long)r * bstride];
        }
        // the two factors in a canonical order (the larger one first, limb by limb): a product does not depend on which operand brought which factor, so
        // A^T A is symmetric bit for bit (acc_fma visits the limb pairs of (x, y) and of (y, x) in different orders; its last bin rounds)
        bool sw = false, open = true;
#pragma unroll
        for (int l = 0; l < K; l++) {
            if (open && x.l[l] != y.l[l]) { sw = x.l[l] < y.l[l]; open = false; }
        }
        mw<K> u, v;
#pragma unroll
        for (int l = 0; l < K; l++) {
            u.l[l] = sw ? y.l[l] : x.l[l];
            v.l[l] = sw ? x.l[l] : y.l[l];
        }
        acc_fma<K + 1, K, K>(s, u, v, sgn);
    }
}
// the entry of C: the renormalised sum plus beta c (c is read only when beta != 0)
template <int K>
MWF void gemm_entry_finish(const acc<K + 1> &s, int beta, double *c, long cplane) {
    mw<K> v = cvt<K, K + 1>(acc_result<K + 1>(s));
    if (beta != 0) {
        const mw<K> c0 = ld_<K>(c, cplane, 0);
        v = beta > 0 ? add<K>(v, c0) : sub<K>(v, c0);
    }
    st<K>(c, cplane, 0, v);
}

}  // namespace mwa

#if defined(__HIPCC__) || defined(__HIP__)
#include "clrs_mw_kernels.hip.h"

// grid: one workgroup of MW_NT threads per row of `tiles` (job, tile row, tile column); dynamic LDS: MW_GEMM_LDS(K) bytes
template <int K>
__global__ __launch_bounds__(MW_NT) void k_mw_gemm(const MwGemmJob *__restrict__ jobs, const int *__restrict__ tiles, const double *A, mwi64 aplane,
                                                  const double *B, mwi64 bplane, double *C, mwi64 cplane) {
    using namespace mwk;
    constexpr int T = MW_GEMM_T, KC = MW_GEMM_KC, LD = MW_GEMM_LD, PL = KC * LD;
    static_assert(MW_NT == T * T && KC == T, "one thread per entry of the tile and per entry of a staged panel");
    const MwGemmJob q = jobs[tiles[3 * blockIdx.x]];
    const int ti = tiles[3 * blockIdx.x + 1], tj = tiles[3 * blockIdx.x + 2];
    const int tid = threadIdx.x, lo = tid & (T - 1), hi = tid >> 4;
    lds_d *As = MW_LDS, *Bs = As + K * PL;
    const int gi = ti * T + lo, gj = tj * T + hi;                 // this thread's entry of C
    const bool live = gi < q.m && gj < q.n;
    // staging: the index that is contiguous in memory runs over the low four bits of the thread number
    const int a_i = q.transa ? hi : lo, a_r = q.transa ? lo : hi; // op(A)(i, r) = A(i, r) or A(r, i)
    const int b_r = q.transb ? hi : lo, b_j = q.transb ? lo : hi; // op(B)(r, j) = B(r, j) or B(j, r)
    const int arow = ti * T + a_i, bcol = tj * T + b_j;
    acc<K + 1> s;
    acc_zero<K + 1>(s);
    for (int r0 = 0; r0 < q.k; r0 += KC) {
        const int ar = r0 + a_r, br = r0 + b_r;
        const bool aok = arow < q.m && ar < q.k, bok = bcol < q.n && br < q.k;
        const mwi64 ai = q.a_off + (q.transa ? ar + (mwi64)arow * q.lda : arow + (mwi64)ar * q.lda);
        const mwi64 bi = q.b_off + (q.transb ? bcol + (mwi64)br * q.ldb : br + (mwi64)bcol * q.ldb);
#pragma unroll
        for (int l = 0; l < K; l++) {
            As[l * PL + a_r * LD + a_i] = aok ? A[l * aplane + ai] : 0.0;
            Bs[l * PL + b_r * LD + b_j] = bok ? B[l * bplane + bi] : 0.0;
        }
        __syncthreads();
        if (live) gemm_entry_accum<K>(s, min(KC, q.k - r0), As + lo, PL, LD, Bs + hi, PL, LD, (double)q.alpha);
        __syncthreads();
    }
    if (live) gemm_entry_finish<K>(s, q.beta, C + q.c_off + gi + (mwi64)gj * q.ldc, cplane);
}
#endif

#endif

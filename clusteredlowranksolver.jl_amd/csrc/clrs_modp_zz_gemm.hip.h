// clrs_modp_zz_gemm.hip.h -- the exact product C = A B of integer matrices given in balanced base-2^24 digit planes (clrs_zz_gemm, include/clrs_hip.h;
// DESIGN.md section 18): the matrix arithmetic around the fixed-width steps of the rounding chain (Gram matrices, normal equations, the checks A x == b of
// project_to_affine_space / is_valid_solution, src/rounding.jl:182-415).  No context, host pointers.  Included at the end of clrs_modp.hip, whose ModpBufs,
// modp_fail and MODPCHECK it uses, behind clrs_modp_tile.hip.h.
//
// A digit-by-digit product is ONE ordinary GEMM of one-digit matrices: A' = [A_0; ...; A_{nda-1}] ((nda m) x k: the planes as they lie in memory),
// B' = [B_0 | ... | B_{ndb-1}] (k x (ndb n)), P = A' B', and plane s of the product is C_s = sum_i P[i m + r, (s - i) n + j] before carries.  A vector of long
// integers is thus a matrix of digits whose columns are reused from LDS like any GEMM's.
//
//   k_zz_widen     int32 -> fp64; B repacked to B'.
//   k_zz_gemm      the hot path: P = A' B'[:, columns of a range of digits] by the tile loop of clrs_modp_tile.hip.h (a 64 x 64 tile of P per workgroup of four
//                  waves on v_mfma_f64_16x16x4, the panels staged in LDS).  Every accumulator is flushed after 7 steps = 28 MFMAs (clrs_modp_zz_arith.h: at most
//                  31 keep the sum below 2^53) and once at the end; the kernel writes (lo, hi) per entry, value = lo + hi 2^24.  One code path: rows >= nda m,
//                  columns >= the range and k >= the inner extent load zeros, stores are masked.
//   k_zz_combine   S[s] += sum_i lo(P[i m + r, (s - i) n + j]) + hi(P[i m + r, (s - 1 - i) n + j]) over the digits of the range, int64 planes
//                  S[nda + ndb][m][n]: sums of at most 2 min(nda, ndb) terms, below 2^62 by the refusal min(nda, ndb) k < 2^30.  One thread per entry of S that
//                  the range reaches, no atomics (the ranges run one after the other on one stream).
//   k_zz_carry     one thread per entry of C: zz_carry_walk (clrs_modp_zz_arith.h) upward through the planes of S.
//
// P takes 16 bytes per entry of an (nda m) x (digits n) matrix: B' is cut into ranges of digits so that P stays below ZZ_GEMM_CHUNK_BYTES (256 MiB;
// clrs_config_set("zz_gemm_chunk_bytes", b) lowers it, for the tests; a range is never less than one digit).  Everything after the GEMM is integer arithmetic,
// so the result does not depend on the ranges.
#pragma once

#include "clrs_modp_zz_arith.h"

#define ZZ_NT 256                     // threads of a workgroup of every kernel: four waves
#define ZZ_FLUSH_STEPS (ZZ_FLUSH_MFMAS / (ZZ_BK / 4))
#define ZZ_GEMM_CHUNK_BYTES ((size_t)256 << 20)
#define ZZ_MAX_DIGITS 32767

static_assert(ZZ_FLUSH_STEPS >= 1 && ZZ_FLUSH_STEPS * (ZZ_BK / 4) <= ZZ_MAX_FLUSH_MFMAS, "an accumulator takes at most 31 MFMAs between two flushes");

extern int g_cfg_zz_gemm_chunk_bytes;          // clrs_hip.hip, clrs_config_set("zz_gemm_chunk_bytes", bytes): 0 = ZZ_GEMM_CHUNK_BYTES

// Ad = A as fp64 (count_a entries as they lie); Bp[kk][t n + j] = B[t][kk][j] as fp64 (k x (ndb n))
__global__ __launch_bounds__(ZZ_NT) void k_zz_widen(const int32_t *__restrict__ A, size_t count_a, double *__restrict__ Ad, const int32_t *__restrict__ B, int k,
                                                    int n, int ndb, double *__restrict__ Bp) {
    const size_t ldb = (size_t)ndb * n, count_b = (size_t)k * ldb;
    for (size_t o = (size_t)blockIdx.x * ZZ_NT + threadIdx.x; o < count_a + count_b; o += (size_t)gridDim.x * ZZ_NT) {
        if (o < count_a) {
            Ad[o] = (double)A[o];
        } else {
            const size_t q = o - count_a, kk = q / ldb, c = q - kk * ldb, t = c / n, j = c - t * n;
            Bp[q] = (double)B[(t * k + kk) * n + j];
        }
    }
}

// P[r, c] = sum_kk A[r, kk] B[kk, c0 + c] for r < M, c < N as (lo, hi); A is M x K (row stride K), B has row stride ldb; a flat grid of `colblocks` workgroups
// per row of tiles; *err counts pairs that are not what a flushed accumulator can be
__global__ __launch_bounds__(ZZ_NT) void k_zz_gemm(const double *__restrict__ A, int M, int K, const double *__restrict__ B, size_t ldb, size_t c0, int N,
                                                   double2 *__restrict__ P, int colblocks, int *__restrict__ err) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int by = blockIdx.x / colblocks, bx = blockIdx.x - by * colblocks;
    const int row0 = by * ZZ_BM, col0 = bx * ZZ_BN;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    modp_v4d acc[2][2], hi[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) hi[ti][tj][reg] = 0.0;
    zz_tile_loop<ZZ_FLUSH_STEPS>(A, M, K, B, ldb, c0, N, row0, col0, acc, [&](modp_v4d (&lo)[2][2]) {
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 2; tj++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    double a = lo[ti][tj][reg], h = hi[ti][tj][reg];
                    zz_flush(&a, &h);
                    lo[ti][tj][reg] = a; hi[ti][tj][reg] = h;
                }
    });
    // accumulator: column l & 15, row (l >> 4) + 4 reg
    int bad = 0;
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r = row0 + wr + 16 * ti + l4 + 4 * reg, c = col0 + wc + 16 * tj + l15;
                double a = acc[ti][tj][reg], h = hi[ti][tj][reg];
                zz_flush(&a, &h);                                                          // (a flushed accumulator flushes to itself)
                if (r < M && c < N) {
                    bad += zz_pair_bad(a, h);
                    P[(size_t)r * N + c] = make_double2(a, h);
                }
            }
    if (bad) atomicAdd(err, bad);
}

// The digits [t0, t1) of B are in P ((nda m) x ((t1 - t0) n)).  Thread (sl, e): plane s = t0 + sl <= t1 + nda - 1 of S, entry e = r n + j
__global__ __launch_bounds__(ZZ_NT) void k_zz_combine(const double2 *__restrict__ P, int m, int n, int nda, int t0, int t1, long long *__restrict__ S) {
    const size_t mn = (size_t)m * n, N = (size_t)(t1 - t0) * n, total = (size_t)(t1 - t0 + nda) * mn;
    for (size_t o = (size_t)blockIdx.x * ZZ_NT + threadIdx.x; o < total; o += (size_t)gridDim.x * ZZ_NT) {
        const size_t sl = o / mn, e = o - sl * mn, r = e / n, j = e - r * n;
        const int s = t0 + (int)sl;
        long long sum = 0;
        const int i_lo = s - t1 > 0 ? s - t1 : 0, i_hi = s - t0 < nda - 1 ? s - t0 : nda - 1;
        for (int i = i_lo; i <= i_hi; i++) {
            const double2 *row = P + ((size_t)i * m + r) * N + j;
            const int t = s - i;                                                           // lo of digit pair (i, t), hi of (i, t - 1)
            if (t < t1) sum += (long long)row[(size_t)(t - t0) * n].x;
            if (t - 1 >= t0) sum += (long long)row[(size_t)(t - 1 - t0) * n].y;
        }
        S[(size_t)s * mn + e] += sum;
    }
}

// C[ndc][m][n] from S[ns][m][n]; *over counts the entries that do not fit in ndc digits
__global__ __launch_bounds__(ZZ_NT) void k_zz_carry(const long long *__restrict__ S, int ns, size_t mn, int32_t *__restrict__ C, int ndc, int *__restrict__ over) {
    const size_t e = (size_t)blockIdx.x * ZZ_NT + threadIdx.x;
    if (e >= mn) return;
    if (zz_carry_walk(S + e, mn, ns, C + e, mn, ndc)) atomicAdd(over, 1);
}

static thread_local double g_zz_ms[3] = {0.0, 0.0, 0.0};

// the device times of this thread's last clrs_zz_gemm: milliseconds in k_zz_gemm, in k_zz_combine and k_zz_carry, and from the first upload to the last download
extern "C" int clrs_zz_gemm_times(double *gemm_ms, double *combine_ms, double *whole_ms) {
    if (!gemm_ms || !combine_ms || !whole_ms) return modp_fail(CLRS_ERR_INVALID, "zz_gemm_times: null argument");
    *gemm_ms = g_zz_ms[0];
    *combine_ms = g_zz_ms[1];
    *whole_ms = g_zz_ms[2];
    return 0;
}

extern "C" int clrs_zz_gemm(int device, int m, int k, int n, int nda, const int32_t *A, int ndb, const int32_t *B, int ndc, int32_t *C, int32_t *info) {
    if (m < 0 || k < 0 || n < 0) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: negative size");
    if (nda < 1 || nda > ZZ_MAX_DIGITS || ndb < 1 || ndb > ZZ_MAX_DIGITS || ndc < 1 || ndc > ZZ_MAX_DIGITS)
        return modp_fail(CLRS_ERR_INVALID, "zz_gemm: nda, ndb and ndc must lie in [1, 32767]");
    const unsigned long long lim = 1ull << 31;
    const unsigned long long na = (unsigned long long)nda * m * k, nb = (unsigned long long)ndb * k * n, nc = (unsigned long long)ndc * m * n;
    if ((unsigned long long)nda * m + ZZ_BM >= lim || (unsigned long long)ndb * n + ZZ_BN >= lim || na >= lim || nb >= lim || nc >= lim)     // (+ a tile: the kernels' row and column arithmetic stays inside int)
        return modp_fail(CLRS_ERR_INVALID, "zz_gemm: an operand or the result has 2^31 elements or more");
    if ((unsigned long long)std::min(nda, ndb) * k >= (1ull << 30)) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: min(nda, ndb) * k must be below 2^30");
    if (!info || (na && !A) || (nb && !B) || (nc && !C)) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: null argument");
    for (size_t o = 0; o < (size_t)na; o++)
        if (A[o] < -(1 << 23) || A[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: a digit of A outside [-2^23, 2^23]");
    for (size_t o = 0; o < (size_t)nb; o++)
        if (B[o] < -(1 << 23) || B[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: a digit of B outside [-2^23, 2^23]");
    if (m == 0 || n == 0 || k == 0) {                                                      // an empty product: zeros, without a device
        std::fill(C, C + (size_t)nc, 0);
        info[0] = info[1] = info[2] = info[3] = 0;
        g_zz_ms[0] = g_zz_ms[1] = g_zz_ms[2] = 0.0;
        return 0;
    }
    const size_t mn = (size_t)m * n, M = (size_t)nda * m, ldb = (size_t)ndb * n;
    const int ns = nda + ndb;
    const size_t bound = modp_chunk_bound(g_cfg_zz_gemm_chunk_bytes, ZZ_GEMM_CHUNK_BYTES);
    const int dc = (int)std::min<size_t>((size_t)ndb, std::max<size_t>(bound / (M * (size_t)n * sizeof(double2)), 1));      // digits of B per range
    const size_t rowtiles = (M + ZZ_BM - 1) / ZZ_BM, maxcolblocks = ((size_t)dc * n + ZZ_BN - 1) / ZZ_BN;
    if (rowtiles * maxcolblocks >= (size_t)lim) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: one digit of B already needs 2^31 workgroups or more");

    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    int32_t *d_A = nullptr, *d_B = nullptr, *d_C = nullptr;
    double *d_Ad = nullptr, *d_Bp = nullptr;
    double2 *d_P = nullptr;
    long long *d_S = nullptr;
    int *d_cnt = nullptr;                                                                  // [0] impossibilities, [1] entries that do not fit
    MODPCHECK(bufs.get(&d_A, (size_t)na)); MODPCHECK(bufs.get(&d_B, (size_t)nb)); MODPCHECK(bufs.get(&d_Ad, (size_t)na)); MODPCHECK(bufs.get(&d_Bp, (size_t)nb));
    MODPCHECK(bufs.get(&d_P, M * (size_t)dc * n)); MODPCHECK(bufs.get(&d_S, (size_t)ns * mn)); MODPCHECK(bufs.get(&d_cnt, (size_t)2));
    ModpEvents ev(5);
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    MODPCHECK(hipEventRecord(ev.e[3], nullptr));
    MODPCHECK(hipMemcpy(d_A, A, (size_t)na * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_B, B, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_S, 0, (size_t)ns * mn * sizeof(long long)));
    MODPCHECK(hipMemset(d_cnt, 0, 2 * sizeof(int)));
    hipLaunchKernelGGL(k_zz_widen, modp_flat_grid((size_t)na + (size_t)nb, ZZ_NT), dim3(ZZ_NT), 0, nullptr, d_A, (size_t)na, d_Ad, d_B, k, n, ndb, d_Bp);
    MODPCHECK(hipGetLastError());
    double ms[2] = {0.0, 0.0};
    long long launched = 0;
    int chunks = 0;
    for (int t0 = 0; t0 < ndb; t0 += dc) {
        const int t1 = std::min(t0 + dc, ndb), N = (t1 - t0) * n;
        const int colblocks = (N + ZZ_BN - 1) / ZZ_BN;
        MODPCHECK(hipEventRecord(ev.e[0], nullptr));
        hipLaunchKernelGGL(k_zz_gemm, dim3((unsigned)(rowtiles * (size_t)colblocks)), dim3(ZZ_NT), 0, nullptr, d_Ad, (int)M, k, d_Bp, ldb, (size_t)t0 * n, N, d_P,
                           colblocks, d_cnt);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(k_zz_combine, modp_flat_grid((size_t)(t1 - t0 + nda) * mn, ZZ_NT), dim3(ZZ_NT), 0, nullptr, d_P, m, n, nda, t0, t1, d_S);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[2], nullptr));
        MODPCHECK(hipEventSynchronize(ev.e[2]));
        float a = 0.f, b = 0.f;
        MODPCHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        ms[0] += a; ms[1] += b;
        launched += (long long)(rowtiles * (size_t)colblocks);
        chunks++;
    }
    MODPCHECK(bufs.drop(d_P)); MODPCHECK(bufs.drop(d_Ad)); MODPCHECK(bufs.drop(d_Bp)); MODPCHECK(bufs.drop(d_A)); MODPCHECK(bufs.drop(d_B));
    MODPCHECK(bufs.get(&d_C, (size_t)nc));
    MODPCHECK(hipEventRecord(ev.e[0], nullptr));
    hipLaunchKernelGGL(k_zz_carry, dim3((unsigned)((mn + ZZ_NT - 1) / ZZ_NT)), dim3(ZZ_NT), 0, nullptr, d_S, ns, mn, d_C, ndc, d_cnt + 1);
    MODPCHECK(hipGetLastError());
    MODPCHECK(hipEventRecord(ev.e[1], nullptr));
    int cnt[2] = {0, 0};
    std::vector<int32_t> h_C((size_t)nc);                                                  // the caller's array is written only by a call that succeeds
    MODPCHECK(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_C.data(), d_C, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipEventRecord(ev.e[4], nullptr));
    MODPCHECK(hipEventSynchronize(ev.e[4]));
    float carry = 0.f, whole = 0.f;
    MODPCHECK(hipEventElapsedTime(&carry, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&whole, ev.e[3], ev.e[4]));
    g_zz_ms[0] = ms[0]; g_zz_ms[1] = ms[1] + carry; g_zz_ms[2] = whole;
    info[0] = cnt[1]; info[1] = chunks; info[2] = (int32_t)std::min<long long>(launched, 0x7fffffffll); info[3] = cnt[0];
    if (cnt[0] != 0) return modp_fail(CLRS_ERR_HIP, "zz_gemm: " + std::to_string(cnt[0]) + " accumulators that are no integers below 2^53");
    if (cnt[1] != 0) return modp_fail(CLRS_ERR_INVALID, "zz_gemm: " + std::to_string(cnt[1]) + " entries of the product do not fit in ndc digits");
    std::copy(h_C.begin(), h_C.end(), C);
    return 0;
}

// clrs_modp_field_adjugate.hip.h -- the determinant and the adjugate of a square matrix over a number field QQ(g), mod many primes
// (clrs_modp_field_adjugate, include/clrs_hip.h): the device half of rounding.inverse_field, the inverse of the basis change
// B = [V | E] over the field (the reference's inv(B), src/rounding.jl:834-836).  The matrix is M = sum_j M_j g^j with integer M_j, NOT symmetric.  At a
// prime p where the monic minimal polynomial splits, g -> r_i is a ring map Z[g] -> F_p (clrs_modp_minors_field.hip.h), so det M(r_i) and
// adj M(r_i) = det M(r_i) M(r_i)^-1 mod p are the images of det M and adj M, both with entries in Z[g]; the D images give their coefficients mod p (a
// Vandermonde solve, on the host).  Every (prime, root) pair is independent: one workgroup per pair.  Included at the end of clrs_modp.hip; it uses the
// checks of clrs_modp_minors.hip.h and the arithmetic of clrs_modp_field_arith.h, and none of the kernels there.
//
//   k_field_residues_full<D>   every entry of the D matrices M(r_i) mod p for every prime of a chunk: the lane layout and the Horner step of
//                       k_minors_residues_field (one wave per entry, the lanes across MINORS_RES_GROUPS x 64 primes, the digits fetched 64 at a time and
//                       handed round by shuffles, each coefficient reduced once per prime), over all n^2 entries and not the lower triangle.
//   k_field_gj_adjugate one workgroup (MINORS_NT threads) per pair, the matrix resident in LDS (dynamic, sized by n): npad = 16 ceil(n / 16) rows of stride
//                       npad + 1; beside it a pivot row and a multiplier column (npad fp64 each), the permutation and its inverse (npad int32 each) and
//                       four 64-bit masks.  In-place Gauss-Jordan inversion, column by column, the rows staying where they are.  Column c: the pivot row r
//                       is the FIRST row that is no pivot row yet and is non-zero in column c (two ballots per wave, handed over through the masks); none:
//                       the column depends on the columns before it mod p, breakdown = c + 1, det = 0, adj = -1, the pair ends.  Otherwise ONE modp_inv
//                       (every thread for itself, as in k_minors_ldl), the pivot row scaled into its buffer with 1 / pivot in position c, the negated
//                       column c into the multiplier buffer, and the rank-1 step A[i, j] <- w_i row_j + (j == c ? 0 : A[i, j]) on every row i != r: column
//                       c becomes column c of the inverse.  det is the running product of the pivots times the sign of the permutation c -> r(c), whose
//                       parity is the number of free rows passed over, counted from the same ballots.  With rowof[c] = r(c) and colof its inverse the
//                       matrix left in LDS is S with M(r)^-1[i, j] = S[rowof[i], colof[j]], and adj[i, j] = det S[rowof[i], colof[j]] goes out row by row.
//
// Exactness: a rank-1 step is one residue plus one product of residues, (p - 1) + (p - 1)^2 < 2^46, exact in fp64 (the rank-1 step of k_minors_ldl).
// Uniqueness: which column has no pivot does not depend on the rows chosen before it (column c has no pivot iff it depends on the columns 0 .. c - 1),
// nor do the determinant and the adjugate, so every output is a mathematical function of the input and a test compares with ==.
//
// The residue buffer of a chunk of primes is bounded as in clrs_modp_minors_field (clrs_config_set("modp_minors_chunk_bytes", b), 8 n^2 D bytes per prime);
// the adjugates of a chunk (4 n^2 D bytes per prime) are downloaded chunk by chunk.
#pragma once
#include "clrs_modp_field_arith.h"

// R[q D + t, i, j] = sum_c M_c[i, j] roots[q D + t]^c mod p_q for every (i, j); digits [D][nd][n][n], mods [pc D] (prime q stands at q D .. q D + D - 1),
// roots [pc D], R [pc D][n][n]
template <int D>
__global__ __launch_bounds__(MINORS_NT) void k_field_residues_full(const int32_t *__restrict__ digits, int n, int nd, const int32_t *__restrict__ mods,
                                                                   const int32_t *__restrict__ roots, int pc, double *__restrict__ R) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * MINORS_WAVES + (threadIdx.x >> 6);
    if (e >= n * n) return;                                                                // (wave-uniform)
    const int q0 = blockIdx.y * (64 * MINORS_RES_GROUPS);
    double p[MINORS_RES_GROUPS], pinv[MINORS_RES_GROUPS], off[MINORS_RES_GROUPS], acc[MINORS_RES_GROUPS][D];
#pragma unroll
    for (int g = 0; g < MINORS_RES_GROUPS; g++) {
        const int q = q0 + 64 * g + lane;
        p[g] = q < pc ? (double)mods[(size_t)q * D] : 2.0;
        pinv[g] = 1.0 / p[g];
        off[g] = p[g] * ceil(8388608.0 / p[g]);                                            // a multiple of p in [2^23, 2^24)
#pragma unroll
        for (int c = 0; c < D; c++) acc[g][c] = 0.0;
    }
    const size_t plane = (size_t)n * n;
#pragma unroll
    for (int c = 0; c < D; c++) {                                                          // coefficient c of the entry mod every prime of the lane
        const int32_t *src = digits + (size_t)c * nd * plane + (size_t)e;
        for (int top = nd - 1; top >= 0; top -= 64) {
            const int l = top - lane;
            const int dig = l >= 0 ? src[(size_t)l * plane] : 0;
            const int cnt = top + 1 < 64 ? top + 1 : 64;
            for (int t = 0; t < cnt; t++) {
                const double d = (double)__shfl(dig, t, 64);
#pragma unroll
                for (int g = 0; g < MINORS_RES_GROUPS; g++)                                // acc 2^24 + d + off < 2^47 + 2^25, exact (k_minors_residues)
                    acc[g][c] = modp_reduce(fma(acc[g][c], 16777216.0, d + off[g]), p[g], pinv[g]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < MINORS_RES_GROUPS; g++) {
        const int q = q0 + 64 * g + lane;
        if (q < pc) {
#pragma unroll
            for (int t = 0; t < D; t++) R[((size_t)q * D + t) * plane + (size_t)e] = ff_residue<D>(acc[g], (double)roots[(size_t)q * D + t], p[g], pinv[g]);
        }
    }
}

// Pair m0 + blockIdx.x: R is the chunk's residues (matrix blockIdx.x), adj [chunk][n][n] the chunk's adjugates, det and breakdown [count] those of the
// whole call; *err counts pivots that are no residues
__global__ __launch_bounds__(MINORS_NT) void k_field_gj_adjugate(const double *__restrict__ R, int n, int npad, const int32_t *__restrict__ mods, int m0,
                                                                 int32_t *__restrict__ adj, int32_t *__restrict__ det, int32_t *__restrict__ breakdown,
                                                                 int *__restrict__ err) {
    extern __shared__ double s_gj[];
    const int LD = npad + 1;
    double *A = s_gj, *prow = s_gj + npad * LD, *wcol = prow + npad;
    unsigned long long *mask = (unsigned long long *)(wcol + npad);                        // [0..1]: candidates of rows 0 .. 63, 64 .. 127; [2..3]: free rows
    int *rowof = (int *)(mask + 4), *colof = rowof + npad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = m0 + blockIdx.x, p_int = mods[m];
    const double p = (double)p_int, pinv = 1.0 / p;
    const double *Rm = R + (size_t)blockIdx.x * n * n;
    int32_t *am = adj + (size_t)blockIdx.x * n * n;
    for (int o = tid; o < n * n; o += MINORS_NT) {
        const int i = o / n, j = o - i * n;
        A[i * LD + j] = Rm[o];
    }
    for (int i = tid; i < npad; i += MINORS_NT) colof[i] = -1;                             // colof[r] < 0: row r is free
    __syncthreads();
    double prod = 1.0;
    int odd = 0;
    for (int c = 0; c < n; c++) {
        if (wave < 2) {                                                                    // rows 0 .. 127, one per lane of the first two waves
            const bool free_row = tid < n && colof[tid] < 0;
            const unsigned long long fm = __ballot(free_row), cm = __ballot(free_row && A[tid * LD + c] != 0.0);
            if (lane == 0) {
                mask[wave] = cm;
                mask[2 + wave] = fm;
            }
        }
        __syncthreads();
        const unsigned long long c0 = mask[0], c1 = mask[1], f0 = mask[2], f1 = mask[3];   // (every thread: the same LDS words)
        if ((c0 | c1) == 0ull) {                                                           // (uniform) column c depends on the columns before it mod p
            for (int o = tid; o < n * n; o += MINORS_NT) am[o] = -1;
            if (tid == 0) {
                det[m] = 0;
                breakdown[m] = c + 1;
            }
            return;
        }
        const int r = c0 ? __ffsll((long long)c0) - 1 : 64 + __ffsll((long long)c1) - 1;
        odd ^= (r < 64 ? __popcll(f0 & ((1ull << r) - 1ull)) : __popcll(f0) + __popcll(f1 & ((1ull << (r - 64)) - 1ull))) & 1;   // free rows passed over
        const double d = A[r * LD + c];
        if (tid == 0 && !(d > 0.0 && d < p && d == floor(d))) atomicAdd(err, 1);
        prod = modp_mul(prod, d, p, pinv);
        const double dinv = modp_inv(d, p_int);                                            // (every thread for itself: no hand-over)
        if (tid < n) {
            prow[tid] = tid == c ? dinv : modp_mul(A[r * LD + tid], dinv, p, pinv);
            wcol[tid] = modp_neg(A[tid * LD + c], p);
        }
        if (tid == 0) {
            rowof[c] = r;
            colof[r] = c;
        }
        __syncthreads();
        for (int j0 = 0; j0 < n; j0 += 64) {                                               // a wave takes the rows wave, wave + 4, ..: lanes along a row
            const int j = j0 + lane;
            if (j < n) {
                const double pj = prow[j];
                for (int i = wave; i < n; i += MINORS_WAVES) {
                    const double a = j == c ? 0.0 : A[i * LD + j];
                    A[i * LD + j] = i == r ? pj : modp_reduce(fma(wcol[i], pj, a), p, pinv);   // (p - 1)^2 + (p - 1) < 2^46
                }
            }
        }
        __syncthreads();
    }
    const double dm = odd ? modp_neg(prod, p) : prod;
    if (tid == 0) {
        det[m] = (int32_t)dm;
        breakdown[m] = 0;
    }
    for (int i = wave; i < n; i += MINORS_WAVES) {
        const double *Si = A + rowof[i] * LD;
        for (int j = lane; j < n; j += 64) am[i * n + j] = (int32_t)modp_mul(dm, Si[colof[j]], p, pinv);
    }
}

static size_t field_gj_lds_bytes(int n) {
    const size_t npad = (size_t)((n + 15) / 16) * 16;
    return npad * (npad + 1 + 2) * sizeof(double) + 4 * sizeof(unsigned long long) + 2 * npad * sizeof(int);
}

static thread_local double g_field_adjugate_ms[3] = {0.0, 0.0, 0.0};

// the device times of this thread's last clrs_modp_field_adjugate: milliseconds in k_field_residues_full, in k_field_gj_adjugate, and from the first
// upload to the last download
extern "C" int clrs_modp_field_adjugate_times(double *residues_ms, double *gj_ms, double *total_ms) {
    if (!residues_ms || !gj_ms || !total_ms) return modp_fail(CLRS_ERR_INVALID, "modp_field_adjugate_times: null argument");
    *residues_ms = g_field_adjugate_ms[0];
    *gj_ms = g_field_adjugate_ms[1];
    *total_ms = g_field_adjugate_ms[2];
    return 0;
}

extern "C" int clrs_modp_field_adjugate(int device, int n, int deg, int nd, const int32_t *digits, int nprimes, const int32_t *primes, const int32_t *roots,
                                        int32_t *adj, int32_t *det, int32_t *breakdown, int32_t *info) {
    const std::string who = "modp_field_adjugate";
    if (deg < FF_MIN_DEG || deg > FF_MAX_DEG) return modp_fail(CLRS_ERR_INVALID, who + ": deg must lie in [2, 4]");
    if (n < 1 || n > CLRS_MODP_MINORS_MAX_N) return modp_fail(CLRS_ERR_INVALID, who + ": n must lie in [1, 128]");
    if (nd < 1 || nd > MINORS_MAX_DIGITS) return modp_fail(CLRS_ERR_INVALID, who + ": nd must lie in [1, 32767]");
    if (nprimes < 1 || nprimes > MINORS_MAX_PRIMES) return modp_fail(CLRS_ERR_INVALID, who + ": nprimes must lie in [1, 65535]");
    if (!digits || !primes || !roots || !adj || !det || !breakdown || !info) return modp_fail(CLRS_ERR_INVALID, who + ": null argument");
    const size_t plane = (size_t)n * n;
    for (size_t o = 0; o < (size_t)deg * nd * plane; o++)
        if (digits[o] < -(1 << 23) || digits[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, who + ": a digit outside [-2^23, 2^23]");
    if (int code = minors_check_primes(who, nprimes, primes)) return code;
    for (int q = 1; q < nprimes; q++)                                                      // the order split primes are drawn in: from 2^23 downwards
        if (primes[q] >= primes[q - 1]) return modp_fail(CLRS_ERR_INVALID, who + ": the primes must descend");
    for (int q = 0; q < nprimes; q++)
        for (int t = 0; t < deg; t++) {
            const int32_t r = roots[(size_t)q * deg + t];
            if (r < 0 || r >= primes[q]) return modp_fail(CLRS_ERR_INVALID, who + ": a root outside [0, p)");
            for (int u = 0; u < t; u++)
                if (roots[(size_t)q * deg + u] == r) return modp_fail(CLRS_ERR_INVALID, who + ": two equal roots of one prime");
        }
    const int count = nprimes * deg, npad = (n + 15) / 16 * 16;
    std::vector<int32_t> mods((size_t)count);                                              // every prime deg times: the modulus of pair q deg + t
    for (size_t m = 0; m < mods.size(); m++) mods[m] = primes[m / deg];
    const size_t bound = modp_chunk_bound(g_cfg_modp_minors_chunk_bytes, MINORS_CHUNK_BYTES);
    const int chunk = deg * (int)std::min<size_t>((size_t)nprimes, std::max<size_t>(bound / (plane * sizeof(double) * deg), 1));   // in pairs: whole primes
    const size_t lds = field_gj_lds_bytes(n);

    MODPCHECK(hipSetDevice(device));
    if (lds > 48 * 1024) MODPCHECK(hipFuncSetAttribute((const void *)k_field_gj_adjugate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ModpBufs bufs;
    int32_t *d_digits = nullptr, *d_roots = nullptr, *d_mods = nullptr, *d_adj = nullptr, *d_det = nullptr, *d_break = nullptr;
    double *d_R = nullptr;
    int *d_err = nullptr;
    MODPCHECK(bufs.get(&d_digits, (size_t)deg * nd * plane)); MODPCHECK(bufs.get(&d_roots, (size_t)count)); MODPCHECK(bufs.get(&d_mods, (size_t)count));
    MODPCHECK(bufs.get(&d_R, (size_t)chunk * plane)); MODPCHECK(bufs.get(&d_adj, (size_t)chunk * plane));
    MODPCHECK(bufs.get(&d_det, (size_t)count)); MODPCHECK(bufs.get(&d_break, (size_t)count)); MODPCHECK(bufs.get(&d_err, (size_t)1));
    ModpEvents ev(5);
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    MODPCHECK(hipEventRecord(ev.e[3], nullptr));
    MODPCHECK(hipMemcpy(d_digits, digits, (size_t)deg * nd * plane * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_roots, roots, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_mods, mods.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_det, 0xff, (size_t)count * sizeof(int32_t)));                    // -1: a pair that wrote nothing is an impossibility below
    MODPCHECK(hipMemset(d_break, 0xff, (size_t)count * sizeof(int32_t)));
    MODPCHECK(hipMemset(d_err, 0, sizeof(int)));
    std::vector<int32_t> h_adj((size_t)count * plane), h_det((size_t)count), h_break((size_t)count);   // the caller's arrays are written only by a call that succeeds
    double ms[2] = {0.0, 0.0};
    int launched = 0;
    for (int m0 = 0; m0 < count; m0 += chunk) {
        const int mc = std::min(chunk, count - m0), pc = mc / deg;
        const dim3 grid((unsigned)((plane + MINORS_WAVES - 1) / MINORS_WAVES), (unsigned)((pc + 64 * MINORS_RES_GROUPS - 1) / (64 * MINORS_RES_GROUPS)));
        MODPCHECK(hipEventRecord(ev.e[0], nullptr));
        if (deg == 2) hipLaunchKernelGGL(k_field_residues_full<2>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
        if (deg == 3) hipLaunchKernelGGL(k_field_residues_full<3>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
        if (deg == 4) hipLaunchKernelGGL(k_field_residues_full<4>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(k_field_gj_adjugate, dim3((unsigned)mc), dim3(MINORS_NT), lds, nullptr, d_R, n, npad, d_mods, m0, d_adj, d_det, d_break, d_err);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[2], nullptr));
        MODPCHECK(hipEventSynchronize(ev.e[2]));
        float a = 0.f, b = 0.f;
        MODPCHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        ms[0] += a; ms[1] += b;
        MODPCHECK(hipMemcpy(h_adj.data() + (size_t)m0 * plane, d_adj, (size_t)mc * plane * sizeof(int32_t), hipMemcpyDeviceToHost));
        launched += mc;
    }
    int err = 0;
    MODPCHECK(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_det.data(), d_det, h_det.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_break.data(), d_break, h_break.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipEventRecord(ev.e[4], nullptr));
    MODPCHECK(hipEventSynchronize(ev.e[4]));
    float total = 0.f;
    MODPCHECK(hipEventElapsedTime(&total, ev.e[3], ev.e[4]));
    g_field_adjugate_ms[0] = ms[0]; g_field_adjugate_ms[1] = ms[1]; g_field_adjugate_ms[2] = total;
    int singular = 0;
    for (int m = 0; m < count; m++) {                                                      // a residue where one belongs, -1 throughout for a singular pair
        const int k = h_break[m];
        const int32_t *a = h_adj.data() + (size_t)m * plane;
        if (k != 0) singular++;
        if (k < 0 || k > n || (k != 0 ? h_det[m] != 0 : (h_det[m] < 1 || h_det[m] >= mods[m]))) err++;
        for (size_t o = 0; o < plane && err == 0; o++)
            if (k != 0 ? a[o] != -1 : (a[o] < 0 || a[o] >= mods[m])) err++;
    }
    info[0] = (int32_t)lds; info[1] = launched; info[2] = singular; info[3] = err;
    if (err != 0) return modp_fail(CLRS_ERR_HIP, who + ": " + std::to_string(err) + " pivots, determinants or entries that are no residues");
    std::copy(h_adj.begin(), h_adj.end(), adj);
    std::copy(h_det.begin(), h_det.end(), det);
    std::copy(h_break.begin(), h_break.end(), breakdown);
    return 0;
}

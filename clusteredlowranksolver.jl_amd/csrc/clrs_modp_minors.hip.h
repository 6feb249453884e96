// clrs_modp_minors.hip.h -- the leading principal minors of a symmetric integer matrix mod many primes (clrs_modp_minors, include/clrs_hip.h; DESIGN.md
// section 17): the device half of an exact positive-definiteness check, the step of the reference's is_valid_solution (src/rounding.jl:367-415) that asks
// Arb for a ball-arithmetic Cholesky (checkpd_cholesky, :447-472).  A symmetric integer matrix M is positive definite iff its n leading principal minors
// are positive; minor k is an integer bounded by Hadamard, so it is determined by its residues mod enough primes; and mod one prime p the minors are the
// running products of the pivots of the elimination M = L D L^T WITHOUT exchanges (an exchange would change which minors are computed).  The primes are
// independent of each other: one workgroup per prime.  Included at the end of clrs_modp.hip, whose ModpBufs, modp_fail and MODPCHECK it uses.
//
//   k_minors_residues   the lower triangle of M mod every prime of a chunk, fp64 residues, one n x n matrix per prime (row-major; the strict upper triangle
//                       is neither written nor read).  One wave per entry (i, j), j <= i, and per MINORS_RES_GROUPS x 64 primes of the chunk, the lanes
//                       across the primes: the digits of the entry are fetched 64 at a time, one per lane, and handed round by shuffles, so an entry's
//                       digits are read once per 256 primes.  Horner from the top digit: acc <- (acc 2^24 + d + c) mod p with c = p ceil(2^23 / p), the
//                       smallest multiple of p that makes a balanced digit d in [-2^23, 2^23] non-negative; acc 2^24 + d + c < 2^47 + 2^25, exact in fp64.
//   k_minors_ldl        one workgroup (MINORS_NT threads, one wave per SIMD) per prime, the matrix resident in LDS (dynamic, sized by n): rows padded
//                       to npad = 16 ceil(n / 16), row stride npad + 1, the padding zero; beside it W (npad x 17).  Right-looking, 16 columns per panel.
//                       In a panel, per column j: the pivot d = A[j, j]; the minor is the running product of the pivots; d = 0 ends the prime's work
//                       (breakdown = j + 1, the minors behind it -1); otherwise ONE modp_inv, W[i, t] = -A[i, j] / d for the rows below, and the rank-1
//                       step A[i, j'] += W[i, t] A[j', j] on the panel's columns j' > j (rows i >= j').  After the panel the symmetric trailing update
//                       A22 <- A22 + W C^T (W = -L21, C = L21 D, the panel's columns as the steps left them) on the 16 x 16 tiles of the lower
//                       triangle, one tile per wave at a time: four v_mfma_f64_16x16x4 and ONE modp_reduce per entry.
//
// Exactness of the trailing update: an entry is one residue plus 16 products of residues, at most (p - 1) + 16 (p - 1)^2 < 2^50 < 2^53 for p < 2^23, so
// the fp64 sum is the exact integer in any order of summation (the argument of k_modp_update, clrs_modp_arith.h) and one reduction afterwards is enough.
// The rank-1 step: a residue plus one product, below 2^46.
//
// Masks, not other code paths: a trailing update runs only behind a FULL panel (c0 + 16 < n), so its k-extent is always 16; the last panel of an n that is
// no multiple of 16, and n < 16, walk the same column loop over w = n - c0 < 16 columns; tiles that reach past n read the zero padding (W and A rows >= n are
// never written) and store only where row < n; diagonal tiles load and store only col <= row.
//
// The residue buffer of a chunk of primes is at most MINORS_CHUNK_BYTES (256 MiB; clrs_config_set("modp_minors_chunk_bytes", b) lowers it, for the tests):
// at n = 128 a matrix is 128 KiB, 2048 primes per chunk.
#pragma once

#define MINORS_NT 256                 // threads of a workgroup of either kernel: four waves
#define MINORS_WAVES (MINORS_NT / 64)
#define MINORS_RES_GROUPS 4           // k_minors_residues: a wave takes 4 x 64 primes of the chunk
#define MINORS_WLD 17                 // row stride of W in LDS
#define MINORS_CHUNK_BYTES ((size_t)256 << 20)
#define MINORS_MAX_DIGITS 32767
#define MINORS_MAX_PRIMES 65535

extern int g_cfg_modp_minors_chunk_bytes;      // clrs_hip.hip, clrs_config_set("modp_minors_chunk_bytes", bytes): 0 = MINORS_CHUNK_BYTES

// the row i and column j <= i of entry e of a lower triangle stored row after row: e = i (i + 1) / 2 + j
__device__ inline void minors_tri(int e, int &i, int &j) {
    i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= e) i++;
    while (i * (i + 1) / 2 > e) i--;
    j = e - i * (i + 1) / 2;
}

// R[q, i, j] = M[i, j] mod primes[q] for j <= i and the pc primes of the chunk; digits [nd][n][n], primes [pc], R [pc][n][n]
__global__ __launch_bounds__(MINORS_NT) void k_minors_residues(const int32_t *__restrict__ digits, int n, int nd, const int32_t *__restrict__ primes, int pc,
                                                               double *__restrict__ R) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * MINORS_WAVES + (threadIdx.x >> 6);
    if (e >= n * (n + 1) / 2) return;                                                      // (wave-uniform)
    int i, j;
    minors_tri(e, i, j);
    const int q0 = blockIdx.y * (64 * MINORS_RES_GROUPS);
    double p[MINORS_RES_GROUPS], pinv[MINORS_RES_GROUPS], off[MINORS_RES_GROUPS], acc[MINORS_RES_GROUPS];
#pragma unroll
    for (int g = 0; g < MINORS_RES_GROUPS; g++) {
        const int q = q0 + 64 * g + lane;
        p[g] = q < pc ? (double)primes[q] : 2.0;
        pinv[g] = 1.0 / p[g];
        off[g] = p[g] * ceil(8388608.0 / p[g]);                                            // a multiple of p in [2^23, 2^24)
        acc[g] = 0.0;
    }
    const size_t plane = (size_t)n * n;
    const int32_t *src = digits + (size_t)i * n + j;
    for (int top = nd - 1; top >= 0; top -= 64) {
        const int l = top - lane;
        const int dig = l >= 0 ? src[(size_t)l * plane] : 0;
        const int cnt = top + 1 < 64 ? top + 1 : 64;
        for (int t = 0; t < cnt; t++) {
            const double d = (double)__shfl(dig, t, 64);
#pragma unroll
            for (int g = 0; g < MINORS_RES_GROUPS; g++) acc[g] = modp_reduce(fma(acc[g], 16777216.0, d + off[g]), p[g], pinv[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < MINORS_RES_GROUPS; g++) {
        const int q = q0 + 64 * g + lane;
        if (q < pc) R[(size_t)q * plane + (size_t)i * n + j] = acc[g];
    }
}

// Prime q0 + blockIdx.x: R is the chunk's residues (matrix blockIdx.x), minors [nprimes][n], breakdown [nprimes]; *err counts pivots that are no residues
__global__ __launch_bounds__(MINORS_NT) void k_minors_ldl(const double *__restrict__ R, int n, int npad, const int32_t *__restrict__ primes, int q0,
                                                          int32_t *__restrict__ minors, int32_t *__restrict__ breakdown, int *__restrict__ err) {
    extern __shared__ double s_minors[];
    const int LD = npad + 1;
    double *A = s_minors, *W = s_minors + npad * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4, t16 = tid & 15, sub = tid >> 4;
    const int q = q0 + blockIdx.x, p_int = primes[q];
    const double p = (double)p_int, pinv = 1.0 / p;
    const double *Rq = R + (size_t)blockIdx.x * n * n;
    int32_t *mq = minors + (size_t)q * n;
    for (int o = tid; o < npad * (LD + MINORS_WLD); o += MINORS_NT) s_minors[o] = 0.0;
    __syncthreads();
    for (int o = tid; o < n * n; o += MINORS_NT) {
        const int i = o / n, j = o - i * n;
        if (j <= i) A[i * LD + j] = Rq[o];
    }
    __syncthreads();
    double prod = 1.0;
    for (int c0 = 0; c0 < n; c0 += 16) {
        const int w = n - c0 < 16 ? n - c0 : 16;
        for (int t = 0; t < w; t++) {
            const int j = c0 + t;
            const double d = A[j * LD + j];                                                // (every thread: the same LDS word)
            if (tid == 0 && !(d >= 0.0 && d < p && d == floor(d))) atomicAdd(err, 1);
            prod = modp_mul(prod, d, p, pinv);
            if (tid == 0) mq[j] = (int32_t)prod;
            if (d == 0.0) {                                                                // (uniform) minor j + 1 is 0 mod p: nothing behind it is defined
                for (int k = j + 1 + tid; k < n; k += MINORS_NT) mq[k] = -1;
                if (tid == 0) breakdown[q] = j + 1;
                return;
            }
            if (j == n - 1) break;
            const double dinv = modp_inv(d, p_int);                                        // (every thread for itself: no hand-over, no barrier)
            for (int i = j + 1 + tid; i < n; i += MINORS_NT) W[i * MINORS_WLD + t] = modp_neg(modp_mul(A[i * LD + j], dinv, p, pinv), p);
            __syncthreads();
            if (t16 > t && t16 < w) {                                                      // column c0 + t16 of the panel, rows from its diagonal down
                const int jc = c0 + t16;
                const double cj = A[jc * LD + j];
                for (int i = j + 1 + sub; i < n; i += MINORS_NT / 16)
                    if (i >= jc) A[i * LD + jc] = modp_reduce(fma(W[i * MINORS_WLD + t], cj, A[i * LD + jc]), p, pinv);
            }
            __syncthreads();
        }
        const int c1 = c0 + 16;
        if (c1 >= n) break;
        // A22 <- A22 + W C^T on the lower triangle's tiles; C = the panel's columns (not written here), W rows >= n zero
        const int nt = (npad - c1) / 16, ntiles = nt * (nt + 1) / 2;
        for (int tile = wave; tile < ntiles; tile += MINORS_WAVES) {
            int bi, bj;
            minors_tri(tile, bi, bj);
            const int r0 = c1 + 16 * bi, s0 = c1 + 16 * bj;
            // operands: A-side lane l holds W[r0 + (l & 15), 4 kk + (l >> 4)], B-side lane l holds C[s0 + (l & 15), 4 kk + (l >> 4)]
            double av[4], bv[4];
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                av[kk] = W[(r0 + l15) * MINORS_WLD + 4 * kk + l4];
                bv[kk] = A[(s0 + l15) * LD + c0 + 4 * kk + l4];
            }
            // accumulator: column l & 15, row (l >> 4) + 4 reg
            const int col = s0 + l15;
            modp_v4d acc;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = r0 + l4 + 4 * reg;
                acc[reg] = col <= row ? A[row * LD + col] : 0.0;
            }
#pragma unroll
            for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bv[kk], acc, 0, 0, 0);
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = r0 + l4 + 4 * reg;
                if (col <= row && row < n) A[row * LD + col] = modp_reduce(acc[reg], p, pinv);
            }
        }
        __syncthreads();
    }
}

static size_t minors_lds_bytes(int n) {
    const size_t npad = (size_t)((n + 15) / 16) * 16;
    return npad * (npad + 1 + MINORS_WLD) * sizeof(double);
}

static thread_local double g_minors_ms[3] = {0.0, 0.0, 0.0};

// the device times of this thread's last clrs_modp_minors: milliseconds in k_minors_residues, in k_minors_ldl, and from the first upload to the last download
extern "C" int clrs_modp_minors_times(double *residues_ms, double *ldl_ms, double *total_ms) {
    if (!residues_ms || !ldl_ms || !total_ms) return modp_fail(CLRS_ERR_INVALID, "modp_minors_times: null argument");
    *residues_ms = g_minors_ms[0];
    *ldl_ms = g_minors_ms[1];
    *total_ms = g_minors_ms[2];
    return 0;
}

// What clrs_modp_minors and clrs_modp_minors_field (clrs_modp_minors_field.hip.h) refuse alike, before any device call: `who` heads the message.
// digits: `planes` row-major n x n planes of balanced digits, each symmetric
static int minors_check_digits(const std::string &who, int n, size_t planes, const int32_t *digits) {
    const size_t plane = (size_t)n * n;
    for (size_t o = 0; o < planes * plane; o++)
        if (digits[o] < -(1 << 23) || digits[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, who + ": a digit outside [-2^23, 2^23]");
    for (size_t l = 0; l < planes; l++)
        for (int i = 0; i < n; i++)
            for (int j = 0; j < i; j++)
                if (digits[l * plane + (size_t)i * n + j] != digits[l * plane + (size_t)j * n + i])
                    return modp_fail(CLRS_ERR_INVALID, who + ": the digit planes are not symmetric");
    return 0;
}

static int minors_check_primes(const std::string &who, int nprimes, const int32_t *primes) {
    std::vector<int32_t> sorted(primes, primes + nprimes);
    std::sort(sorted.begin(), sorted.end());
    for (int q = 0; q < nprimes; q++) {
        const int v = sorted[q];
        if (!modp_prime_ok(v)) return modp_fail(CLRS_ERR_INVALID, who + ": every modulus must be a prime with 2 <= p < 2^23");
        if (q > 0 && sorted[q - 1] == v) return modp_fail(CLRS_ERR_INVALID, who + ": a repeated prime");
    }
    return 0;
}

// What k_minors_ldl left for `count` matrices (matrix q eliminated mod primes[q]): the counters into info, and, unless an impossibility was met (a
// breakdown outside [0, n], a residue where none belongs: CLRS_ERR_HIP, the caller's arrays untouched), the rows into the caller's arrays.
static int minors_deliver(const std::string &who, int n, int count, const int32_t *primes, const std::vector<int32_t> &h_minors, const std::vector<int32_t> &h_break,
                          int err, size_t lds, int launched, int32_t *minors, int32_t *breakdown, int32_t *info) {
    int broke = 0;
    for (int q = 0; q < count; q++) {
        const int k = h_break[q];
        if (k != 0) broke++;
        if (k < 0 || k > n) err++;
        for (int j = 0; j < n && err == 0; j++) {                                          // a residue where one belongs, -1 behind a breakdown
            const int32_t v = h_minors[(size_t)q * n + j];
            if (k != 0 && j >= k ? v != -1 : (v < 0 || v >= primes[q] || (k != 0 && j == k - 1 && v != 0))) err++;
        }
    }
    info[0] = (int32_t)lds; info[1] = launched; info[2] = broke; info[3] = err;
    if (err != 0) return modp_fail(CLRS_ERR_HIP, who + ": " + std::to_string(err) + " pivots or minors that are no residues");
    std::copy(h_minors.begin(), h_minors.end(), minors);
    std::copy(h_break.begin(), h_break.end(), breakdown);
    return 0;
}

// The device half of clrs_modp_minors and clrs_modp_minors_field: `count` matrices of residues, matrix m eliminated mod mods[m] (a host array), `chunk`
// of them resident at a time.  upload(bufs) allocates and fills what the residue launch reads; residues(m0, mc, d_mods, d_R) launches the kernel that
// fills d_R with the matrices m0 .. m0 + mc - 1 (d_mods: the device copy of mods).  ms receives the times of clrs_modp_minors_times.
template <class Upload, class Residues>
static int minors_run(const std::string &who, int device, int n, int count, int chunk, const int32_t *mods, Upload upload, Residues residues, double *ms_out,
                      int32_t *minors, int32_t *breakdown, int32_t *info) {
    const size_t plane = (size_t)n * n;
    const int npad = (n + 15) / 16 * 16;
    const size_t lds = minors_lds_bytes(n);

    MODPCHECK(hipSetDevice(device));
    if (lds > 48 * 1024) MODPCHECK(hipFuncSetAttribute((const void *)k_minors_ldl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ModpBufs bufs;
    int32_t *d_mods = nullptr, *d_minors = nullptr, *d_break = nullptr;
    double *d_R = nullptr;
    int *d_err = nullptr;
    MODPCHECK(bufs.get(&d_mods, (size_t)count)); MODPCHECK(bufs.get(&d_R, (size_t)chunk * plane));
    MODPCHECK(bufs.get(&d_minors, (size_t)count * n)); MODPCHECK(bufs.get(&d_break, (size_t)count)); MODPCHECK(bufs.get(&d_err, (size_t)1));
    ModpEvents ev(5);
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    MODPCHECK(hipEventRecord(ev.e[3], nullptr));
    if (int code = upload(bufs)) return code;
    MODPCHECK(hipMemcpy(d_mods, mods, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_minors, 0xff, (size_t)count * n * sizeof(int32_t)));
    MODPCHECK(hipMemset(d_break, 0, (size_t)count * sizeof(int32_t)));
    MODPCHECK(hipMemset(d_err, 0, sizeof(int)));
    double ms[2] = {0.0, 0.0};
    int launched = 0;
    for (int m0 = 0; m0 < count; m0 += chunk) {
        const int mc = std::min(chunk, count - m0);
        MODPCHECK(hipEventRecord(ev.e[0], nullptr));
        residues(m0, mc, d_mods, d_R);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(k_minors_ldl, dim3((unsigned)mc), dim3(MINORS_NT), lds, nullptr, d_R, n, npad, d_mods, m0, d_minors, d_break, d_err);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[2], nullptr));
        MODPCHECK(hipEventSynchronize(ev.e[2]));
        float a = 0.f, b = 0.f;
        MODPCHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        ms[0] += a; ms[1] += b;
        launched += mc;
    }
    int err = 0;
    std::vector<int32_t> h_minors((size_t)count * n), h_break((size_t)count);          // the caller's arrays are written only by a call that succeeds
    MODPCHECK(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_minors.data(), d_minors, h_minors.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_break.data(), d_break, h_break.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipEventRecord(ev.e[4], nullptr));
    MODPCHECK(hipEventSynchronize(ev.e[4]));
    float total = 0.f;
    MODPCHECK(hipEventElapsedTime(&total, ev.e[3], ev.e[4]));
    ms_out[0] = ms[0]; ms_out[1] = ms[1]; ms_out[2] = total;
    return minors_deliver(who, n, count, mods, h_minors, h_break, err, lds, launched, minors, breakdown, info);
}

extern "C" int clrs_modp_minors(int device, int n, int nd, const int32_t *digits, int nprimes, const int32_t *primes, int32_t *minors, int32_t *breakdown,
                                int32_t *info) {
    if (n < 1 || n > CLRS_MODP_MINORS_MAX_N) return modp_fail(CLRS_ERR_INVALID, "modp_minors: n must lie in [1, 128]");
    if (nd < 1 || nd > MINORS_MAX_DIGITS) return modp_fail(CLRS_ERR_INVALID, "modp_minors: nd must lie in [1, 32767]");
    if (nprimes < 1 || nprimes > MINORS_MAX_PRIMES) return modp_fail(CLRS_ERR_INVALID, "modp_minors: nprimes must lie in [1, 65535]");
    if (!digits || !primes || !minors || !breakdown || !info) return modp_fail(CLRS_ERR_INVALID, "modp_minors: null argument");
    const size_t plane = (size_t)n * n;
    if (int code = minors_check_digits("modp_minors", n, (size_t)nd, digits)) return code;
    if (int code = minors_check_primes("modp_minors", nprimes, primes)) return code;
    const size_t bound = modp_chunk_bound(g_cfg_modp_minors_chunk_bytes, MINORS_CHUNK_BYTES);
    const int chunk = (int)std::min<size_t>((size_t)nprimes, std::max<size_t>(bound / (plane * sizeof(double)), 1));
    const int ne = n * (n + 1) / 2;
    int32_t *d_digits = nullptr;
    auto upload = [&](ModpBufs &bufs) -> int {
        MODPCHECK(bufs.get(&d_digits, (size_t)nd * plane));
        MODPCHECK(hipMemcpy(d_digits, digits, (size_t)nd * plane * sizeof(int32_t), hipMemcpyHostToDevice));
        return 0;
    };
    auto residues = [&](int q0, int pc, const int32_t *d_primes, double *d_R) {
        hipLaunchKernelGGL(k_minors_residues, dim3((unsigned)((ne + MINORS_WAVES - 1) / MINORS_WAVES), (unsigned)((pc + 64 * MINORS_RES_GROUPS - 1) / (64 * MINORS_RES_GROUPS))),
                           dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_primes + q0, pc, d_R);
    };
    return minors_run("modp_minors", device, n, nprimes, chunk, primes, upload, residues, g_minors_ms, minors, breakdown, info);
}

// clrs_modp_minors_field.hip.h -- the leading principal minors of a symmetric matrix over a number field QQ(g), mod many primes (clrs_modp_minors_field,
// clrs_modp_field_frobenius, include/clrs_hip.h): the device half of an exact positive-definiteness check over the field, where the
// reference's checkpd_cholesky(A; FF, g) (src/rounding.jl:417-472) embeds the block at Arb balls of the root and doubles the precision until it gives up.
// The matrix is M = sum_j M_j g^j with integer M_j and f, the minimal polynomial of g, monic of degree D.  At a prime p where f has D distinct roots
// r_1 .. r_D, g -> r_i is a ring map Z[g] -> F_p, so the leading minors of the integer residue matrix M(r_i) mod p are the images of the minors of M; the
// D images give the D coefficients of a minor mod p (a Vandermonde solve, on the host).  Included at the end of clrs_modp.hip after clrs_modp_minors.hip.h,
// whose k_minors_ldl, minors_run and checks it uses unchanged.
//
//   k_minors_residues_field<D>   the lower triangles of the D matrices M(r_i) mod p for every prime of a chunk: the layout of k_minors_residues (one wave per
//                       entry, the lanes across MINORS_RES_GROUPS x 64 primes, the digits fetched 64 at a time and handed round by shuffles).  A lane first
//                       reduces the D coefficients of its entry mod its prime, ONCE each, by the same Horner and offset over the digits; then it evaluates
//                       at its D roots (ff_residue) and writes D residues, matrix q D + i for the pair (prime q, root i).
//   k_field_frobenius<D>  one lane per prime: x^p mod (f, p) by FF_FROBENIUS_BITS steps of square and multiply, the multiply selected, not branched
//                       (ff_frobenius, clrs_modp_field_arith.h).  A prime splits f completely iff the result is x (and p divides neither lc(f) nor disc(f)).
#pragma once
#include "clrs_modp_field_arith.h"

#define FIELD_FROBENIUS_MAX_PRIMES (1 << 20)        // primes of one call of clrs_modp_field_frobenius: every prime below 2^23 (564163) fits

// R[q D + i, r, c] = sum_j M_j[r, c] roots[q D + i]^j mod p_q for c <= r; digits [D][nd][n][n], mods [pc D] (prime q stands at q D .. q D + D - 1),
// roots [pc D], R [pc D][n][n]
template <int D>
__global__ __launch_bounds__(MINORS_NT) void k_minors_residues_field(const int32_t *__restrict__ digits, int n, int nd, const int32_t *__restrict__ mods,
                                                                     const int32_t *__restrict__ roots, int pc, double *__restrict__ R) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * MINORS_WAVES + (threadIdx.x >> 6);
    if (e >= n * (n + 1) / 2) return;                                                      // (wave-uniform)
    int i, j;
    minors_tri(e, i, j);
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
        const int32_t *src = digits + (size_t)c * nd * plane + (size_t)i * n + j;
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
            for (int t = 0; t < D; t++)
                R[((size_t)q * D + t) * plane + (size_t)i * n + j] = ff_residue<D>(acc[g], (double)roots[(size_t)q * D + t], p[g], pinv[g]);
        }
    }
}

// out[q, 0 .. D - 1] = the coefficients of x^p mod (f, p) for p = primes[q], or -1 throughout where p divides the leading coefficient; f [D + 1] low to high
template <int D>
__global__ __launch_bounds__(MINORS_NT) void k_field_frobenius(const long long *__restrict__ f, const int32_t *__restrict__ primes, int nprimes,
                                                               int32_t *__restrict__ out) {
    const int q = blockIdx.x * MINORS_NT + threadIdx.x;
    if (q >= nprimes) return;
    const int p_int = primes[q];
    const double p = (double)p_int, pinv = 1.0 / p;
    double fp[D + 1], xr[D - 1][D], res[D];
#pragma unroll
    for (int j = 0; j <= D; j++) {
        const long long v = f[j] % (long long)p_int;
        fp[j] = (double)(v < 0 ? v + p_int : v);
    }
    const bool monic = fp[D] != 0.0;
    ff_fold_table<D>(fp, monic ? modp_inv(fp[D], p_int) : 0.0, p, pinv, xr);               // (lc = 0: a table of zeros, the result is discarded)
    ff_frobenius<D>(p_int, xr, p, pinv, res);
#pragma unroll
    for (int j = 0; j < D; j++) out[(size_t)q * D + j] = monic ? (int32_t)res[j] : -1;
}

static thread_local double g_minors_field_ms[3] = {0.0, 0.0, 0.0};

// the device times of this thread's last clrs_modp_minors_field, as clrs_modp_minors_times gives them
extern "C" int clrs_modp_minors_field_times(double *residues_ms, double *ldl_ms, double *total_ms) {
    if (!residues_ms || !ldl_ms || !total_ms) return modp_fail(CLRS_ERR_INVALID, "modp_minors_field_times: null argument");
    *residues_ms = g_minors_field_ms[0];
    *ldl_ms = g_minors_field_ms[1];
    *total_ms = g_minors_field_ms[2];
    return 0;
}

extern "C" int clrs_modp_minors_field(int device, int n, int deg, int nd, const int32_t *digits, int nprimes, const int32_t *primes, const int32_t *roots,
                                      int32_t *minors, int32_t *breakdown, int32_t *info) {
    const std::string who = "modp_minors_field";
    if (deg < FF_MIN_DEG || deg > FF_MAX_DEG) return modp_fail(CLRS_ERR_INVALID, who + ": deg must lie in [2, 4]");
    if (n < 1 || n > CLRS_MODP_MINORS_MAX_N) return modp_fail(CLRS_ERR_INVALID, who + ": n must lie in [1, 128]");
    if (nd < 1 || nd > MINORS_MAX_DIGITS) return modp_fail(CLRS_ERR_INVALID, who + ": nd must lie in [1, 32767]");
    if (nprimes < 1 || nprimes > MINORS_MAX_PRIMES) return modp_fail(CLRS_ERR_INVALID, who + ": nprimes must lie in [1, 65535]");
    if (!digits || !primes || !roots || !minors || !breakdown || !info) return modp_fail(CLRS_ERR_INVALID, who + ": null argument");
    const size_t plane = (size_t)n * n;
    if (int code = minors_check_digits(who, n, (size_t)deg * nd, digits)) return code;
    if (int code = minors_check_primes(who, nprimes, primes)) return code;
    for (int q = 0; q < nprimes; q++)
        for (int t = 0; t < deg; t++) {
            const int32_t r = roots[(size_t)q * deg + t];
            if (r < 0 || r >= primes[q]) return modp_fail(CLRS_ERR_INVALID, who + ": a root outside [0, p)");
            for (int u = 0; u < t; u++)
                if (roots[(size_t)q * deg + u] == r) return modp_fail(CLRS_ERR_INVALID, who + ": two equal roots of one prime");
        }
    std::vector<int32_t> mods((size_t)nprimes * deg);                                       // every prime deg times: the modulus of matrix q deg + t
    for (size_t m = 0; m < mods.size(); m++) mods[m] = primes[m / deg];
    const size_t bound = modp_chunk_bound(g_cfg_modp_minors_chunk_bytes, MINORS_CHUNK_BYTES);
    const int chunk = (int)std::min<size_t>((size_t)nprimes, std::max<size_t>(bound / (plane * sizeof(double) * deg), 1));      // in primes: 8 n^2 deg bytes each
    const int ne = n * (n + 1) / 2;
    int32_t *d_digits = nullptr, *d_roots = nullptr;
    auto upload = [&](ModpBufs &bufs) -> int {
        MODPCHECK(bufs.get(&d_digits, (size_t)deg * nd * plane)); MODPCHECK(bufs.get(&d_roots, (size_t)nprimes * deg));
        MODPCHECK(hipMemcpy(d_digits, digits, (size_t)deg * nd * plane * sizeof(int32_t), hipMemcpyHostToDevice));
        MODPCHECK(hipMemcpy(d_roots, roots, (size_t)nprimes * deg * sizeof(int32_t), hipMemcpyHostToDevice));
        return 0;
    };
    auto residues = [&](int m0, int mc, const int32_t *d_mods, double *d_R) {              // matrices m0 .. m0 + mc - 1 = the primes m0 / deg .. of the chunk
        const int pc = mc / deg;
        const dim3 grid((unsigned)((ne + MINORS_WAVES - 1) / MINORS_WAVES), (unsigned)((pc + 64 * MINORS_RES_GROUPS - 1) / (64 * MINORS_RES_GROUPS)));
        if (deg == 2) hipLaunchKernelGGL(k_minors_residues_field<2>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
        if (deg == 3) hipLaunchKernelGGL(k_minors_residues_field<3>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
        if (deg == 4) hipLaunchKernelGGL(k_minors_residues_field<4>, grid, dim3(MINORS_NT), 0, nullptr, d_digits, n, nd, d_mods + m0, d_roots + m0, pc, d_R);
    };
    return minors_run(who, device, n, nprimes * deg, chunk * deg, mods.data(), upload, residues, g_minors_field_ms, minors, breakdown, info);
}

// the primes below 2^23, sieved once: clrs_modp_field_frobenius takes every one of them in a call, too many for trial division each
static const std::vector<bool> &field_prime_sieve() {
    static const std::vector<bool> sieve = [] {
        std::vector<bool> s((size_t)1 << MODP_MAX_PRIME_BITS, true);
        s[0] = s[1] = false;
        for (size_t d = 2; d * d < s.size(); d++)
            if (s[d])
                for (size_t m = d * d; m < s.size(); m += d) s[m] = false;
        return s;
    }();
    return sieve;
}

extern "C" int clrs_modp_field_frobenius(int device, int deg, const int64_t *minpoly, int nprimes, const int32_t *primes, int32_t *out) {
    const std::string who = "modp_field_frobenius";
    if (deg < FF_MIN_DEG || deg > FF_MAX_DEG) return modp_fail(CLRS_ERR_INVALID, who + ": deg must lie in [2, 4]");
    if (nprimes < 1 || nprimes > FIELD_FROBENIUS_MAX_PRIMES) return modp_fail(CLRS_ERR_INVALID, who + ": nprimes must lie in [1, 2^20]");
    if (!minpoly || !primes || !out) return modp_fail(CLRS_ERR_INVALID, who + ": null argument");
    if (minpoly[deg] == 0) return modp_fail(CLRS_ERR_INVALID, who + ": the leading coefficient is zero");
    const std::vector<bool> &sieve = field_prime_sieve();
    for (int q = 0; q < nprimes; q++)
        if (primes[q] < 2 || primes[q] >= (1 << MODP_MAX_PRIME_BITS) || !sieve[(size_t)primes[q]])
            return modp_fail(CLRS_ERR_INVALID, who + ": every modulus must be a prime with 2 <= p < 2^23");
    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    long long *d_f = nullptr;
    int32_t *d_primes = nullptr, *d_out = nullptr;
    MODPCHECK(bufs.get(&d_f, (size_t)deg + 1)); MODPCHECK(bufs.get(&d_primes, (size_t)nprimes)); MODPCHECK(bufs.get(&d_out, (size_t)nprimes * deg));
    long long f[FF_MAX_DEG + 1];
    for (int j = 0; j <= deg; j++) f[j] = (long long)minpoly[j];
    MODPCHECK(hipMemcpy(d_f, f, ((size_t)deg + 1) * sizeof(long long), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_primes, primes, (size_t)nprimes * sizeof(int32_t), hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((nprimes + MINORS_NT - 1) / MINORS_NT));
    if (deg == 2) hipLaunchKernelGGL(k_field_frobenius<2>, grid, dim3(MINORS_NT), 0, nullptr, d_f, d_primes, nprimes, d_out);
    if (deg == 3) hipLaunchKernelGGL(k_field_frobenius<3>, grid, dim3(MINORS_NT), 0, nullptr, d_f, d_primes, nprimes, d_out);
    if (deg == 4) hipLaunchKernelGGL(k_field_frobenius<4>, grid, dim3(MINORS_NT), 0, nullptr, d_f, d_primes, nprimes, d_out);
    MODPCHECK(hipGetLastError());
    std::vector<int32_t> h_out((size_t)nprimes * deg);                                      // the caller's array is written only by a call that succeeds
    MODPCHECK(hipMemcpy(h_out.data(), d_out, h_out.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::copy(h_out.begin(), h_out.end(), out);
    return 0;
}

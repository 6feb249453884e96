// Host build of the arithmetic of the exact integer matrix product (csrc/clrs_modp_zz_arith.h): the SAME zz_split / zz_flush / zz_pair_bad / zz_carry_walk the
// kernels of clrs_modp_zz_gemm.hip.h call, and a whole product built from them the way the kernels are (plain loops where the kernels tile).  Test
// infrastructure; compiled by tests/zz_util.py (g++ -O2 -std=c++17) as a shared library, and with -DZZ_HOST_MAIN -fsanitize=address,undefined as a stand-alone
// program that checks itself against __int128 arithmetic.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_zz_arith.h"

#define ZZH_BK 16                                             // k-extent of a step of k_zz_gemm
#define ZZH_FLUSH_STEPS (ZZ_FLUSH_MFMAS / (ZZH_BK / 4))

extern "C" int zz_constants_host(int *out) {
    out[0] = ZZ_MAX_FLUSH_MFMAS; out[1] = ZZ_FLUSH_MFMAS; out[2] = ZZH_FLUSH_STEPS; out[3] = ZZ_DIGIT_BITS;
    return 0;
}

extern "C" int zz_split_host(int count, const double *acc, double *lo, double *c, int *bad) {
    for (int i = 0; i < count; i++) {
        c[i] = zz_split(acc[i], &lo[i]);
        bad[i] = zz_pair_bad(lo[i], c[i]);
    }
    return 0;
}

// One flush cycle: an accumulator that holds `rem`, then nmfma MFMAs of k-extent 4 (products a[4 f + q] b[4 f + q] added in order), then the flush.
// out: [0] the accumulator before the flush, [1] lo, [2] hi after it (hi started at hi0)
extern "C" int zz_flush_cycle_host(int nmfma, const int32_t *a, const int32_t *b, double rem, double hi0, double *out) {
    double acc = rem, hi = hi0;
    for (int f = 0; f < nmfma; f++)
        for (int q = 0; q < 4; q++) acc = fma((double)a[4 * f + q], (double)b[4 * f + q], acc);
    out[0] = acc;
    zz_flush(&acc, &hi);
    out[1] = acc; out[2] = hi;
    return zz_pair_bad(acc, hi);
}

// S: count entries of ns sums each (entry e at S + e * ns); C: count entries of ndc digits each; returns the number of entries that do not fit
extern "C" int zz_carry_host(int count, int ns, const long long *S, int ndc, int32_t *C) {
    int over = 0;
    for (int e = 0; e < count; e++) over += zz_carry_walk(S + (size_t)e * ns, 1, ns, C + (size_t)e * ndc, 1, ndc);
    return over;
}

// The whole product as clrs_zz_gemm forms it: A [nda][m][k], B [ndb][k][n], C [ndc][m][n]; `dc` digits of B per range.  info as the C function's ([2] = 0).
// Returns 0, -1 when an entry does not fit (C untouched), -2 for an impossibility.
extern "C" int zz_gemm_host(int m, int k, int n, int nda, const int32_t *A, int ndb, const int32_t *B, int ndc, int32_t *C, int dc, int32_t *info) {
    const size_t mn = (size_t)m * n, M = (size_t)nda * m, ldb = (size_t)ndb * n;
    const int ns = nda + ndb;
    std::vector<double> Ad((size_t)nda * m * k), Bp((size_t)k * ldb);
    for (size_t o = 0; o < Ad.size(); o++) Ad[o] = (double)A[o];                            // k_zz_widen
    for (int t = 0; t < ndb; t++)
        for (int kk = 0; kk < k; kk++)
            for (int j = 0; j < n; j++) Bp[(size_t)kk * ldb + (size_t)t * n + j] = (double)B[((size_t)t * k + kk) * n + j];
    std::vector<long long> S((size_t)ns * mn, 0ll);
    int bad = 0, chunks = 0;
    const int nsteps = (k + ZZH_BK - 1) / ZZH_BK;
    for (int t0 = 0; t0 < ndb; t0 += dc, chunks++) {
        const int t1 = std::min(t0 + dc, ndb);
        const size_t N = (size_t)(t1 - t0) * n, c0 = (size_t)t0 * n;
        std::vector<double> lo(M * N), hi(M * N);
        for (size_t r = 0; r < M; r++)                                                     // k_zz_gemm
            for (size_t c = 0; c < N; c++) {
                double acc = 0.0, h = 0.0;
                for (int step = 0; step < nsteps; step++) {
                    for (int q = 0; q < ZZH_BK; q++) {
                        const int kk = step * ZZH_BK + q;
                        if (kk < k) acc = fma(Ad[r * k + kk], Bp[(size_t)kk * ldb + c0 + c], acc);
                    }
                    if ((step + 1) % ZZH_FLUSH_STEPS == 0) zz_flush(&acc, &h);
                }
                zz_flush(&acc, &h);
                bad += zz_pair_bad(acc, h);
                lo[r * N + c] = acc; hi[r * N + c] = h;
            }
        for (int s = t0; s <= t1 + nda - 1; s++)                                           // k_zz_combine
            for (size_t e = 0; e < mn; e++) {
                const size_t r = e / n, j = e - r * n;
                long long sum = 0;
                const int i_lo = std::max(s - t1, 0), i_hi = std::min(s - t0, nda - 1);
                for (int i = i_lo; i <= i_hi; i++) {
                    const size_t row = ((size_t)i * m + r) * N + j;
                    const int t = s - i;
                    if (t < t1) sum += (long long)lo[row + (size_t)(t - t0) * n];
                    if (t - 1 >= t0) sum += (long long)hi[row + (size_t)(t - 1 - t0) * n];
                }
                S[(size_t)s * mn + e] += sum;
            }
    }
    std::vector<int32_t> out((size_t)ndc * mn);
    int over = 0;
    for (size_t e = 0; e < mn; e++) over += zz_carry_walk(S.data() + e, mn, ns, out.data() + e, mn, ndc);   // k_zz_carry
    info[0] = over; info[1] = chunks; info[2] = 0; info[3] = bad;
    if (bad) return -2;
    if (over) return -1;
    std::copy(out.begin(), out.end(), C);
    return 0;
}

#ifdef ZZ_HOST_MAIN
// the stand-alone self-check: products whose exact entries fit __int128, digits drawn with the extremes +-2^23 and +-(2^23 - 1) frequent
static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned long long next_u64() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return g_state;
}
static int32_t draw_digit() {
    const unsigned long long u = next_u64();
    switch (u & 7) {
        case 0: return 1 << 23;
        case 1: return -(1 << 23);
        case 2: return (1 << 23) - 1;
        case 3: return -((1 << 23) - 1);
        default: return (int32_t)((u >> 8) % (1ull << 24)) - (1 << 23);
    }
}

static int check_case(int m, int k, int n, int nda, int ndb, int dc) {
    std::vector<int32_t> A((size_t)nda * m * k), B((size_t)ndb * k * n);
    for (auto &v : A) v = draw_digit();
    for (auto &v : B) v = draw_digit();
    const int ndc = nda + ndb + 2;
    std::vector<int32_t> C((size_t)ndc * m * n, -7);
    int32_t info[4];
    if (zz_gemm_host(m, k, n, nda, A.data(), ndb, B.data(), ndc, C.data(), dc, info) != 0) return 1;
    for (int r = 0; r < m; r++)
        for (int j = 0; j < n; j++) {
            // the exact entry by digit pairs in __int128: plane sums below 2^46 k min(nda, ndb), folded from the top (nda + ndb <= 4: below 2^120)
            __int128 exact = 0;
            for (int s = nda + ndb - 2; s >= 0; s--) {
                __int128 plane = 0;
                for (int i = 0; i < nda; i++) {
                    const int t = s - i;
                    if (t < 0 || t >= ndb) continue;
                    for (int kk = 0; kk < k; kk++)
                        plane += (__int128)A[((size_t)i * m + r) * k + kk] * (__int128)B[((size_t)t * k + kk) * n + j];
                }
                exact = exact * ((__int128)1 << 24) + plane;
            }
            __int128 got = 0;
            for (int s = ndc - 1; s >= 0; s--) {
                const int32_t d = C[((size_t)s * m + r) * n + j];
                if (d < -(1 << 23) || d >= (1 << 23)) return 2;
                got = got * ((__int128)1 << 24) + d;
            }
            if (got != exact) return 3;
        }
    // one digit too few for a value that needs them all is refused and leaves C untouched
    std::vector<int32_t> small((size_t)m * n, -7);
    std::vector<int32_t> one((size_t)m * k, 1 << 23), two((size_t)k * n, 1 << 23);
    if (zz_gemm_host(m, k, n, 1, one.data(), 1, two.data(), 1, small.data(), 1, info) != -1 || info[0] != m * n) return 4;
    for (int32_t v : small)
        if (v != -7) return 5;
    return 0;
}

int main() {
    const int shapes[][6] = {{1, 1, 1, 1, 1, 1}, {3, 5, 2, 2, 2, 1}, {3, 5, 2, 2, 2, 2}, {2, 113, 3, 1, 3, 2}, {4, 129, 1, 2, 2, 1}, {1, 500, 2, 3, 1, 1}, {5, 17, 5, 2, 2, 5}};
    for (const auto &s : shapes) {
        const int code = check_case(s[0], s[1], s[2], s[3], s[4], s[5]);
        if (code != 0) {
            std::printf("zz_host: case %d x %d x %d, digits %d x %d, %d per range: failure %d\n", s[0], s[1], s[2], s[3], s[4], s[5], code);
            return 1;
        }
    }
    // the split at the ends of the exact range and at ties
    const double probes[] = {0.0, 9007199254740991.0, -9007199254740991.0, 8388608.0, -8388608.0, 3.0 * 8388608.0, -3.0 * 8388608.0, 16777216.0 * 5.0 + 8388608.0};
    for (double v : probes) {
        double lo;
        const double c = zz_split(v, &lo);
        if (c * ZZ_BASE + lo != v || fabs(lo) > 8388608.0 || zz_pair_bad(lo, c)) {
            std::printf("zz_host: split of %.0f failed\n", v);
            return 1;
        }
    }
    std::printf("zz_host: ok\n");
    return 0;
}
#endif

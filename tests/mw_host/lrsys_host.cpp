// Host build of the index arithmetic of the low-rank system assembly (csrc/clrs_modp_lrsys_arith.h): the SAME lrsys_panels / lrsys_stride / lrsys_p_range /
// lrsys_slot / lrsys_slot_next / lrsys_value the kernel k_lrsys_tile calls, and the whole entry restated with them the way the kernel forms it: the same
// panels, the same order of the slots (four per MFMA), the same flush period, zz_flush, zz_pair_bad and zz_carry_walk of csrc/clrs_modp_zz_arith.h.  Test
// infrastructure; compiled by tests/lrsys_util.py (g++ -O2 -std=c++17) as a shared library.
#include <algorithm>
#include <vector>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_lrsys_arith.h"

extern "C" int lrsys_constants_host(int *out) {
    out[0] = LRSYS_TILE; out[1] = LRSYS_ROW_CAP; out[2] = LRSYS_FLUSH_MFMAS; out[3] = ZZ_MAX_FLUSH_MFMAS; out[4] = LRSYS_MAX_K;
    return 0;
}

extern "C" int lrsys_panels_host(int rmax, int ndu, int ndw, int *out) {
    lrsys_panels(rmax, ndu, ndw, &out[0], &out[1], &out[2]);
    out[3] = lrsys_stride(out[0] * out[1]);
    out[4] = lrsys_stride(out[0] * out[2]);
    return 0;
}

extern "C" int lrsys_stride_host(int len) { return lrsys_stride(len); }

// out: [np, plo, phi]
extern "C" int lrsys_p_range_host(int s, int p0, int dp, int q0, int dq, int *out) {
    out[0] = lrsys_p_range(s, p0, dp, q0, dq, &out[1], &out[2]);
    return 0;
}

// the (term, digit offset) of the slots lane4, lane4 + 4, ... (count of them) by one division and then lrsys_slot_next; out: [count][2]
extern "C" int lrsys_slots_host(int lane4, int np, int count, int *out) {
    int tt, pp;
    lrsys_slot(lane4, np, &tt, &pp);
    for (int k = 0; k < count; k++) {
        out[2 * k] = tt; out[2 * k + 1] = pp;
        lrsys_slot_next(np, &tt, &pp);
    }
    return 0;
}

// The whole call as clrs_zz_lowrank_system forms it: U [ndu][n][T], W [ndw][n][T], C [ndc][R][nc]; panels of tp terms, dp and dq digits (tp <= 0: lrsys_panels).
// info as the C function's ([1] = panels visited, [2] = 0).  Returns 0, -1 when an entry does not fit (C untouched), -2 for an impossibility.
extern "C" int lrsys_host(int n, int T, int R, const int32_t *rowptr, int ndu, const int32_t *U, int ndw, const int32_t *W, int nc, const int32_t *col_a,
                          const int32_t *col_b, int ndc, int32_t *C, int tp, int dp, int dq, int32_t *info) {
    const int ns = ndu + ndw - 1;
    int rmax = 1;
    for (int i = 0; i < R; i++) rmax = std::max(rmax, rowptr[i + 1] - rowptr[i]);
    if (tp <= 0) lrsys_panels(rmax, ndu, ndw, &tp, &dp, &dq);
    std::vector<int32_t> out((size_t)ndc * R * nc);
    std::vector<long long> S((size_t)ns);
    int bad = 0, over = 0, panels = 0;
    for (int i = 0; i < R; i++)
        for (int c = 0; c < nc; c++) {
            const int a = col_a[c], b = col_b[c];
            std::fill(S.begin(), S.end(), 0ll);
            for (int t0 = rowptr[i]; t0 < rowptr[i + 1]; t0 += tp) {
                const int tc = std::min(tp, rowptr[i + 1] - t0);
                for (int p0 = 0; p0 < ndu; p0 += dp) {
                    const int dpc = std::min(dp, ndu - p0);
                    for (int q0 = 0; q0 < ndw; q0 += dq) {
                        const int dqc = std::min(dq, ndw - q0);
                        panels++;
                        for (int s = p0 + q0; s <= p0 + dpc - 1 + q0 + dqc - 1; s++) {
                            int plo, phi;
                            const int np = lrsys_p_range(s, p0, dpc, q0, dqc, &plo, &phi);
                            const int slots = tc * np;
                            double acc = 0.0, hi = 0.0;
                            int mfmas = 0;
                            for (int g0 = 0; g0 < slots; g0 += 4) {
                                for (int l4 = 0; l4 < 4 && g0 + l4 < slots; l4++) {
                                    int tt, pp;
                                    lrsys_slot(g0 + l4, np, &tt, &pp);
                                    const int p = plo + pp, t = t0 + tt;
                                    acc = fma((double)U[((size_t)p * n + a) * T + t], (double)W[((size_t)(s - p) * n + b) * T + t], acc);
                                }
                                if (++mfmas == LRSYS_FLUSH_MFMAS) {
                                    mfmas = 0;
                                    zz_flush(&acc, &hi);
                                }
                            }
                            zz_flush(&acc, &hi);
                            bad += zz_pair_bad(acc, hi);
                            S[s] += lrsys_value(acc, hi, a != b);
                        }
                    }
                }
            }
            over += zz_carry_walk(S.data(), 1, ns, out.data() + (size_t)i * nc + c, (size_t)R * nc, ndc);
        }
    info[0] = over; info[1] = panels; info[2] = 0; info[3] = bad;
    if (bad) return -2;
    if (over) return -1;
    std::copy(out.begin(), out.end(), C);
    return 0;
}

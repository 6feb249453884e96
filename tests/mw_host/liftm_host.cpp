// Host build of the per-entry residual update of the lifting with a matrix of right-hand sides (liftm_entry, csrc/clrs_modp_lift_arith.h): the SAME text
// k_liftm_r of clrs_modp_liftm.hip.h calls, over arrays in the device's planar layout.  Test infrastructure; compiled by tests/dixon_multi_util.py
// (g++ -O2 -std=c++17).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_lift_arith.h"

// count entries: P [nd][count][2] doubles (lo, hi), r [(nrl + 1)][count] limbs in place, rbar[count] the residues returned, flags[count]
extern "C" int liftm_entry_host(int count, int nd, int nrl, int p, const double *P, int32_t *r, int32_t *rbar, int32_t *flags) {
    int32_t pw[64];
    if (nrl + 1 > 64) return -1;
    lift_power_table(p, nrl + 1, pw);
    for (int e = 0; e < count; e++) {
        int f;
        rbar[e] = liftm_entry(P + 2 * (size_t)e, (size_t)count, nd, r + e, (size_t)count, nrl, p, pw, &f);
        flags[e] = f;
    }
    return 0;
}

// One step of the lifting of n x m right-hand sides on the host: x = C rbar mod p in int64 (C n x n residues, rbar n x m), the row sums of every digit plane
// of A (Ad [nd][n][n]) times x split into a balanced low digit and the rest -- a pair (lo, hi) as k_zz_gemm leaves it -- and liftm_entry per entry.
// r [(nrl + 1)][n][m] limbs and rbar in place, x out, cnt[2] the two counters.  n m nd pairs on the stack of the caller's array P (scratch, [nd][n m][2]).
extern "C" int liftm_step_host(int n, int m, int nd, int nrl, int p, const int32_t *C, const int32_t *Ad, int32_t *r, int32_t *rbar, int32_t *x, double *P,
                               int *cnt) {
    int32_t pw[64];
    if (nrl + 1 > 64) return -1;
    lift_power_table(p, nrl + 1, pw);
    const size_t ce = (size_t)n * m;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) {
            long long s = 0;
            for (int c = 0; c < n; c++) s += (long long)C[(size_t)i * n + c] * rbar[(size_t)c * m + j];
            x[(size_t)i * m + j] = (int32_t)((unsigned long long)s % (unsigned long long)p);
        }
    for (int l = 0; l < nd; l++)
        for (int i = 0; i < n; i++)
            for (int j = 0; j < m; j++) {
                long long s = 0;
                for (int c = 0; c < n; c++) s += (long long)Ad[((size_t)l * n + i) * n + c] * x[(size_t)c * m + j];
                int32_t lo;
                const long long hi = lift_carry(s, &lo);
                P[2 * ((size_t)l * ce + (size_t)i * m + j)] = (double)lo;
                P[2 * ((size_t)l * ce + (size_t)i * m + j) + 1] = (double)hi;
            }
    for (size_t e = 0; e < ce; e++) {
        int f;
        rbar[e] = liftm_entry(P + 2 * e, ce, nd, r + e, ce, nrl, p, pw, &f);
        cnt[0] += f & 1;
        cnt[1] += (f >> 1) & 1;
    }
    return 0;
}

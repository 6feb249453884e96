// Host build of the limb arithmetic of the p-adic lifting (csrc/clrs_modp_lift_arith.h): the SAME lift_carry / lift_div_p / lift_renorm / lift_residue /
// lift_power_table the kernels of clrs_modp_lift.hip.h call, over arrays of limb vectors (vector v at limbs + v * nl, stride 1).  Test infrastructure;
// compiled by tests/dixon_util.py (g++ -O2 -std=c++17).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_lift_arith.h"

// digits[i * nl + l]: the balanced digits of values[i] by repeated lift_carry; carry_out[i]: what is left after nl digits
extern "C" int lift_split_host(int count, int nl, const long long *values, int32_t *digits, long long *carry_out) {
    for (int i = 0; i < count; i++) {
        long long v = values[i];
        for (int l = 0; l < nl; l++) v = lift_carry(v, &digits[(size_t)i * nl + l]);
        carry_out[i] = v;
    }
    return 0;
}

// in place: limbs <- floor(limbs / p) as lift_div_p leaves it (not balanced), rem[i] the remainder
extern "C" int lift_div_host(int p, int count, int nl, int32_t *limbs, int32_t *rem) {
    for (int i = 0; i < count; i++) rem[i] = lift_div_p(limbs + (size_t)i * nl, 1, nl, p);
    return 0;
}

extern "C" int lift_renorm_host(int count, int nl, int32_t *limbs, long long *carry_out) {
    for (int i = 0; i < count; i++) carry_out[i] = lift_renorm(limbs + (size_t)i * nl, 1, nl);
    return 0;
}

extern "C" int lift_residue_host(int p, int count, int nl, const int32_t *limbs, int32_t *out) {
    int32_t pw[64];
    if (nl > 64) return -1;
    lift_power_table(p, nl, pw);
    for (int i = 0; i < count; i++) out[i] = lift_residue(limbs + (size_t)i * nl, 1, nl, pw, p);
    return 0;
}

extern "C" int lift_power_table_host(int p, int count, int32_t *pw) {
    lift_power_table(p, count, pw);
    return 0;
}

// One step of the lifting on the host, built from the same pieces as k_lift_x / k_lift_r (plain loops where the kernels reduce over a wave): C (n x n residues),
// Ad (nd planes n x n), r ((nrl + 1) x n limbs, the working limb on top), rbar (n), x (n) out, cnt[2] the two counters.  Returns 0.
extern "C" int lift_step_host(int n, int nd, int nrl, int p, const int32_t *C, const int32_t *Ad, int32_t *r, int32_t *rbar, int32_t *x, int *cnt) {
    int32_t pw[64];
    if (nrl + 1 > 64) return -1;
    lift_power_table(p, nrl + 1, pw);
    for (int i = 0; i < n; i++) {
        long long s = 0;
        for (int c = 0; c < n; c++) s += (long long)C[(size_t)i * n + c] * rbar[c];
        x[i] = (int32_t)((unsigned long long)s % (unsigned long long)p);
    }
    for (int i = 0; i < n; i++) {
        long long carry = 0;
        for (int l = 0; l < nrl + 1; l++) {
            long long s = 0;
            if (l < nd)
                for (int c = 0; c < n; c++) s += (long long)Ad[((size_t)l * n + i) * n + c] * x[c];
            int32_t d;
            carry = lift_carry(carry + (l < nrl ? (long long)r[(size_t)l * n + i] : 0ll) - s, &d);
            r[(size_t)l * n + i] = d;
        }
        int flags;
        const int32_t res = lift_finish_row(r + i, (size_t)n, nrl, p, pw, carry, &flags);
        cnt[0] += flags & 1;
        cnt[1] += (flags >> 1) & 1;
        rbar[i] = res;                                             // (after the loop over c above: every x is already formed)
    }
    return 0;
}

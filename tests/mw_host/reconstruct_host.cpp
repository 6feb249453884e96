// Host build of the limb arithmetic of the rational reconstruction (csrc/clrs_modp_rec_arith.h): the SAME rec_* functions the kernels of clrs_modp_rec.hip.h
// are made of, behind a C interface, and a whole half-extended Euclid built from them the way k_rec_euclid is.  Test infrastructure; compiled by
// tests/reconstruct_util.py (g++ -O2 -std=c++17).
#include <vector>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_rec_arith.h"

extern "C" int rec_horner_host(int n, int p, int d, int32_t *v, long long *carry) {
    *carry = rec_horner_step(v, n, p, d);
    return 0;
}

// the K digits X[K - 1] .. X[0] by lazy steps on the limbs that can be non-zero, then one normalisation: what k_rec_horner does.  max_limb: the largest
// limb seen before the normalisation.
extern "C" int rec_horner_lazy_host(int n, int p, int K, const int32_t *X, int32_t *v, int32_t *max_limb, long long *carry) {
    const int pbits = rec_bits((unsigned long long)p);
    for (int l = 0; l < n; l++) v[l] = 0;
    *max_limb = 0;
    for (int j = 0; j < K; j++) {
        const int bound = ((j + 1) * pbits + REC_DIGIT_BITS - 1) / REC_DIGIT_BITS;
        rec_horner_step_lazy(v, bound < n ? bound : n, p, X[K - 1 - j]);
        for (int l = 0; l < n; l++) *max_limb = v[l] > *max_limb ? v[l] : *max_limb;
    }
    *carry = rec_normalize(v, n);
    return 0;
}

extern "C" int rec_length_host(const int32_t *v, int n) { return rec_length(v, n); }

extern "C" int rec_compare_host(const int32_t *a, int la, const int32_t *b, int lb) { return rec_compare(a, la, b, lb); }

extern "C" int rec_top_bits_host(const int32_t *v, int len, int nbits, long long *out, int *e) {
    *out = (long long)rec_top_bits(v, len, nbits, e);
    return 0;
}

// which = 0: rec_quotient_estimate, 1: rec_quotient_window
extern "C" int rec_estimate_host(int which, const int32_t *r0, int l0, const int32_t *r1, int l1, int32_t *c, int *s) {
    *c = which ? rec_quotient_window(r0, l0, r1, l1, s) : rec_quotient_estimate(r0, l0, r1, l1, s);
    return 0;
}

extern "C" int rec_submul_host(int32_t *r0, int l0, int32_t c, int s, const int32_t *r1, int l1) { return rec_submul(r0, l0, c, s, r1, l1); }

extern "C" int rec_addmul_host(int32_t *u0, int l0, int cap, int32_t c, int s, const int32_t *u1, int l1) { return rec_addmul(u0, l0, cap, c, s, u1, l1); }

extern "C" int rec_residue_host(const int32_t *v, int len, int p) {
    std::vector<int32_t> pw((size_t)(len > 0 ? len : 1));
    rec_power_table(p, len, pw.data());
    return rec_residue(v, len, pw.data(), p);
}

extern "C" int rec_power_bound_host(int p, int K) { return rec_power_limbs_bound(p, K); }

// m (room for 2 rec_power_limbs_bound limbs) <- p^K; returns its length
extern "C" int rec_power_host(int p, int K, int32_t *m) {
    std::vector<int32_t> tmp((size_t)2 * rec_power_limbs_bound(p, K) + 2);
    return rec_power(p, K, m, tmp.data());
}

// The half-extended Euclid of k_rec_euclid on one entry: m (length Lm), x (length lx), the bounds N, D with their lengths.  num, den: nl limbs each.
// out[0] = status (0 accepted, 1 rejected), out[1] = neg, out[2] = the (c, s) steps, out[3] = impossibilities, out[4] = the largest shift s seen.
extern "C" int rec_euclid_host(int p, int Lm, const int32_t *m, const int32_t *x, int lx, const int32_t *N, int lN, const int32_t *D, int lD, int nl, int32_t *num,
                               int32_t *den, int32_t *out) {
    const int cap = Lm + 1;
    std::vector<int32_t> rows((size_t)4 * cap, 0), pw((size_t)cap);
    rec_power_table(p, cap, pw.data());
    int32_t *r0 = rows.data(), *r1 = r0 + cap, *u0 = r1 + cap, *u1 = u0 + cap;
    for (int l = 0; l < Lm; l++) r0[l] = m[l];
    for (int l = 0; l < lx; l++) r1[l] = x[l];
    u1[0] = 1;
    int l0 = Lm, l1 = lx, lu0 = 0, lu1 = 1, swaps = 0, steps = 0, smax = 0;
    bool bad = false;
    while (!bad && rec_compare(r1, l1, N, lN) > 0) {
        for (;;) {
            int s;
            const int32_t c = rec_quotient_estimate(r0, l0, r1, l1, &s);
            if (c == 0) break;
            smax = s > smax ? s : smax;
            l0 = rec_submul(r0, l0, c, s, r1, l1);
            lu0 = l0 < 0 ? -1 : rec_addmul(u0, lu0, cap, c, s, u1, lu1);
            steps++;
            if (lu0 < 0) { bad = true; break; }
        }
        int32_t *t = r0; r0 = r1; r1 = t;
        t = u0; u0 = u1; u1 = t;
        int tl = l0; l0 = l1; l1 = tl;
        tl = lu0; lu0 = lu1; lu1 = tl;
        swaps++;
    }
    bool ok = !bad && lu1 > 0 && rec_compare(u1, lu1, D, lD) <= 0;
    if (ok) ok = !(rec_residue(r1, l1, pw.data(), p) == 0 && rec_residue(u1, lu1, pw.data(), p) == 0);
    for (int l = 0; l < nl; l++) {
        num[l] = ok && l < l1 ? r1[l] : 0;
        den[l] = ok && l < lu1 ? u1[l] : 0;
    }
    out[0] = ok ? 0 : 1;
    out[1] = ok && (swaps & 1) && l1 > 0 ? 1 : 0;
    out[2] = steps;
    out[3] = bad ? 1 : 0;
    out[4] = smax;
    return 0;
}

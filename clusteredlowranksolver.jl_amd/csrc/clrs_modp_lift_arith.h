// clrs_modp_lift_arith.h -- scalar arithmetic on integers held in balanced base-2^24 digits, for the p-adic lifting of clrs_modp_lift.hip.h (Dixon 1982;
// DESIGN.md section 15).  One text for the kernels and for a g++ build (tests/mw_host/lift_host.cpp), like clrs_modp_arith.h.
//
// An integer v is sum_l d_l 2^(24 l), little-endian, every digit an int32 in [-2^23, 2^23): negative numbers need no sign plane.  The functions below walk a
// limb vector through a pointer and a stride (limb l at v[l * stride]), so the same text serves a planar device array (stride = the row pitch) and a host
// array (stride = 1).  Everything is plain integer arithmetic in `long long`; nothing here rounds.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LIFTF __host__ __device__ inline
#else
#define LIFTF inline
#endif

#define LIFT_DIGIT_BITS 24
#define LIFT_BASE (1ll << LIFT_DIGIT_BITS)          // 2^24
#define LIFT_HALF (1ll << (LIFT_DIGIT_BITS - 1))    // 2^23: digits lie in [-LIFT_HALF, LIFT_HALF)

// the balanced low digit of v: d = ((v + 2^23) mod 2^24) - 2^23, for |v| < 2^62
LIFTF int32_t lift_digit(long long v) { return (int32_t)(((v + LIFT_HALF) & (LIFT_BASE - 1)) - LIFT_HALF); }

// one step of carry propagation: *digit = the balanced low digit of v, returns (v - *digit) / 2^24 (exact)
LIFTF long long lift_carry(long long v, int32_t *digit) {
    const int32_t d = lift_digit(v);
    *digit = d;
    return (v - (long long)d) / LIFT_BASE;
}

// floor(a / p) for p > 0 (C++ division truncates towards zero)
LIFTF long long lift_floor_div(long long a, long long p) {
    long long q = a / p;
    if (a % p < 0) q--;
    return q;
}

// Signed long division of the balanced limb vector t (nl limbs) by p, 2 <= p < 2^23, from the top limb: the limbs are replaced by quotient limbs q_l with
// sum_l q_l 2^(24 l) = floor(t / p), and t - p floor(t / p) in [0, p) is returned.  The running remainder stays in [0, p), so rem 2^24 + t_l lies in
// [-2^23, p 2^24) and every q_l in [-2^22, 2^24): an int32, but not balanced (lift_renorm).
LIFTF int32_t lift_div_p(int32_t *t, size_t stride, int nl, int p) {
    long long rem = 0;
    for (int l = nl - 1; l >= 0; l--) {
        const long long cur = rem * LIFT_BASE + (long long)t[(size_t)l * stride];
        const long long q = lift_floor_div(cur, (long long)p);
        rem = cur - q * (long long)p;
        t[(size_t)l * stride] = (int32_t)q;
    }
    return (int32_t)rem;
}

// Carry propagation over limbs of any int32 size, low to high: afterwards every limb is a balanced digit.  Returns the carry out of the top limb (0 when the
// number fits in nl balanced limbs).
LIFTF long long lift_renorm(int32_t *q, size_t stride, int nl) {
    long long carry = 0;
    for (int l = 0; l < nl; l++) {
        int32_t d;
        carry = lift_carry(carry + (long long)q[(size_t)l * stride], &d);
        q[(size_t)l * stride] = d;
    }
    return carry;
}

// The residue in [0, p) of a balanced limb vector, pw[l] = 2^(24 l) mod p: a digit times pw[l] is below 2^46 in magnitude, so up to 2^15 limbs sum exactly in
// an int64 before the one reduction.
LIFTF int32_t lift_residue(const int32_t *v, size_t stride, int nl, const int32_t *pw, int p) {
    long long acc = 0;
    for (int l = 0; l < nl; l++) acc += (long long)v[(size_t)l * stride] * (long long)pw[l];
    long long r = acc % (long long)p;
    if (r < 0) r += p;
    return (int32_t)r;
}

// What is left of a row of the residual update once r - A x stands in the nrl + 1 limbs at r (balanced, `carry` = what left the top limb): divide by p, bring the
// quotient back to balanced digits, which must fit in nrl limbs, and return the new r mod p.  *flags: bit 0 the division left a remainder, bit 1 a limb overflow.
LIFTF int32_t lift_finish_row(int32_t *r, size_t stride, int nrl, int p, const int32_t *pw, long long carry, int *flags) {
    bool over = carry != 0;                                                               // r - A x itself left the working limb
    const int32_t rem = lift_div_p(r, stride, nrl + 1, p);
    over = lift_renorm(r, stride, nrl + 1) != 0 || over;
    over = r[(size_t)nrl * stride] != 0 || over;                                           // the quotient must fit in nrl limbs
    *flags = (rem != 0 ? 1 : 0) | (over ? 2 : 0);
    return lift_residue(r, stride, nrl, pw, p);
}

// pw[l] = 2^(24 l) mod p for l < count (host side of the table the kernels are given)
LIFTF void lift_power_table(int p, int count, int32_t *pw) {
    const long long b = LIFT_BASE % (long long)p;
    long long v = 1 % (long long)p;
    for (int l = 0; l < count; l++) {
        pw[l] = (int32_t)v;
        v = v * b % (long long)p;
    }
}

// The residual update of ONE entry when the products A x come from the exact GEMM of clrs_modp_zz_gemm.hip.h (clrs_modp_liftm.hip.h):
// P holds (lo, hi) pairs of doubles, pair l (one per digit plane of A, l < nd) at P[2 l pstride] and P[2 l pstride + 1], with
// sum_c a_l[i, c] x[c] = lo_l + hi_l 2^24 exactly, |lo_l| <= 2^23 and |hi_l| <= n 2^22 + n < 2^38.  Limb l of A x is therefore s_l = lo_l + hi_(l-1), an int64
// far below 2^62; r_l - s_l goes through lift_carry up the nrl limbs at r and the working limb on top (nrl >= nd + 2, so the hi of the top plane has a limb), and
// lift_finish_row does the rest.  Balanced digits are unique, so the limbs, the residue returned and *flags are those of k_lift_r on the same entry.
LIFTF int32_t liftm_entry(const double *P, size_t pstride, int nd, int32_t *r, size_t rstride, int nrl, int p, const int32_t *pw, int *flags) {
    long long carry = 0;
    for (int l = 0; l < nrl + 1; l++) {
        long long s = 0;
        if (l < nd) s += (long long)P[2 * (size_t)l * pstride];
        if (l >= 1 && l <= nd) s += (long long)P[2 * (size_t)(l - 1) * pstride + 1];
        int32_t d;
        carry = lift_carry(carry + (l < nrl ? (long long)r[(size_t)l * rstride] : 0ll) - s, &d);
        r[(size_t)l * rstride] = d;
    }
    return lift_finish_row(r, rstride, nrl, p, pw, carry, flags);
}

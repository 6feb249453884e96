// clrs_modp_rec_arith.h -- scalar arithmetic on non-negative integers held in base-2^24 digits, for the rational reconstruction of the Dixon solutions
// (clrs_modp_rec.hip.h, clrs_modp_dixon_reconstruct).  One text for the kernels and for a g++ build
// (tests/mw_host/reconstruct_host.cpp), like clrs_modp_lift_arith.h.
//
// An integer v >= 0 is sum_l d_l 2^(24 l), little-endian, every digit an int32 in [0, 2^24), given by a pointer and a length.  The LENGTH of v is the
// index of its highest non-zero limb plus one, 0 for v = 0; the functions that take a length expect exactly that (no leading zero limbs) unless they
// say otherwise.  Remainders of the Euclidean algorithm never go negative and the cofactors are carried as magnitudes, so there is no sign anywhere.
// Everything is plain integer arithmetic on int32 / int64: no floating point, no inline assembly.  The kernels use the same formulas with the limb loop
// spread over the lanes of a wave.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RECF __host__ __device__ inline
#else
#define RECF inline
#endif

#define REC_DIGIT_BITS 24
#define REC_BASE (1ll << REC_DIGIT_BITS)      // 2^24
#define REC_MASK (REC_BASE - 1)
#define REC_MAX_LIMBS 32767                   // a column of a schoolbook product stays below 2^63

// the number of bits of v (0 for v = 0)
RECF int rec_bits(unsigned long long v) { return v ? 64 - __builtin_clzll(v) : 0; }

// the length of the limb vector v[0 .. n): the index of its highest non-zero limb plus one
RECF int rec_length(const int32_t *v, int n) {
    while (n > 0 && v[n - 1] == 0) n--;
    return n;
}

// -1, 0, 1 as a < b, a == b, a > b; la and lb are lengths
RECF int rec_compare(const int32_t *a, int la, const int32_t *b, int lb) {
    if (la != lb) return la > lb ? 1 : -1;
    for (int l = la - 1; l >= 0; l--)
        if (a[l] != b[l]) return a[l] > b[l] ? 1 : -1;
    return 0;
}

// One Horner step v <- v p + d over n limbs, fully carried; 0 <= d < 2^24, 2 <= p < 2^24.  Returns what left the top limb.
RECF long long rec_horner_step(int32_t *v, int n, int p, int d) {
    long long carry = d;
    for (int l = 0; l < n; l++) {
        const long long t = (long long)v[l] * (long long)p + carry;       // below 2^48 + 2^25
        v[l] = (int32_t)(t & REC_MASK);
        carry = t >> REC_DIGIT_BITS;
    }
    return carry;
}

// The same step without rippling the carry, as k_rec_horner does it: new_l = lo24(t_l) + hi(t_{l-1}), t_l = v_l p, and d into limb 0.  Limbs below
// 2^25 stay below 2^25 (t_l < 2^48 for p < 2^23, so both parts are below 2^24); the value is the same.  One rec_normalize at the end.
RECF void rec_horner_step_lazy(int32_t *v, int n, int p, int d) {
    long long hi = d;
    for (int l = 0; l < n; l++) {
        const long long t = (long long)v[l] * (long long)p;
        v[l] = (int32_t)((t & REC_MASK) + hi);
        hi = t >> REC_DIGIT_BITS;
    }
}

// carry propagation over limbs of any non-negative int32 size: afterwards every limb is a digit.  Returns what left the top limb.
RECF long long rec_normalize(int32_t *v, int n) {
    long long carry = 0;
    for (int l = 0; l < n; l++) {
        const long long t = (long long)v[l] + carry;
        v[l] = (int32_t)(t & REC_MASK);
        carry = t >> REC_DIGIT_BITS;
    }
    return carry;
}

// The top bits of v (length len > 0): floor(v / 2^e) with e = max(bits(v) - nbits, 0), nbits <= 62.  At most four limbs are read.
RECF unsigned long long rec_top_bits(const int32_t *v, int len, int nbits, int *e) {
    unsigned long long acc = (unsigned long long)v[len - 1];
    int have = rec_bits(acc), l = len - 2;
    const int total = REC_DIGIT_BITS * (len - 1) + have;
    while (l >= 0 && have < nbits) {
        const int take = nbits - have < REC_DIGIT_BITS ? nbits - have : REC_DIGIT_BITS;
        acc = (acc << take) | ((unsigned long long)v[l] >> (REC_DIGIT_BITS - take));
        have += take;
        l--;
    }
    *e = total - have;
    return acc;
}

// The quotient estimate from the top limbs alone: (c, s) with 0 <= c < 2^24 and c 2^(24 s) r1 <= r0, for r1 > 0 (lengths l0, l1 >= 1).  With
// T0 = the top 62 bits of r0 (r0 >= T0 2^e0) and T1 = the top 31 bits of r1, plus one when bits were cut off (r1 <= T1 2^e1),
// r0 / r1 >= floor(T0 / T1) 2^(e0 - e1) =: V, and c 2^(24 s) is V cut to its top 1 to 24 bits at a limb boundary.  V is within 2^-29 of the
// quotient, so c = 0 happens only for r0 < r1 or r0 / r1 < 1 + 2^-29: the caller then compares (rec_quotient_estimate).
RECF int32_t rec_quotient_window(const int32_t *r0, int l0, const int32_t *r1, int l1, int *s) {
    *s = 0;
    if (l0 < l1) return 0;
    int e0, e1;
    const unsigned long long T0 = rec_top_bits(r0, l0, 62, &e0);
    const unsigned long long T1 = rec_top_bits(r1, l1, 31, &e1) + (e1 > 0 ? 1ull : 0ull);
    const unsigned long long Q = T0 / T1;
    const int E = e0 - e1, nb = rec_bits(Q) + E;                      // V = Q 2^E has nb bits
    if (nb <= 0) return 0;
    const int sl = nb <= REC_DIGIT_BITS ? 0 : (nb - 1) / REC_DIGIT_BITS;     // the smallest s with nb - 24 s <= 24
    const int sh = REC_DIGIT_BITS * sl - E;                                    // c = floor(V / 2^(24 s)); sh < bits(Q) when positive
    *s = sl;
    return (int32_t)(sh >= 0 ? Q >> sh : Q << -sh);
}

// The quotient estimate: never above the true quotient (c 2^(24 s) r1 <= r0), at least 1 whenever r0 >= r1, and 0 exactly when r0 < r1.  r1 > 0.
RECF int32_t rec_quotient_estimate(const int32_t *r0, int l0, const int32_t *r1, int l1, int *s) {
    const int32_t c = rec_quotient_window(r0, l0, r1, l1, s);
    if (c != 0) return c;
    *s = 0;
    return rec_compare(r0, l0, r1, l1) >= 0 ? 1 : 0;
}

// r0 <- r0 - c 2^(24 s) r1 over the limbs s .. l0 - 1 of r0.  Limb l takes lo24(t_{l-s}) and hi(t_{l-s-1}), t_j = c r1[j] < 2^48, so it lies in
// (-2^25, 2^24) before the borrow.  Returns the new length of r0, or -1 when the result would be negative (r0 is then garbage).
RECF int rec_submul(int32_t *r0, int l0, int32_t c, int s, const int32_t *r1, int l1) {
    long long carry = 0, hi = 0;
    for (int l = s; l < l0; l++) {
        const int j = l - s;
        const long long t = j < l1 ? (long long)c * (long long)r1[j] : 0ll;
        const long long v = (long long)r0[l] - (t & REC_MASK) - hi + carry;
        hi = t >> REC_DIGIT_BITS;
        r0[l] = (int32_t)(v & REC_MASK);
        carry = v >> REC_DIGIT_BITS;                                   // (arithmetic shift: the floor)
    }
    if (carry != 0 || hi != 0 || l0 < l1 + s) return -1;
    return rec_length(r0, l0);
}

// u0 <- u0 + c 2^(24 s) u1, u0 in a row of `cap` limbs of which the first l0 count (what lies above them is not read).  Returns the new length, or -1
// when the sum does not fit in cap limbs.
RECF int rec_addmul(int32_t *u0, int l0, int cap, int32_t c, int s, const int32_t *u1, int l1) {
    long long carry = 0, hi = 0;
    int end = l1 + s + 2 > l0 + 1 ? l1 + s + 2 : l0 + 1, len = l0;     // the product has at most l1 + 1 limbs, the sum one more
    if (l1 == 0 || c == 0) return l0;
    for (int l = s < l0 ? s : l0; l < end; l++) {                      // (from l0 when s lies above it: the limbs between become zeros)
        const int j = l - s;
        const long long t = j >= 0 && j < l1 ? (long long)c * (long long)u1[j] : 0ll;
        const long long v = (l < l0 ? (long long)u0[l] : 0ll) + (t & REC_MASK) + hi + carry;
        hi = t >> REC_DIGIT_BITS;
        carry = v >> REC_DIGIT_BITS;
        if (l < cap) u0[l] = (int32_t)(v & REC_MASK);
        else if ((v & REC_MASK) != 0) return -1;
        if ((v & REC_MASK) != 0 && l + 1 > len) len = l + 1;
    }
    return carry != 0 || hi != 0 ? -1 : len;
}

// pw[l] = 2^(24 l) mod p for l < count
RECF void rec_power_table(int p, int count, int32_t *pw) {
    const long long b = REC_BASE % (long long)p;
    long long v = 1 % (long long)p;
    for (int l = 0; l < count; l++) {
        pw[l] = (int32_t)v;
        v = v * b % (long long)p;
    }
}

// v mod p from the table pw[l] = 2^(24 l) mod p: a digit times pw[l] is below 2^47, reduced as it is added
RECF int32_t rec_residue(const int32_t *v, int len, const int32_t *pw, int p) {
    unsigned long long acc = 0;
    for (int l = 0; l < len; l++) acc = (acc + (unsigned long long)v[l] * (unsigned long long)pw[l]) % (unsigned long long)p;
    return (int32_t)acc;
}

// out (la + lb limbs, distinct from a and b) <- a b, schoolbook by columns: a column sum of at most 2^15 products below 2^48 fits.  Host side.
inline void rec_mul(const int32_t *a, int la, const int32_t *b, int lb, int32_t *out) {
    unsigned long long carry = 0;
    for (int k = 0; k < la + lb; k++) {
        unsigned long long col = carry & (unsigned long long)REC_MASK;
        carry >>= REC_DIGIT_BITS;
        const int lo = k - (lb - 1) > 0 ? k - (lb - 1) : 0, hi = k < la - 1 ? k : la - 1;
        for (int i = lo; i <= hi; i++) {
            const unsigned long long t = (unsigned long long)a[i] * (unsigned long long)b[k - i];
            col += t & (unsigned long long)REC_MASK;
            carry += t >> REC_DIGIT_BITS;
        }
        out[k] = (int32_t)(col & (unsigned long long)REC_MASK);
        carry += col >> REC_DIGIT_BITS;
    }
}

// An upper bound of the length of p^K: every power p^j, j <= K, is below 2^(K bits(p))
RECF int rec_power_limbs_bound(int p, int K) { return (int)(((long long)K * rec_bits((unsigned long long)p) + REC_DIGIT_BITS - 1) / REC_DIGIT_BITS) + 1; }

// m <- p^K by squaring (host side), K >= 0: m and tmp each have room for 2 rec_power_limbs_bound(p, K) limbs.  Returns the length of p^K.
inline int rec_power(int p, int K, int32_t *m, int32_t *tmp) {
    int len = 1, top = 0;
    m[0] = 1;
    while ((K >> top) > 1) top++;
    for (int bit = top; bit >= 0; bit--) {
        if (bit != top) {                                             // m <- m^2
            rec_mul(m, len, m, len, tmp);
            len = rec_length(tmp, 2 * len);
            for (int l = 0; l < len; l++) m[l] = tmp[l];
        }
        if ((K >> bit) & 1) {                                          // m <- m p
            m[len] = 0;
            rec_horner_step(m, len + 1, p, 0);
            len = rec_length(m, len + 1);
        }
    }
    return len;
}

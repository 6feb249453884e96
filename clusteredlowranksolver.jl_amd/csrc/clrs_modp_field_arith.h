// clrs_modp_field_arith.h -- scalar arithmetic for a number field QQ(g) seen through a prime p < 2^23 at which the minimal polynomial f of g (degree D,
// monic mod p) splits: the evaluation g -> r at a root r of f mod p (a ring map Z[g] -> F_p), and the arithmetic of F_p[x] / (f) that decides whether p
// splits (x^p = x).  One text for the kernels of clrs_modp_minors_field.hip.h and for a g++ build (tests/mw_host/modp_field_host.cpp), as
// clrs_modp_arith.h is, on whose modp_reduce and modp_mul it builds.  DESIGN.md section 24.
//
// Every intermediate is an exact integer below 2^53 held in fp64; the bound stands beside each line.  D is a template parameter and every loop over it
// is unrolled, so no array below is indexed by a value unknown at compile time.
#pragma once
#include "clrs_modp_arith.h"

#define FF_MIN_DEG 2
#define FF_MAX_DEG 4                // the degrees the kernels are instantiated for: 2, 3, 4
#define FF_FROBENIUS_BITS 23        // x^p by square and multiply over this many bits of p, p < 2^23

// sum_j c[j] r^j mod p for residues c[0 .. D - 1] and r in [0, p): Horner from the top coefficient
template <int D>
MODPF double ff_residue(const double (&c)[D], double r, double p, double pinv) {
    double acc = c[D - 1];
#pragma unroll
    for (int j = D - 2; j >= 0; j--) acc = modp_reduce(fma(acc, r, c[j]), p, pinv);      // acc r + c[j] <= (p - 1)^2 + (p - 1) < 2^46
    return acc;
}

// f mod p made monic, as the table the products below fold with: row i holds x^(D + i) mod (f, p), i = 0 .. D - 2, as residues.  f[0 .. D] are the
// coefficients of f mod p in [0, p), lcinv = f[D]^-1 mod p (f[D] != 0 mod p).
template <int D>
MODPF void ff_fold_table(const double (&f)[D + 1], double lcinv, double p, double pinv, double (&xr)[D - 1][D]) {
#pragma unroll
    for (int j = 0; j < D; j++) xr[0][j] = modp_neg(modp_mul(f[j], lcinv, p, pinv), p);  // x^D = -sum_j (f_j / f_D) x^j; a product below 2^46
#pragma unroll
    for (int i = 1; i < D - 1; i++) {                                                      // x^(D + i) = x x^(D + i - 1): shift, fold the top term with row 0
        const double top = xr[i - 1][D - 1];
#pragma unroll
        for (int j = 0; j < D; j++) xr[i][j] = modp_reduce(fma(top, xr[0][j], j > 0 ? xr[i - 1][j - 1] : 0.0), p, pinv);   // (p - 1)^2 + (p - 1) < 2^46
    }
}

// out = a b in F_p[x] / (f): the 2 D - 1 coefficients of the plain product, each a sum of at most D products of residues (below D 2^46 <= 2^48), reduced;
// then coefficient j is one residue plus the D - 1 high coefficients times their rows of the table: (p - 1) + (D - 1)(p - 1)^2 < 2^48 for D <= 4
// (below 2^49 up to D = 8), reduced once.  `out` may be `a` or `b`.
template <int D>
MODPF void ff_mulmod(const double (&a)[D], const double (&b)[D], const double (&xr)[D - 1][D], double p, double pinv, double (&out)[D]) {
    double t[2 * D - 1];
#pragma unroll
    for (int k = 0; k < 2 * D - 1; k++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < D; i++)
            if (k - i >= 0 && k - i < D) s = fma(a[i], b[k - i], s);                       // at most D products below 2^46: s < 2^48 (D <= 4), exact
        t[k] = modp_reduce(s, p, pinv);
    }
#pragma unroll
    for (int j = 0; j < D; j++) {
        double s = t[j];
#pragma unroll
        for (int i = 0; i < D - 1; i++) s = fma(t[D + i], xr[i][j], s);                    // (p - 1) + (D - 1)(p - 1)^2 < 2^48, exact
        out[j] = modp_reduce(s, p, pinv);
    }
}

// One step of x^p by square and multiply, without a branch: acc <- acc^2, then acc x where `bit` is set (both are formed, one is selected).
// acc x: a shift, the top coefficient folded with row 0 of the table, a residue plus one product, below 2^46.
template <int D>
MODPF void ff_frobenius_step(double (&acc)[D], int bit, const double (&xr)[D - 1][D], double p, double pinv) {
    double s[D];
    ff_mulmod<D>(acc, acc, xr, p, pinv, s);
    const double top = s[D - 1];
#pragma unroll
    for (int j = 0; j < D; j++) {
        const double sx = modp_reduce(fma(top, xr[0][j], j > 0 ? s[j - 1] : 0.0), p, pinv);   // (p - 1)^2 + (p - 1) < 2^46
        acc[j] = bit ? sx : s[j];
    }
}

// x^p mod (f, p) into out[0 .. D - 1], f given by its table: FF_FROBENIUS_BITS steps whatever p is (the leading zero bits square 1)
template <int D>
MODPF void ff_frobenius(int p_int, const double (&xr)[D - 1][D], double p, double pinv, double (&out)[D]) {
#pragma unroll
    for (int j = 0; j < D; j++) out[j] = j == 0 ? 1.0 : 0.0;
    for (int b = FF_FROBENIUS_BITS - 1; b >= 0; b--) ff_frobenius_step<D>(out, (p_int >> b) & 1, xr, p, pinv);
}

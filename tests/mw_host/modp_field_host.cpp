// Host build of the number-field arithmetic mod p (csrc/clrs_modp_field_arith.h): the SAME ff_residue / ff_fold_table / ff_mulmod / ff_frobenius_step the
// kernels of clrs_modp_minors_field.hip.h call, over arrays and for every built degree.  Test infrastructure; compiled by tests/pd_field_util.py
// (g++ -O2 -std=c++17).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_field_arith.h"

template <int D>
static void residue_t(int p, int count, const double *c, const double *r, double *out) {
    const double pd = (double)p, pinv = 1.0 / pd;
    for (int i = 0; i < count; i++) {
        double cc[D];
        for (int j = 0; j < D; j++) cc[j] = c[(long)i * D + j];
        out[i] = ff_residue<D>(cc, r[i], pd, pinv);
    }
}

// what a lane of k_minors_residues_field does with one coefficient: Horner over balanced digits (top first) with the offset, then nothing else
extern "C" double ff_digits_host(int p, int nd, const int *digits) {
    const double pd = (double)p, pinv = 1.0 / pd, off = pd * ceil(8388608.0 / pd);
    double acc = 0.0;
    for (int l = nd - 1; l >= 0; l--) acc = modp_reduce(fma(acc, 16777216.0, (double)digits[l] + off), pd, pinv);
    return acc;
}

// out[count]: sum_j c[i][j] r[i]^j mod p
extern "C" int ff_residue_host(int deg, int p, int count, const double *c, const double *r, double *out) {
    if (deg == 2) residue_t<2>(p, count, c, r, out);
    else if (deg == 3) residue_t<3>(p, count, c, r, out);
    else if (deg == 4) residue_t<4>(p, count, c, r, out);
    else return -1;
    return 0;
}

template <int D>
static int field_t(int p, const double *f, const double *a, const double *b, int bit, double *table, double *prod, double *step, double *frob) {
    const double pd = (double)p, pinv = 1.0 / pd;
    double ff[D + 1], xr[D - 1][D], aa[D], bb[D], out[D];
    for (int j = 0; j <= D; j++) ff[j] = f[j];
    if (ff[D] == 0.0) return -2;
    ff_fold_table<D>(ff, modp_inv(ff[D], p), pd, pinv, xr);
    for (int i = 0; i < D - 1; i++)
        for (int j = 0; j < D; j++) table[i * D + j] = xr[i][j];
    for (int j = 0; j < D; j++) { aa[j] = a[j]; bb[j] = b[j]; }
    ff_mulmod<D>(aa, bb, xr, pd, pinv, out);
    for (int j = 0; j < D; j++) prod[j] = out[j];
    ff_frobenius_step<D>(aa, bit, xr, pd, pinv);
    for (int j = 0; j < D; j++) step[j] = aa[j];
    ff_frobenius<D>(p, xr, pd, pinv, out);
    for (int j = 0; j < D; j++) frob[j] = out[j];
    return 0;
}

// f [deg + 1] residues; table [(deg - 1) deg] = x^(deg + i) mod (f, p); prod = a b; step = a^2 x^bit; frob = x^p, all mod (f, p)
extern "C" int ff_field_host(int deg, int p, const double *f, const double *a, const double *b, int bit, double *table, double *prod, double *step,
                             double *frob) {
    if (deg == 2) return field_t<2>(p, f, a, b, bit, table, prod, step, frob);
    if (deg == 3) return field_t<3>(p, f, a, b, bit, table, prod, step, frob);
    if (deg == 4) return field_t<4>(p, f, a, b, bit, table, prod, step, frob);
    return -1;
}

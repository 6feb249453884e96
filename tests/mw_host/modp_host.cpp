// Host build of the scalar arithmetic mod p (csrc/clrs_modp_arith.h): the SAME modp_reduce / modp_mul / modp_inv / modp_is_prime the kernels of
// clrs_modp.hip call, over arrays.  Test infrastructure; compiled by tests/modp_util.py (g++ -O2 -std=c++17).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_modp_arith.h"

extern "C" int modp_reduce_host(int p, int count, const double *x, double *out) {
    const double pd = (double)p, pinv = 1.0 / pd;
    for (int i = 0; i < count; i++) out[i] = modp_reduce(x[i], pd, pinv);
    return 0;
}

extern "C" int modp_mul_host(int p, int count, const double *a, const double *b, double *out) {
    const double pd = (double)p, pinv = 1.0 / pd;
    for (int i = 0; i < count; i++) out[i] = modp_mul(a[i], b[i], pd, pinv);
    return 0;
}

extern "C" int modp_inv_host(int p, int count, const double *a, double *out) {
    for (int i = 0; i < count; i++) out[i] = modp_inv(a[i], p);
    return 0;
}

extern "C" int modp_is_prime_host(int p) { return modp_is_prime(p) ? 1 : 0; }

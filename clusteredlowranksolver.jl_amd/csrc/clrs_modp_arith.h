// clrs_modp_arith.h -- scalar arithmetic in the field of integers mod a prime p, 2 <= p < 2^23, on residues held in fp64.  One text for the kernels of
// clrs_modp.hip and for a g++ build (tests/mw_host/modp_host.cpp), as mw_cf_round and kv_entry are.
//
// Why fp64: a product of two residues is below 2^46 and a sum of up to 32 such products plus one residue is below 2^53, so it is an exact integer in an
// fp64 accumulator in any order of summation (at the largest prime below 2^23, p = 8388593: 32 (p - 1)^2 + (p - 1) < 2^52).  The trailing update of the
// elimination is therefore a plain v_mfma_f64_16x16x4 product with ONE reduction per entry after the whole k-sum.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MODPF __host__ __device__ inline
#else
#define MODPF inline
#endif

#define MODP_MAX_PRIME_BITS 23      // supported moduli: primes 2 <= p < 2^23

// x mod p for an integer 0 <= x < 2^53 held in fp64; pinv = 1.0 / p (rounded).  x * pinv is within (x / p) 2^-52 < 1 of x / p (x < 2^53, p >= 2), so
// q is floor(x / p) - 1, floor(x / p) or floor(x / p) + 1 and x - q p is an integer in [-p, 2p): the fma returns it exactly, one correction each way ends it.
MODPF double modp_reduce(double x, double p, double pinv) {
    const double q = floor(x * pinv);
    double r = fma(-q, p, x);
    if (r < 0.0) r += p;
    if (r >= p) r -= p;
    return r;
}

// a b mod p for residues a, b in [0, p): the product is below 2^46, exact
MODPF double modp_mul(double a, double b, double p, double pinv) { return modp_reduce(a * b, p, pinv); }

// -a mod p
MODPF double modp_neg(double a, double p) { return a == 0.0 ? 0.0 : p - a; }

// a^-1 mod p for a residue a != 0, p prime: a^(p - 2) (Fermat) by square and multiply; 1 for p = 2
MODPF double modp_inv(double a, int p_int) {
    const double p = (double)p_int, pinv = 1.0 / p;
    double r = 1.0, b = a;
    for (int e = p_int - 2; e > 0; e >>= 1) {
        if (e & 1) r = modp_mul(r, b, p, pinv);
        b = modp_mul(b, b, p, pinv);
    }
    return r;
}

// trial division; p < 2^23 ends within 2896 steps
MODPF bool modp_is_prime(int p) {
    if (p < 2) return false;
    if (p < 4) return true;
    if (p % 2 == 0) return false;
    for (long long d = 3; d * d <= (long long)p; d += 2)
        if (p % d == 0) return false;
    return true;
}

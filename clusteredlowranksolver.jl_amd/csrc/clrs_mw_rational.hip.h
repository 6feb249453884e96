// clrs_mw_rational.hip.h -- rounding a multi-word number to a rational by continued fractions: what the reference's roundx(v, g, 1) -> clindep does per entry
// of a kernel vector for the field QQ (src/rounding.jl:470-512, 623-628), DESIGN.md section 13.
//
// The relation a0 v + a1 = 0 the reference looks for (lindep at 1, 6, 11, ... bits, the first with |a0 v + a1| < kernel_round_errbound) is, for QQ, the pair
// (p, q) with the smallest q >= 1 such that |q v - p| < errbound: a best approximation of the second kind, hence a continued-fraction convergent of v.  So:
// generate the convergents p_k / q_k of x = |v| (a_k = floor of the running remainder, p_k = a_k p_{k-1} + p_{k-2}, the same for q; p, q fp64 integers below
// 2^53) and return the FIRST with |q_k x - p_k| < errbound, that quantity evaluated in K limbs from the original x -- not from the running remainder, so a
// floor decided one off next to an integer (the last step of a noisy rational) changes how many steps are taken, not which (p, q) comes out.
//
// One MWF function, host and device (tests/mw_host/mw_rational_host.cpp compiles it with g++), and one kernel: one lane per number, nothing shared.
#ifndef CLRS_MW_RATIONAL_HIP_H
#define CLRS_MW_RATIONAL_HIP_H

#include "clrs_mw_arith.h"

#define MW_CF_FOUND 0        // num / den is the first convergent below the bound
#define MW_CF_NONE 1         // no convergent with p, q < 2^53 meets the bound within MW_CF_STEPS steps
#define MW_CF_NOT_FINITE 2   // the head of v is NaN or Inf
#define MW_CF_STEPS 96       // (the longest expansion with q < 2^53 has 77 partial quotients)
#define MW_CF_CAP 0x1p53

namespace mwa {

// r >= 0, head below 2^53 -> a = floor(r) as an fp64 integer, f = r - a in [0, 1) (its head may round to 1.0 when r is just below an integer)
template <int K>
MWF void mw_floor(const mw<K> &r, double &a, mw<K> &f) {
    a = __builtin_floor(r.l[0]);
    f = add_d<K>(r, -a);
    if (f.l[0] < 0.0) {              // an integer head with a negative tail: one less
        a -= 1.0;
        f = add_d<K>(f, 1.0);
    }
}

// see the head of the file.  num carries the sign of v; den >= 1; both 0 unless MW_CF_FOUND is returned.
template <int K>
MWF int mw_cf_round(const mw<K> &v, double errbound, double &num, double &den) {
    num = den = 0.0;
    if (!(__builtin_fabs(v.l[0]) <= 0x1.fffffffffffffp1023)) return MW_CF_NOT_FINITE;
    double s[K];
#pragma unroll
    for (int i = 0; i < K; i++) s[i] = v.l[i];
    renorm<K>(s);                    // (the head then carries the sign, whatever the caller's limbs looked like; the value is unchanged)
    mw<K> x;
#pragma unroll
    for (int i = 0; i < K; i++) x.l[i] = s[i];
    const bool negative = x.l[0] < 0.0;
    if (negative) x = neg<K>(x);
    double p1 = 1.0, p2 = 0.0, q1 = 0.0, q2 = 1.0;          // p_{k-1}, p_{k-2}, q_{k-1}, q_{k-2}
    mw<K> r = x;
    for (int step = 0; step < MW_CF_STEPS; step++) {
        if (!(r.l[0] < MW_CF_CAP)) return MW_CF_NONE;
        double a;
        mw<K> f;
        mw_floor<K>(r, a, f);
        // an integer below 2^53 is exact in fp64 and rounding is monotone: the fma is exact or not below the cap
        const double p = fma_(a, p1, p2), q = fma_(a, q1, q2);
        if (!(p < MW_CF_CAP) || !(q < MW_CF_CAP)) return MW_CF_NONE;
        acc<K> c;
        acc_zero<K>(c);
        acc_fma_d<K, K>(c, x, q);
        acc_push<K, 0>(c, -p);
        const mw<K> e = acc_result<K>(c);
        if (__builtin_fabs(e.l[0]) < errbound) {
            num = negative ? -p : p;
            den = q;
            return MW_CF_FOUND;
        }
        if (!(f.l[0] > 0.0)) return MW_CF_NONE;             // the expansion ended (x is p / q exactly) above the bound
        r = recip<K>(f);
        p2 = p1; p1 = p;
        q2 = q1; q1 = q;
    }
    return MW_CF_NONE;
}

// the K-limb quotient of two fp64 integers; den = 0 (no relation found) gives 0
template <int K>
MWF mw<K> mw_from_ratio(double num, double den) {
    if (den == 0.0) return zero<K>();
    return div<K>(from_double<K>(num), from_double<K>(den));
}

}  // namespace mwa

#if defined(__HIPCC__) || defined(__HIP__)
#include "clrs_mw_kernels.hip.h"

// grid: ceil(count / MW_NT) workgroups, one lane per number.  v, vq: planar pools [K][plane]; num, den, status: [plane].  Lane i takes the number at position
// idx[i] of the plane (idx == nullptr: position i) and writes num, den, status and the K planes of num / den there; nothing else is written.
template <int K>
__global__ __launch_bounds__(MW_NT) void k_mw_rationalize(const double *__restrict__ v, mwi64 plane, const mwi64 *__restrict__ idx, int count, double errbound,
                                                         double *__restrict__ num, double *__restrict__ den, int *__restrict__ status, double *__restrict__ vq) {
    const mwi64 i = (mwi64)blockIdx.x * MW_NT + threadIdx.x;
    if (i >= count) return;
    const mwi64 o = idx ? idx[i] : i;
    if (o < 0 || o >= plane) return;                        // (the host builds idx inside the plane: nothing is stored outside it)
    double p, q;
    const int s = mwa::mw_cf_round<K>(mwa::ld<K>(v, plane, o), errbound, p, q);
    num[o] = p;
    den[o] = q;
    status[o] = s;
    mwa::st<K>(vq, plane, o, mwa::mw_from_ratio<K>(p, q));
}
#endif

#endif

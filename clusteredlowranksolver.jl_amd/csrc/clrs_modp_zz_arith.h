// clrs_modp_zz_arith.h -- the scalar arithmetic of the exact integer matrix product clrs_zz_gemm (clrs_modp_zz_gemm.hip.h): the split of
// an fp64 accumulator that holds an exact integer into a remainder and a multiple of 2^24, the flush built on it, and the carry walk that turns int64 column
// sums into balanced base-2^24 digits.  One text for the kernels and for a g++ build (tests/mw_host/zz_host.cpp), like clrs_modp_lift_arith.h.
//
// Why a flush is needed: a digit lies in [-2^23, 2^23], a product of two digits is at most 2^46 in magnitude, and one v_mfma_f64_16x16x4 adds four of them to an
// accumulator.  A remainder of at most 2^23 plus 4 F products stays at most 2^23 + F 2^48, which is below 2^53 iff F <= 31 (F = 32 gives 2^53 + 2^23): up to
// there every partial sum is an integer below 2^53 and the fp64 sum is exact in any order.  So after at most ZZ_MAX_FLUSH_MFMAS MFMAs the accumulator is split,
// acc = lo + c 2^24 with c = rint(acc 2^-24): the scaling by a power of two is exact, c is an integer, fma(-c, 2^24, acc) is the exact remainder (it is
// representable: an integer of magnitude <= 2^23), and c goes into a second fp64 sum `hi`, |hi| <= k 2^22 + k for an inner extent k, far below 2^53.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZZF __host__ __device__ inline
#else
#define ZZF inline
#endif

#define ZZ_DIGIT_BITS 24
#define ZZ_BASE 16777216.0                       // 2^24
#define ZZ_INV_BASE (1.0 / 16777216.0)           // 2^-24
#define ZZ_HALF (1ll << (ZZ_DIGIT_BITS - 1))     // 2^23: input digits lie in [-2^23, 2^23], output digits in [-2^23, 2^23)
#define ZZ_EXACT_LIMIT 9007199254740992.0        // 2^53
#define ZZ_MAX_FLUSH_MFMAS 31                    // the most MFMAs (of k-extent 4) an accumulator may take between two flushes
#define ZZ_FLUSH_MFMAS 28                        // what k_zz_gemm takes: seven steps of k-extent 16

// acc = *lo + c 2^24 exactly, for an integer |acc| < 2^53: returns c = rint(acc 2^-24) (ties to even), |*lo| <= 2^23
ZZF double zz_split(double acc, double *lo) {
    const double c = rint(acc * ZZ_INV_BASE);
    *lo = fma(-c, ZZ_BASE, acc);
    return c;
}

// the flush: the accumulator keeps its remainder, the multiple of 2^24 moves into *hi (counted in units of 2^24)
ZZF void zz_flush(double *acc, double *hi) {
    double lo;
    *hi += zz_split(*acc, &lo);
    *acc = lo;
}

// 0 when (lo, hi) is what a flushed accumulator must be: integers, |lo| <= 2^23, |hi| < 2^53 (a NaN fails every comparison)
ZZF int zz_pair_bad(double lo, double hi) {
    return !(lo == rint(lo) && fabs(lo) <= (double)ZZ_HALF && hi == rint(hi) && fabs(hi) < ZZ_EXACT_LIMIT);
}

// the balanced low digit of v: ((v + 2^23) mod 2^24) - 2^23, for |v| < 2^62
ZZF int32_t zz_digit(long long v) { return (int32_t)(((v + ZZ_HALF) & ((1ll << ZZ_DIGIT_BITS) - 1)) - ZZ_HALF); }

// The carry walk of one entry: S holds ns int64 column sums (sum s at S[s * sstride], |S| < 2^62), the value is sum_s S[s] 2^(24 s).  Writes its ndc balanced
// digits (digit s at C[s * cstride]): planes above ns receive what the carry leaves, so a negative value is sign-extended through its digits.  Returns 1 when
// the value does not fit in ndc digits -- a non-zero digit at or above plane ndc, or a carry left at the end -- and 0 otherwise.  A carry is below 2^40 in
// magnitude, so two planes past the last sum exhaust it.
ZZF int zz_carry_walk(const long long *S, size_t sstride, int ns, int32_t *C, size_t cstride, int ndc) {
    long long carry = 0;
    int over = 0;
    const int top = ndc > ns + 2 ? ndc : ns + 2;
    for (int s = 0; s < top; s++) {
        const long long v = carry + (s < ns ? S[(size_t)s * sstride] : 0ll);
        const int32_t d = zz_digit(v);
        carry = (v - (long long)d) / (1ll << ZZ_DIGIT_BITS);                               // (exact: v - d is a multiple of 2^24)
        if (s < ndc) C[(size_t)s * cstride] = d;
        else if (d != 0) over = 1;
    }
    return (over || carry != 0) ? 1 : 0;
}

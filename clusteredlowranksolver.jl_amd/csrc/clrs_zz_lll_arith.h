// clrs_zz_lll_arith.h -- the arithmetic of the batched LLL reduction clrs_zz_lll (clrs_zz_lll.hip), one text for the kernel and for a
// g++ build (tests/mw_host/lll_host.cpp), like clrs_modp_zz_arith.h.  Both are compiled with -ffp-contract=off: two_sum and two_prod must stay what they are.
//
// The basis rows are long integers in balanced base-2^24 digits (plane s of row i, column c at D[(s * d + i) * c_total + c]) and every change to them is an
// exact integer operation (lll_row_update_column, a swap of two entries of the order table).  The Gram-Schmidt data are K-limb floating point (clrs_mw_arith.h)
// and only steer.  The pieces:
//
//   lll_entry_to_mw      an entry -> its K-limb image, from its top LLL_CONV_DIGITS(K) digits
//   lll_lane_partial     the part of <b_a, b_b> one lane of a wave owns: columns lane, lane + 64, ... below cols_gram, in that order
//   lll_tree_add         one node of the in-wave tree that sums the 64 partials (offsets 32, 16, ..., 1; lane 0 ends with the sum)
//   lll_chol_mu / lll_chol_sub   the Cholesky row: r_ki final -> mu_ki = r_ki / r_ii, then s_j <- s_j - mu_ji r_ki for every j > i (i ascending)
//   lll_quotient / lll_mu_sub_x  X_j = rint(head mu_kj), then mu_ki <- mu_ki - X_j mu_ji for every i < j (j descending)
//   lll_quotient_split   X = sum_t xd[t] 2^(24 (t + sh)): at most four digits and a digit shift
//   lll_row_update_column   b_k <- b_k - sum_j X_j b_j in one column: int64 digit sums and the carry walk, in place
//   lll_lovasz_swap      s_{k-1} < delta r_{k-1,k-1}
//
// Range: an entry of nd <= LLL_MAX_ND = 20 digits is below 2^480 in magnitude, a Gram entry over at most 256 columns below 2^968: everything stays a finite
// double without a common exponent per row.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "clrs_modp_zz_arith.h"
#include "clrs_mw_arith.h"

#define LLL_MAX_ROWS 128
#define LLL_MAX_COLS 256
#define LLL_MAX_ND 20
#define LLL_NT 256                        // threads of the one workgroup of a lattice
#define LLL_WAVES (LLL_NT / 64)
#define LLL_MAX_PASSES 64                 // size-reduction passes per visit of an index
#define LLL_CONV_DIGITS(K) ((53 * (K) + 23) / 24 + 2)
#define LLL_XDIGITS 4

// status of a lattice (info[b][0]); LLL_RUNNING only between the launches of one call
#define LLL_OK 0
#define LLL_CAP 1
#define LLL_ARITH 2
#define LLL_OVERFLOW 3
#define LLL_RUNNING (-1)

namespace zlll {
using mwa::mw;

// 2^e for -1022 <= e <= 1023
ZZF double lll_pow2(int e) {
    const uint64_t bits = (uint64_t)(e + 1023) << 52;
    double v;
    __builtin_memcpy(&v, &bits, sizeof v);
    return v;
}

ZZF bool lll_finite(double v) { return v - v == 0.0; }

// the K-limb image of the entry sum_s p[s * stride] 2^(24 s): its top LLL_CONV_DIGITS(K) digits from the highest non-zero one down, every term exact
template <int K>
ZZF mw<K> lll_entry_to_mw(const int32_t *p, size_t stride, int nd) {
    int top = nd - 1;
    while (top >= 0 && p[(size_t)top * stride] == 0) top--;
    mwa::acc<K> a;
    mwa::acc_zero<K>(a);
    const int low = top - LLL_CONV_DIGITS(K) + 1 > 0 ? top - LLL_CONV_DIGITS(K) + 1 : 0;
    for (int s = top; s >= low; s--) mwa::acc_push<K, 0>(a, (double)p[(size_t)s * stride] * lll_pow2(ZZ_DIGIT_BITS * s));
    return mwa::acc_result<K>(a);
}

// what lane `lane` adds to <b_ra, b_rb>: the columns lane, lane + 64, ... below cols_gram (ra, rb: physical rows)
template <int K>
ZZF mw<K> lll_lane_partial(const int32_t *D, int d, int c_total, int nd, int ra, int rb, int cols_gram, int lane) {
    const size_t stride = (size_t)d * c_total;
    mwa::acc<K> a;
    mwa::acc_zero<K>(a);
    for (int c = lane; c < cols_gram; c += 64) {
        const mw<K> x = lll_entry_to_mw<K>(D + (size_t)ra * c_total + c, stride, nd);
        const mw<K> y = lll_entry_to_mw<K>(D + (size_t)rb * c_total + c, stride, nd);
        mwa::acc_fma<K, K, K>(a, x, y);
    }
    return mwa::acc_result<K>(a);
}

template <int K>
ZZF mw<K> lll_tree_add(const mw<K> &a, const mw<K> &b) { return mwa::add<K>(a, b); }

template <int K>
ZZF mw<K> lll_chol_mu(const mw<K> &r, const mw<K> &rdiag) { return mwa::div<K>(r, rdiag); }

template <int K>
ZZF mw<K> lll_chol_sub(const mw<K> &s, const mw<K> &mu, const mw<K> &r) { return mwa::fnma<K>(s, mu, r); }

// |mu| > eta
template <int K>
ZZF bool lll_exceeds(const mw<K> &mu, double eta) {
    const mw<K> d = mwa::add_d<K>(mwa::abs<K>(mu), -eta);
    return d.l[0] > 0.0;
}

// the quotient of a size-reduction step, from the head limb: an integer m 2^e with |m| <= 2^53
template <int K>
ZZF double lll_quotient(const mw<K> &mu) { return rint(mu.l[0]); }

// mu_ki - X mu_ji
template <int K>
ZZF mw<K> lll_mu_sub_x(const mw<K> &mu_ki, const mw<K> &mu_ji, double X) {
    mwa::acc<K> c;
#pragma unroll
    for (int i = 0; i < K; i++) c.s[i] = mu_ki.l[i];
    mwa::acc_fma_d<K, K>(c, mu_ji, X, -1.0);
    return mwa::acc_result<K>(c);
}

// The finite integer X = sum_t xd[t] 2^(24 (t + *sh)), digits in [-2^23, 2^23].  With e the exponent of the last bit of the fp64 X, sh = max(e, 0) / 24 and
// m = X 2^(-24 sh) is an integer below 2^(53 + 23): three splits (zz_split, exact) leave a fourth digit below 2^5.  Returns 0, or 1 when X is no finite integer.
ZZF int lll_quotient_split(double X, int32_t *xd, int32_t *sh) {
    for (int t = 0; t < LLL_XDIGITS; t++) xd[t] = 0;
    *sh = 0;
    if (!lll_finite(X) || X != rint(X)) return 1;
    if (X == 0.0) return 0;
    int ex;
    (void)frexp(X, &ex);                                   // |X| in [2^(ex - 1), 2^ex): the last bit of the mantissa has exponent ex - 53
    const int e = ex - 53 > 0 ? ex - 53 : 0;
    *sh = e / ZZ_DIGIT_BITS;
    double m = X * lll_pow2(-ZZ_DIGIT_BITS * *sh);       // exact: a power of two, and the result is an integer
    for (int t = 0; t < LLL_XDIGITS - 1; t++) {
        double lo;
        m = zz_split(m, &lo);
        xd[t] = (int32_t)lo;
    }
    xd[LLL_XDIGITS - 1] = (int32_t)m;
    return 0;
}

// Column `col` of b_k <- b_k - sum_{j < k} X_j b_j, in place, X_j = sum_t xd[4 j + t] 2^(24 (t + sh[j])) (rows through the order table).  Per digit plane one
// int64 sum -- at most 4 (k) products of a digit and a quotient digit, each at most 2^46, plus the digit and the carry: below 2^56 for 128 rows -- and one
// step of the carry walk of clrs_modp_zz_arith.h (zz_digit, then the exact division by 2^24; the walk is taken plane by plane here so that no thread keeps nd
// sums).  The walk goes on through the planes the products reach above nd; returns 1 when the entry leaves its nd digits -- a non-zero digit at or above plane
// nd, or a carry left at the end (the digits written are then not the entry's) -- and 0 otherwise.
ZZF int lll_row_update_column(int32_t *D, int d, int c_total, int nd, int col, const int32_t *ord, int k, const int32_t *xd, const int32_t *sh) {
    const size_t stride = (size_t)d * c_total;
    int32_t *bk = D + (size_t)ord[k] * c_total + col;
    long long carry = 0;
    int top = nd, over = 0;                                // the planes the products reach: those at and above nd must come out zero
    for (int j = 0; j < k; j++) {
        const int32_t *x = xd + LLL_XDIGITS * j;
        if ((x[0] | x[1] | x[2] | x[3]) != 0 && nd + sh[j] + LLL_XDIGITS > top) top = nd + sh[j] + LLL_XDIGITS;
    }
    for (int s = 0; s < top; s++) {
        long long v = carry + (s < nd ? (long long)bk[(size_t)s * stride] : 0ll);
        for (int j = 0; j < k; j++) {
            const int32_t *x = xd + LLL_XDIGITS * j;
            if ((x[0] | x[1] | x[2] | x[3]) == 0) continue;
            const int32_t *bj = D + (size_t)ord[j] * c_total + col;
            for (int t = 0; t < LLL_XDIGITS; t++) {
                const int src = s - sh[j] - t;
                if (src >= 0 && src < nd) v -= (long long)x[t] * (long long)bj[(size_t)src * stride];
            }
        }
        const int32_t dg = zz_digit(v);
        carry = (v - (long long)dg) / (1ll << ZZ_DIGIT_BITS);
        if (s < nd) bk[(size_t)s * stride] = dg;
        else if (dg != 0) over = 1;
    }
    return (over || carry != 0) ? 1 : 0;
}

// the Lovasz decision at index k >= 1: exchange when s_{k-1} = r_kk + mu_{k,k-1}^2 r_{k-1,k-1} is below delta r_{k-1,k-1}
template <int K>
ZZF bool lll_lovasz_swap(const mw<K> &s_km1, const mw<K> &r_prev, double delta) {
    return mwa::less<K>(s_km1, mwa::mul_d<K>(r_prev, delta));
}

// r_kk must be a positive finite number
template <int K>
ZZF bool lll_diag_ok(const mw<K> &r) { return lll_finite(r.l[0]) && r.l[0] > 0.0; }

}  // namespace zlll

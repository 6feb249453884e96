// clrs_mw_field_round_arith.h -- rounding a multi-word number to a number field QQ(g) of degree deg = 2 .. 4 by an integer relation: what the reference's
// roundx(x, g, deg) -> clindep -> lindep does per entry of a kernel vector (src/rounding.jl:481-534, 623-628), DESIGN.md section 23.  One text for the kernel
// (clrs_mw_field_round.hip) and for a g++ build (tests/mw_host/field_round_host.cpp), both compiled with -ffp-contract=off.
//
// Per number v: u = (v, g^0, .., g^(deg - 1)), D = deg + 1 entries, and a relation a_0 u_0 + .. + a_deg u_deg ~ 0 with small integers a is the first row of an
// LLL-reduced basis of the lattice spanned by the rows [e_i | s_p,i], s_p,i = floor(2^p u_i), searched at p = 1, 6, 11, .. bits.
//
//   fixed point, once     W_i = floor(2^P u_i) for the top rung P, as base-2^24 digits in two's complement (digits in [0, 2^24), the top one carries the
//                         sign), summed from the K limbs in integers: fr_fixed_point.  A limb's bits below 2^-(P + 48) are floored away one limb at a time,
//                         so W_i is one below the floor of the exact sum when that sum lies within K 2^-48 above an integer -- which moves a last bit of the
//                         lattice, never the answer: acceptance reads the original limbs
//   the ladder            s_p = floor(W / 2^(P - p)).  The state is the exact integers U (D x D, unimodular) and c = U s_p; the step from p to p' = p + nb is
//                         c <- 2^nb c + U t with t_i the next nb bits of W_i (fr_advance; nb = 1 into the first rung, 5 afterwards).  No p-bit number is ever
//                         multiplied, and the rows [U_i | c_i] are the previous reduced basis with its last column rescaled
//   LLL at a rung         (delta, eta) = (0.99, 0.51).  A visit computes the Gram-Schmidt data of all D rows from the exact digits in 2-limb arithmetic
//                         (fr_gram_schmidt: every index a compile-time constant, so the data stay in registers), size-reduces every row (quotients with j
//                         descending, rows ascending; exact row operations fr_row_sub) until no |mu| exceeds eta, then exchanges the first pair of rows that
//                         fails the Lovasz test and starts over.  Nothing floating point survives a visit, let alone a rung
//   acceptance            a = U_0; err = |sum_i a_i u_i| in K limbs from the original numbers; the first rung with err < errbound.  Then
//                         vq = -(sum_{k >= 1} a_k g^(k - 1)) / a_0 in K limbs
//
// Storage: everything a lane keeps between rungs lives in an int32 workspace, element e of lane i at ws[e * stride + i] (coalesced on the device, stride = count):
// FR_HDR header ints (status, next rung, exchanges, rungs visited), the nw digits of W_0, then the lattice, digit s of row i, column c at element
// FR_HDR + nw + (s * D + i) * (D + 1) + c, balanced digits as in clrs_zz_lll_arith.h.  The digits of W_1 .. W_deg are the same for every number: `gw`, [deg][nw].
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "clrs_zz_lll_arith.h"

#define FR_FOUND 0            // rel is a relation below errbound, a_0 != 0
#define FR_EXHAUSTED 1        // no rung up to the top one gave a relation below errbound
#define FR_NOT_FINITE 2       // a limb of v is NaN or Inf
#define FR_STEER 3            // the Gram-Schmidt data were unusable, or a cap (passes per visit, exchanges per rung) was hit
#define FR_OVERFLOW 4         // an entry of the lattice left its nd digits (or |v| >= 2^22)
#define FR_NO_FIELD 5         // the accepted relation has a_0 = 0: the powers of g are dependent to this accuracy
#define FR_RUNNING (-1)       // only between the launches of one call

#define FR_MIN_DEG 2
#define FR_MAX_DEG 4
#define FR_HDR 4              // header ints of a lane: status, next rung index, exchanges, rungs visited
#define FR_MAX_PASSES 64      // size-reduction passes per visit
#define FR_MAX_EXCHANGES 4096 // exchanges per rung
#define FR_LAUNCH_RUNGS 16    // rungs a launch advances a lane by (clrs_config_set("field_round_launch_rungs", n))
#define FR_DELTA 0.99
#define FR_ETA 0.51
#define FR_FRAC_DIGITS 2      // digits kept below 2^-P while the limbs are summed
#define FR_V_LIMIT 0x1p22     // |v| and |g^k| must stay below this

namespace frnd {
using mwa::mw;

// the top rung: min(bits, 53 limbs - 16) rounded down onto the ladder 1, 6, 11, ..
ZZF int fr_top_bits(int bits, int limbs) {
    const int m = bits < 53 * limbs - 16 ? bits : 53 * limbs - 16;
    return 1 + 5 * ((m - 1) / 5);
}
ZZF int fr_rungs(int P) { return (P - 1) / 5 + 1; }              // rung r is at p = 1 + 5 r bits
ZZF int fr_w_digits(int P) { return P / ZZ_DIGIT_BITS + 2; }     // 24 nw >= P + 25: bits P .. P + 23 (floor(u) and its sign) are inside
ZZF int fr_ws_elems(int D, int P, int nd) { return FR_HDR + fr_w_digits(P) + nd * D * (D + 1); }

struct FrArgs {
    const double *v;          // [K][plane_v]
    long long plane_v;
    const double *gpow;       // [K][deg], limb l of g^k at gpow[l * deg + k]
    const int32_t *gw;        // [deg][nw]
    int count, P, nw, nd;
    double errbound;
    int32_t *ws;              // [fr_ws_elems][stride]
    long long stride;
    int32_t *rel;             // [nd][D][plane]
    int32_t *status, *rung;   // [plane]
    double *err;              // [plane]
    double *vq;               // [K][plane]
    int32_t *info;            // [2][plane]: exchanges, rungs visited
    long long plane;
};

// x = M 2^e, an integer M below 2^53 in magnitude, moved to units of 2^(-P - 48): M 2^q with q >= 0, bits below the unit floored away
ZZF void fr_limb_split(double x, int P, long long *M, int *q) {
    *M = 0;
    *q = 0;
    if (x == 0.0) return;
    int ex;
    const double f = frexp(x, &ex);
    long long m = (long long)ldexp(f, 53);
    long long qq = (long long)ex - 53 + P + ZZ_DIGIT_BITS * FR_FRAC_DIGITS;
    if (qq < 0) {
        m = -qq >= 63 ? (m < 0 ? -1ll : 0ll) : (m >> (int)(-qq));
        qq = 0;
    }
    *M = m;
    *q = (int)qq;
}

// digit plane s of M 2^q read as an infinite two's complement number: a value in [0, 2^24)
ZZF long long fr_limb_plane(long long M, int q, int s) {
    const int lo = ZZ_DIGIT_BITS * s - q;
    long long piece;
    if (lo >= 63) piece = M < 0 ? -1ll : 0ll;
    else if (lo >= 0) piece = M >> lo;
    else if (lo > -ZZ_DIGIT_BITS) piece = (long long)((unsigned long long)M << (-lo));
    else piece = 0;
    return piece & ((1ll << ZZ_DIGIT_BITS) - 1);
}

// the nw digits of W = floor(2^P u), digit s at w[s * stride]; |u| < FR_V_LIMIT and every limb finite
template <int K>
ZZF void fr_fixed_point(const mw<K> &u, int P, int nw, int32_t *w, size_t stride) {
    long long M[K];
    int q[K];
#pragma unroll
    for (int l = 0; l < K; l++) fr_limb_split(u.l[l], P, &M[l], &q[l]);
    long long carry = 0;
    for (int s = 0; s < nw + FR_FRAC_DIGITS; s++) {
        long long t = carry;
#pragma unroll
        for (int l = 0; l < K; l++) t += fr_limb_plane(M[l], q[l], s);
        if (s >= FR_FRAC_DIGITS) w[(size_t)(s - FR_FRAC_DIGITS) * stride] = (int32_t)(t & ((1ll << ZZ_DIGIT_BITS) - 1));
        carry = t >> ZZ_DIGIT_BITS;
    }
}

// bits lo .. lo + n - 1 of W (n <= 24, lo + n <= 24 nw)
ZZF int32_t fr_bits(const int32_t *w, size_t stride, int nw, int lo, int n) {
    const int s = lo / ZZ_DIGIT_BITS, o = lo % ZZ_DIGIT_BITS;
    long long x = (long long)w[(size_t)s * stride];
    if (s + 1 < nw) x |= (long long)w[(size_t)(s + 1) * stride] << ZZ_DIGIT_BITS;
    return (int32_t)((x >> o) & ((1ll << n) - 1));
}

template <int K>
ZZF bool fr_all_finite(const mw<K> &u) {
    bool ok = true;
#pragma unroll
    for (int l = 0; l < K; l++) ok = ok && zlll::lll_finite(u.l[l]);
    return ok;
}

// the digits of W_i: the lane's own for i = 0, the shared ones above
template <int D>
ZZF int32_t fr_u_bits(const FrArgs &a, const int32_t *ws, int i, int lo, int n) {
    return i == 0 ? fr_bits(ws + (size_t)FR_HDR * a.stride, (size_t)a.stride, a.nw, lo, n) : fr_bits(a.gw + (size_t)(i - 1) * a.nw, 1, a.nw, lo, n);
}

// the lattice of a lane: digit s of row i, column c at L[((s * D + i) * (D + 1) + c) * stride]
template <int D>
ZZF int32_t *fr_entry(int32_t *L, size_t stride, int i, int c) { return L + (size_t)(i * (D + 1) + c) * stride; }
template <int D>
ZZF size_t fr_digit_stride(size_t stride) { return (size_t)D * (D + 1) * stride; }

// what a lane that ends leaves in the outputs; a: the row of the relation or null
template <int K, int D>
ZZF void fr_finish(const FrArgs &a, long long i, int32_t *ws, int status, int p, double err, const int32_t *row, const mw<K> &vq) {
    const size_t ds = fr_digit_stride<D>((size_t)a.stride);
    for (int s = 0; s < a.nd; s++)
#pragma unroll
        for (int c = 0; c < D; c++) a.rel[((size_t)s * D + c) * a.plane + i] = row ? row[(size_t)c * a.stride + (size_t)s * ds] : 0;
    a.status[i] = status;
    a.rung[i] = p;
    a.err[i] = err;
    mwa::st<K>(a.vq, (long)a.plane, (long)i, vq);
    a.info[i] = ws[2 * a.stride];
    a.info[a.plane + i] = ws[3 * a.stride];
    ws[0] = status;
}

// the first step of a lane: the header, W_0, and the lattice [I | floor(u)] of "rung -1" (p = 0)
template <int K, int D>
ZZF void fr_init(const FrArgs &a, long long i) {
    int32_t *ws = a.ws + i;
    const size_t st = (size_t)a.stride;
    ws[0] = FR_RUNNING;
    ws[st] = 0;
    ws[2 * st] = 0;
    ws[3 * st] = 0;
    const mw<K> v = mwa::ld<K>(a.v, (long)a.plane_v, (long)i);
    if (!fr_all_finite<K>(v)) {
        fr_finish<K, D>(a, i, ws, FR_NOT_FINITE, 0, 0.0, nullptr, mwa::zero<K>());
        return;
    }
    if (!(fabs(v.l[0]) < FR_V_LIMIT)) {
        fr_finish<K, D>(a, i, ws, FR_OVERFLOW, 0, 0.0, nullptr, mwa::zero<K>());
        return;
    }
    double s[K];
#pragma unroll
    for (int l = 0; l < K; l++) s[l] = v.l[l];
    mwa::renorm<K>(s);                                   // (non-overlapping limbs: the integer sum then sees each bit once; the value is unchanged)
    mw<K> x;
#pragma unroll
    for (int l = 0; l < K; l++) x.l[l] = s[l];
    fr_fixed_point<K>(x, a.P, a.nw, ws + (size_t)FR_HDR * st, st);
    int32_t *L = ws + (size_t)(FR_HDR + a.nw) * st;
    const size_t ds = fr_digit_stride<D>(st);
#pragma unroll
    for (int r = 0; r < D; r++) {
#pragma unroll
        for (int c = 0; c <= D; c++) {
            int32_t *e = fr_entry<D>(L, st, r, c);
            int32_t d0 = c == r ? 1 : 0;
            if (c == D) {
                d0 = fr_u_bits<D>(a, ws, r, a.P, ZZ_DIGIT_BITS);
                if (d0 >= (int32_t)ZZ_HALF) d0 -= (int32_t)(1 << ZZ_DIGIT_BITS);
            }
            e[0] = d0;                                   // (|u| < 2^22: one balanced digit)
            for (int sd = 1; sd < a.nd; sd++) e[(size_t)sd * ds] = 0;
        }
    }
}

// c <- 2^nb c + U t.  Returns 1 when an entry of c leaves its nd digits.
template <int D>
ZZF int fr_advance(int32_t *L, size_t st, int nd, int nb, const int32_t (&t)[D]) {
    const size_t ds = fr_digit_stride<D>(st);
    int over = 0;
#pragma unroll
    for (int r = 0; r < D; r++) {
        int32_t *c = fr_entry<D>(L, st, r, D);
        long long carry = 0;
        for (int s = 0; s < nd + 2; s++) {
            long long x = carry;
            if (s < nd) {
                x += (long long)c[(size_t)s * ds] * (1ll << nb);
#pragma unroll
                for (int j = 0; j < D; j++) x += (long long)fr_entry<D>(L, st, r, j)[(size_t)s * ds] * (long long)t[j];
            }
            const int32_t dg = zz_digit(x);
            carry = (x - (long long)dg) / (1ll << ZZ_DIGIT_BITS);
            if (s < nd) c[(size_t)s * ds] = dg;
            else if (dg != 0) over = 1;
        }
        if (carry != 0) over = 1;
    }
    return over;
}

// row k <- row k - X row j, every column, X = sum_t xd[t] 2^(24 (t + sh)).  Returns 1 when an entry leaves its nd digits.
template <int D>
ZZF int fr_row_sub(int32_t *L, size_t st, int nd, int k, int j, const int32_t (&xd)[LLL_XDIGITS], int sh) {
    const size_t ds = fr_digit_stride<D>(st);
    int over = 0;
    const int top = nd + sh + LLL_XDIGITS;
    for (int c = 0; c <= D; c++) {
        int32_t *bk = fr_entry<D>(L, st, k, c);
        const int32_t *bj = fr_entry<D>(L, st, j, c);
        long long carry = 0;
        for (int s = 0; s < top; s++) {
            long long x = carry + (s < nd ? (long long)bk[(size_t)s * ds] : 0ll);
#pragma unroll
            for (int t = 0; t < LLL_XDIGITS; t++) {
                const int src = s - sh - t;
                if (xd[t] != 0 && src >= 0 && src < nd) x -= (long long)xd[t] * (long long)bj[(size_t)src * ds];
            }
            const int32_t dg = zz_digit(x);
            carry = (x - (long long)dg) / (1ll << ZZ_DIGIT_BITS);
            if (s < nd) bk[(size_t)s * ds] = dg;
            else if (dg != 0) over = 1;
        }
        if (carry != 0) over = 1;
    }
    return over;
}

template <int D>
ZZF void fr_row_swap(int32_t *L, size_t st, int nd, int k) {
    const size_t ds = fr_digit_stride<D>(st);
    for (int c = 0; c <= D; c++) {
        int32_t *x = fr_entry<D>(L, st, k - 1, c), *y = fr_entry<D>(L, st, k, c);
        for (int s = 0; s < nd; s++) {
            const int32_t t = x[(size_t)s * ds];
            x[(size_t)s * ds] = y[(size_t)s * ds];
            y[(size_t)s * ds] = t;
        }
    }
}

// the Gram-Schmidt data of the D rows as they stand: mu[i][j] (j < i), r[i] = |b_i*|^2, sk[i] = r_i + mu_{i,i-1}^2 r_{i-1} (the Cholesky sum one term short).
// Returns false when a diagonal is not a positive finite number or a mu is not finite.
template <int D>
struct FrGs {
    mw<2> mu[D][D], r[D], sk[D];
};
template <int D>
ZZF bool fr_gram_schmidt(const int32_t *L, size_t st, int nd, FrGs<D> &g) {
    const size_t ds = fr_digit_stride<D>(st);
    mw<2> B[D][D + 1];
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
        for (int c = 0; c <= D; c++) B[i][c] = zlll::lll_entry_to_mw<2>(L + (size_t)(i * (D + 1) + c) * st, ds, nd);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < D; i++) {
        mw<2> rr[D];
#pragma unroll
        for (int j = 0; j <= i; j++) {
            mwa::acc<2> dot;
            mwa::acc_zero<2>(dot);
#pragma unroll
            for (int c = 0; c <= D; c++) mwa::acc_fma<2, 2, 2>(dot, B[i][c], B[j][c]);
            mw<2> s = mwa::acc_result<2>(dot);
#pragma unroll
            for (int t = 0; t < j; t++) {
                if (j == i && t == i - 1) g.sk[i] = s;
                s = zlll::lll_chol_sub<2>(s, g.mu[j][t], rr[t]);
            }
            rr[j] = s;
            if (j < i) {
                g.mu[i][j] = zlll::lll_chol_mu<2>(s, g.r[j]);
                ok = ok && zlll::lll_finite(g.mu[i][j].l[0]);
            } else {
                g.r[i] = s;
                ok = ok && zlll::lll_diag_ok<2>(s);
            }
        }
    }
    g.sk[0] = g.r[0];
    return ok;
}

// LLL of the lane's lattice; returns 0, FR_STEER or FR_OVERFLOW, and adds the exchanges to *exchanges
template <int D>
ZZF int fr_lll(int32_t *L, size_t st, int nd, int *exchanges) {
    int here = 0;
    for (;;) {
        FrGs<D> g;
        int pass = 0;
        for (;;) {
            if (!fr_gram_schmidt<D>(L, st, nd, g)) return FR_STEER;
            bool any = false;
#pragma unroll
            for (int k = 1; k < D; k++)
#pragma unroll
                for (int j = 0; j < k; j++) any = any || zlll::lll_exceeds<2>(g.mu[k][j], FR_ETA);
            if (!any) break;
            if (pass >= FR_MAX_PASSES) return FR_STEER;
            pass++;
#pragma unroll
            for (int k = 1; k < D; k++) {
#pragma unroll
                for (int j = k - 1; j >= 0; j--) {
                    const double X = zlll::lll_quotient<2>(g.mu[k][j]);
                    if (X == 0.0) continue;
                    int32_t xd[LLL_XDIGITS], sh;
                    if (zlll::lll_quotient_split(X, xd, &sh)) return FR_STEER;
#pragma unroll
                    for (int i = 0; i < j; i++) g.mu[k][i] = zlll::lll_mu_sub_x<2>(g.mu[k][i], g.mu[j][i], X);
                    g.mu[k][j] = mwa::add_d<2>(g.mu[k][j], -X);
                    if (fr_row_sub<D>(L, st, nd, k, j, xd, sh)) return FR_OVERFLOW;
                }
            }
        }
        int k_swap = 0;
#pragma unroll
        for (int k = D - 1; k >= 1; k--) {
            if (!zlll::lll_finite(g.sk[k].l[0])) return FR_STEER;
            if (zlll::lll_lovasz_swap<2>(g.sk[k], g.r[k - 1], FR_DELTA)) k_swap = k;
        }
        if (k_swap == 0) return 0;
        if (here >= FR_MAX_EXCHANGES) return FR_STEER;
        fr_row_swap<D>(L, st, nd, k_swap);
        here++;
        (*exchanges)++;
    }
}

// One rung of lane i.  Returns true while the lane is still running afterwards.
template <int K, int D>
ZZF bool fr_rung(const FrArgs &a, long long i) {
    int32_t *ws = a.ws + i;
    const size_t st = (size_t)a.stride;
    if (ws[0] != FR_RUNNING) return false;
    const int r = ws[st], p = 1 + 5 * r, nb = r == 0 ? 1 : 5;
    int32_t *L = ws + (size_t)(FR_HDR + a.nw) * st;
    int32_t t[D];
#pragma unroll
    for (int j = 0; j < D; j++) t[j] = fr_u_bits<D>(a, ws, j, a.P - p, nb);
    ws[st] = r + 1;
    ws[3 * st] += 1;
    int status = fr_advance<D>(L, st, a.nd, nb, t) ? FR_OVERFLOW : 0;
    if (status == 0) {
        int exchanges = ws[2 * st];
        status = fr_lll<D>(L, st, a.nd, &exchanges);
        ws[2 * st] = exchanges;
    }
    if (status != 0) {
        fr_finish<K, D>(a, i, ws, status, p, 0.0, nullptr, mwa::zero<K>());
        return false;
    }
    // acceptance: |sum_i a_i u_i| from the original numbers
    const size_t ds = fr_digit_stride<D>(st);
    mw<K> ak[D];
#pragma unroll
    for (int c = 0; c < D; c++) ak[c] = zlll::lll_entry_to_mw<K>(L + (size_t)c * st, ds, a.nd);
    mwa::acc<K> e;
    mwa::acc_zero<K>(e);
    mwa::acc_fma<K, K, K>(e, ak[0], mwa::ld<K>(a.v, (long)a.plane_v, (long)i));
    mwa::acc<K> top;
    mwa::acc_zero<K>(top);
#pragma unroll
    for (int c = 1; c < D; c++) mwa::acc_fma<K, K, K>(top, ak[c], mwa::ld<K>(a.gpow, (long)(D - 1), (long)(c - 1)));
    const mw<K> num = mwa::acc_result<K>(top);
    mwa::acc_add<K, K>(e, num);
    const double err = fabs(mwa::acc_result<K>(e).l[0]);
    if (err < a.errbound) {
        if (ak[0].l[0] == 0.0) fr_finish<K, D>(a, i, ws, FR_NO_FIELD, p, err, L, mwa::zero<K>());
        else fr_finish<K, D>(a, i, ws, FR_FOUND, p, err, L, mwa::neg<K>(mwa::div<K>(num, ak[0])));
        return false;
    }
    if (p >= a.P) {
        fr_finish<K, D>(a, i, ws, FR_EXHAUSTED, p, err, nullptr, mwa::zero<K>());
        return false;
    }
    return true;
}

// what one launch does for lane i
template <int K, int D>
ZZF void fr_lane(const FrArgs &a, long long i, int first, int launch_rungs) {
    if (first) fr_init<K, D>(a, i);
    for (int n = 0; n < launch_rungs; n++)
        if (!fr_rung<K, D>(a, i)) break;
}

}  // namespace frnd

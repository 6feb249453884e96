// clrs_minpoly_arith.h -- the minimal polynomial of a multi-word number by an integer relation among its own powers: what the reference's
// min_poly(v, d) -> clindep -> lindep does per selected kernel entry (src/find_field.jl:111-113, src/rounding.jl:481-509), DESIGN.md section 27.  One text
// for the kernel (clrs_minpoly.hip) and for a g++ build (tests/mw_host/minpoly_host.cpp), both compiled with -ffp-contract=off.
//
// Per number v and degree deg = 1 .. 4: u = (1, v, v^2, .., v^deg), D = deg + 1 entries, and a relation a_0 + a_1 v + .. + a_deg v^deg ~ 0 with small integers
// a is the first row of an LLL-reduced basis of [I | floor(2^p u)], searched at p = 1, 6, 11, .. bits.  Everything but the source of the fixed-point digits is
// clrs_mw_field_round_arith.h as it stands: fr_fixed_point, the ladder step fr_advance, the exact row operations, FrGs<D> / fr_lll<D> with (delta, eta) =
// (0.99, 0.51), the caps and the status codes.  The differences:
//
//   powers       u_1 = v as given, u_k = mul(u_(k-1), v) in K limbs (mp_power).  They are private to the number, so the digits of W_1 .. W_deg live in the
//                lane's own workspace where the field kernel reads a shared table; W_0 = 2^P needs no storage (mp_u_bits).  The powers themselves are not
//                kept: acceptance forms them again by the same products, which gives the same limbs
//   acceptance   err = |a_0 + sum_k a_k u_k| in K limbs; the first rung with err < errbound
//   status 5     the accepted relation has a_deg = 0 or a_0 = 0: v satisfies a relation of lower degree to this accuracy, or is 0
//
// Storage, element e of lane i at ws[e * stride + i]: FR_HDR header ints, the nw digits of W_1, .., of W_deg, then the lattice laid out as in the field
// kernel, digit s of row i, column c at element FR_HDR + deg nw + (s * D + i) * (D + 1) + c.
#pragma once
#include "clrs_mw_field_round_arith.h"

#define MP_NO_DEGREE FR_NO_FIELD   // status 5
#define MP_MIN_DEG 1
#define MP_MAX_DEG FR_MAX_DEG

namespace mpoly {
using frnd::mw;

ZZF int mp_ws_elems(int D, int P, int nd) { return FR_HDR + (D - 1) * frnd::fr_w_digits(P) + nd * D * (D + 1); }

struct MpArgs {
    const double *v;          // [K][plane_v]
    long long plane_v;
    int count, P, nw, nd;
    double errbound;
    int32_t *ws;              // [mp_ws_elems][stride]
    long long stride;
    int32_t *rel;             // [nd][D][plane], coefficients low to high
    int32_t *status, *rung;   // [plane]
    double *err;              // [plane]
    int32_t *info;            // [2][plane]: exchanges, rungs visited
    long long plane;
};

// the next power: u_(k+1) from u_k
template <int K>
ZZF mw<K> mp_power(const mw<K> &uk, const mw<K> &v) { return mwa::mul<K>(uk, v); }

// bits lo .. lo + n - 1 of W_i: of 2^P for i = 0, of the lane's own digits above
template <int D>
ZZF int32_t mp_u_bits(const MpArgs &a, const int32_t *ws, int i, int lo, int n) {
    if (i == 0) return (a.P >= lo && a.P - lo < n) ? (int32_t)(1 << (a.P - lo)) : 0;
    return frnd::fr_bits(ws + (size_t)(FR_HDR + (i - 1) * a.nw) * a.stride, (size_t)a.stride, a.nw, lo, n);
}

// what a lane that ends leaves in the outputs; row: the row of the relation or null
template <int D>
ZZF void mp_finish(const MpArgs &a, long long i, int32_t *ws, int status, int p, double err, const int32_t *row) {
    const size_t ds = frnd::fr_digit_stride<D>((size_t)a.stride);
    for (int s = 0; s < a.nd; s++)
#pragma unroll
        for (int c = 0; c < D; c++) a.rel[((size_t)s * D + c) * a.plane + i] = row ? row[(size_t)c * a.stride + (size_t)s * ds] : 0;
    a.status[i] = status;
    a.rung[i] = p;
    a.err[i] = err;
    a.info[i] = ws[2 * a.stride];
    a.info[a.plane + i] = ws[3 * a.stride];
    ws[0] = status;
}

// the first step of a lane: the header, W_1 .. W_deg, and the lattice [I | floor(u)] of "rung -1" (p = 0)
template <int K, int D>
ZZF void mp_init(const MpArgs &a, long long i) {
    int32_t *ws = a.ws + i;
    const size_t st = (size_t)a.stride;
    ws[0] = FR_RUNNING;
    ws[st] = 0;
    ws[2 * st] = 0;
    ws[3 * st] = 0;
    const mw<K> v = mwa::ld<K>(a.v, (long)a.plane_v, (long)i);
    if (!frnd::fr_all_finite<K>(v)) {
        mp_finish<D>(a, i, ws, FR_NOT_FINITE, 0, 0.0, nullptr);
        return;
    }
    mw<K> u = v;
    for (int k = 1; k < D; k++) {
        if (k > 1) u = mp_power<K>(u, v);
        if (!(fabs(u.l[0]) < FR_V_LIMIT)) {
            mp_finish<D>(a, i, ws, FR_OVERFLOW, 0, 0.0, nullptr);
            return;
        }
        double s[K];
#pragma unroll
        for (int l = 0; l < K; l++) s[l] = u.l[l];
        mwa::renorm<K>(s);                                   // (non-overlapping limbs: the integer sum then sees each bit once; the value is unchanged)
        mw<K> x;
#pragma unroll
        for (int l = 0; l < K; l++) x.l[l] = s[l];
        frnd::fr_fixed_point<K>(x, a.P, a.nw, ws + (size_t)(FR_HDR + (k - 1) * a.nw) * st, st);
    }
    int32_t *L = ws + (size_t)(FR_HDR + (D - 1) * a.nw) * st;
    const size_t ds = frnd::fr_digit_stride<D>(st);
#pragma unroll
    for (int r = 0; r < D; r++) {
#pragma unroll
        for (int c = 0; c <= D; c++) {
            int32_t *e = frnd::fr_entry<D>(L, st, r, c);
            int32_t d0 = c == r ? 1 : 0;
            if (c == D) {
                d0 = mp_u_bits<D>(a, ws, r, a.P, ZZ_DIGIT_BITS);
                if (d0 >= (int32_t)ZZ_HALF) d0 -= (int32_t)(1 << ZZ_DIGIT_BITS);
            }
            e[0] = d0;                                       // (|u| < 2^22: one balanced digit)
            for (int sd = 1; sd < a.nd; sd++) e[(size_t)sd * ds] = 0;
        }
    }
}

// One rung of lane i.  Returns true while the lane is still running afterwards.
template <int K, int D>
ZZF bool mp_rung(const MpArgs &a, long long i) {
    int32_t *ws = a.ws + i;
    const size_t st = (size_t)a.stride;
    if (ws[0] != FR_RUNNING) return false;
    const int r = ws[st], p = 1 + 5 * r, nb = r == 0 ? 1 : 5;
    int32_t *L = ws + (size_t)(FR_HDR + (D - 1) * a.nw) * st;
    int32_t t[D];
#pragma unroll
    for (int j = 0; j < D; j++) t[j] = mp_u_bits<D>(a, ws, j, a.P - p, nb);
    ws[st] = r + 1;
    ws[3 * st] += 1;
    int status = frnd::fr_advance<D>(L, st, a.nd, nb, t) ? FR_OVERFLOW : 0;
    if (status == 0) {
        int exchanges = ws[2 * st];
        status = frnd::fr_lll<D>(L, st, a.nd, &exchanges);
        ws[2 * st] = exchanges;
    }
    if (status != 0) {
        mp_finish<D>(a, i, ws, status, p, 0.0, nullptr);
        return false;
    }
    // acceptance: |a_0 + sum_k a_k u_k| from the powers as mp_init formed them
    const size_t ds = frnd::fr_digit_stride<D>(st);
    const mw<K> v = mwa::ld<K>(a.v, (long)a.plane_v, (long)i);
    mwa::acc<K> e;
    mwa::acc_zero<K>(e);
    const mw<K> a0 = zlll::lll_entry_to_mw<K>(L, ds, a.nd);
    mwa::acc_add<K, K>(e, a0);
    mw<K> u = v;
    double lead = 0.0;
    for (int c = 1; c < D; c++) {
        if (c > 1) u = mp_power<K>(u, v);
        const mw<K> ac = zlll::lll_entry_to_mw<K>(L + (size_t)c * st, ds, a.nd);
        mwa::acc_fma<K, K, K>(e, ac, u);
        lead = ac.l[0];
    }
    const double err = fabs(mwa::acc_result<K>(e).l[0]);
    if (err < a.errbound) {
        mp_finish<D>(a, i, ws, (a0.l[0] == 0.0 || lead == 0.0) ? MP_NO_DEGREE : FR_FOUND, p, err, L);
        return false;
    }
    if (p >= a.P) {
        mp_finish<D>(a, i, ws, FR_EXHAUSTED, p, err, nullptr);
        return false;
    }
    return true;
}

// what one launch does for lane i
template <int K, int D>
ZZF void mp_lane(const MpArgs &a, long long i, int first, int launch_rungs) {
    if (first) mp_init<K, D>(a, i);
    for (int n = 0; n < launch_rungs; n++)
        if (!mp_rung<K, D>(a, i)) break;
}

}  // namespace mpoly

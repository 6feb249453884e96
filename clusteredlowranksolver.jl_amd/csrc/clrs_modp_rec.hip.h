// clrs_modp_rec.hip.h -- the rational reconstruction of the Dixon solutions on the device (clrs_modp_dixon_reconstruct, include/clrs_hip.h; DESIGN.md
// section 16): what rounding.solve_dixon does per entry on the host after the lifting -- x_i = sum_k X[k, i] p^k by Horner, then the half-extended
// Euclidean algorithm on (m = p^K, x_i) stopped at the first remainder <= N -- with the limb arithmetic of clrs_modp_rec_arith.h spread over the lanes
// of a wave.  Included at the end of clrs_modp.hip, whose ModpBufs it uses.
//
//   k_rec_horner   one wave per entry, the lanes stride the limbs (lane t owns the limbs t, t + 64, ...).  K steps v <- v p + X[k, i], k = K - 1 .. 0, on
//                  a row of the global workspace, without rippling the carry (new_l = lo24(v_l p) + hi(v_{l-1} p): every limb stays below 2^25), over
//                  the limbs that can be non-zero at that step only; one normalisation at the end, which also finds the length.
//   k_rec_euclid   one wave per entry, no barrier, no LDS.  Four rows of the workspace: r0 = m, r1 = x_i, u0 = |t0| = 0, u1 = |t1| = 1.  While r1 > N:
//                  r0 is brought below r1 by steps (c, s), c < 2^24 (rec_quotient_window on the top limbs: never above the true quotient), each one
//                  pass r0 -= c 2^(24 s) r1 and one pass u0 += c 2^(24 s) u1; then the pairs are swapped (pointers, not rows).  Lengths live in
//                  wave-uniform registers.  The sign of t1 is the parity of the swaps.  Accepted: u1 <= D and p does not divide both r1 and u1.
//
// Carries and borrows: a pass walks the limbs low to high.  Each lane forms its limb's part alone, from two products (for the subtraction a value in
// (-2^25, 2^24), for the addition one below 3 2^24), cuts it to a digit and hands the excess to the lane above; the single units still over after that
// are settled 64 limbs at a time by carry look-ahead on two ballots (rec_wave_pass), so only scalars travel from one 64 limbs to the next and the loads
// and the lanes' work run ahead of that chain: 64 REC_GROUP limbs at a time, the next group's loads issued before this group's arithmetic.
//
// A row is written by one lane and read by another (a shift s that is no multiple of 64, the top limbs every lane reads for the estimate): the same wave,
// whose memory operations are performed in order, so a wave-scope fence (no instruction, an order for the compiler) is all that stands between.
#pragma once
#include "clrs_modp_rec_arith.h"

#define REC_NT 256                    // four waves per workgroup, one entry per wave
#define REC_WAVES (REC_NT / 64)

__device__ inline void rec_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// Every lane's v (any int32 the callers form) becomes a digit in [0, 2^24); what is over moves one lane up, `carry` enters lane 0, and what leaves lane 63
// is returned (wave-uniform).
__device__ inline int rec_wave_carry(int &v, int carry, int lane) {
    int cin = lane == 0 ? carry : 0, out = 0;
    for (;;) {
        v += cin;
        const int co = v >> REC_DIGIT_BITS;                            // (arithmetic shift: the floor, negative for a borrow)
        v &= (int)REC_MASK;
        out += __builtin_amdgcn_readlane(co, 63);
        cin = __shfl_up(co, 1, 64);
        if (lane == 0) cin = 0;
        if (!__any(cin != 0)) break;
    }
    return out;
}

// the length of v[0 .. upper): a scan from the top, 64 limbs at a time
__device__ inline int rec_wave_length(const int32_t *v, int upper, int lane) {
    for (int top = upper; top > 0; top -= 64) {
        const int l = top - 1 - lane;
        const unsigned long long nz = __ballot(l >= 0 && v[l >= 0 ? l : 0] != 0);
        if (nz) return top - (__ffsll((long long)nz) - 1);
    }
    return 0;
}

// -1, 0, 1 as a < b, a == b, a > b (la, lb lengths): the lengths first, then from the top, 64 limbs at a time, to the first limb that differs
__device__ inline int rec_wave_compare(const int32_t *a, int la, const int32_t *b, int lb, int lane) {
    if (la != lb) return la > lb ? 1 : -1;
    for (int top = la; top > 0; top -= 64) {
        const int l = top - 1 - lane;
        const int av = l >= 0 ? a[l] : 0, bv = l >= 0 ? b[l] : 0;
        const unsigned long long ne = __ballot(av != bv);
        if (ne) {
            const int f = __ffsll((long long)ne) - 1;
            return __shfl(av, f, 64) > __shfl(bv, f, 64) ? 1 : -1;
        }
    }
    return 0;
}

#define REC_GROUP 4                   // passes take 64 REC_GROUP limbs at a time: the loads of a group are in flight together, and the next group's behind them

// The limb-local parts of 64 REC_GROUP limbs from `base`: a[g] = x[l] and t[g] = lo24(c y[l - s]) + hi(c y[l - s - 1]) for l = base + 64 g + lane, zero
// where l lies outside [lo, hi) (a) or l - s outside [0, ly) (t).  Two products per limb instead of a hand-over between lanes.
__device__ inline void rec_wave_parts(const int32_t *__restrict__ x, int lo, int hi, unsigned c, int s, const int32_t *__restrict__ y, int ly, int base, int lane,
                                      int (&a)[REC_GROUP], int (&t)[REC_GROUP]) {
    unsigned b[REC_GROUP], bm[REC_GROUP];
#pragma unroll
    for (int g = 0; g < REC_GROUP; g++) {
        const int l = base + 64 * g + lane, j = l - s;
        a[g] = l >= lo && l < hi ? x[l] : 0;
        b[g] = j >= 0 && j < ly ? (unsigned)y[j] : 0u;
        bm[g] = j >= 1 && j - 1 < ly ? (unsigned)y[j - 1] : 0u;
    }
#pragma unroll
    for (int g = 0; g < REC_GROUP; g++)
        t[g] = (int)(((unsigned long long)c * b[g]) & (unsigned long long)REC_MASK) + (int)(((unsigned long long)c * bm[g]) >> REC_DIGIT_BITS);
}

// One pass x <- x -+ c 2^(24 s) y (SUB: minus) over the limbs from lo up to `end`: x is read in [lo, hi_read) and written in [lo, hi_store).  Per 64 limbs:
// every lane cuts its part v to a digit d and an excess co = floor(v / 2^24) (-2 .. 0 or 0 .. 2), takes the excess of the lane below (lane 0: of lane 63
// of the 64 limbs before) and has w = d + that in [-2, 2^24 + 1].  What is still over after that is at most one unit per lane and is settled by carry
// look-ahead on two ballots: G = the lanes that are over by themselves (w < 0, or w >= 2^24), P = the lanes that would pass a unit on (w = 0, or
// w = 2^24 - 1); the units that arrive are the carries of the 64-bit sum (G | P) + G + cin, bit i of ((G | P) + G + cin) ^ P for lane i, and the carry
// out of that sum is cin for the next 64 limbs.  So between the groups of 64 limbs only scalars are handed on, and the lanes' work of a whole group of
// REC_GROUP times 64 limbs is independent.  Returns the highest limb index + 1 that is non-zero among the limbs >= lo (at least `len`), or -1 when a
// unit is left over at the end or a non-zero limb lies at or above hi_store.
template <bool SUB>
__device__ inline int rec_wave_pass(int32_t *__restrict__ x, int lo, int hi_read, int hi_store, int end, int c, int s, const int32_t *__restrict__ y, int ly,
                                    int len, int lane) {
    int a[REC_GROUP], t[REC_GROUP], an[REC_GROUP] = {}, tn[REC_GROUP] = {};
    int prev63 = 0;                                                    // the excess of lane 63 of the 64 limbs before (wave-uniform)
    unsigned long long cin = 0;                                        // the unit that enters lane 0 from the look-ahead before
    const int first = lo & ~63;
    rec_wave_parts(x, lo, hi_read, (unsigned)c, s, y, ly, first, lane, a, t);
    for (int base = first; base < end; base += 64 * REC_GROUP) {
        if (base + 64 * REC_GROUP < end) rec_wave_parts(x, lo, hi_read, (unsigned)c, s, y, ly, base + 64 * REC_GROUP, lane, an, tn);
        int w[REC_GROUP];
        unsigned long long G[REC_GROUP], P[REC_GROUP];
#pragma unroll
        for (int g = 0; g < REC_GROUP; g++) {                          // the lanes' part, independent from one 64 to the next but for prev63
            const int v = SUB ? a[g] - t[g] : a[g] + t[g];             // in (-2^25, 2^24), or below 3 2^24
            const int co = v >> REC_DIGIT_BITS;                        // (arithmetic shift: the floor)
            int up = __shfl_up(co, 1, 64);
            if (lane == 0) up = prev63;
            prev63 = __builtin_amdgcn_readlane(co, 63);
            w[g] = (v & (int)REC_MASK) + up;
            G[g] = __ballot(SUB ? w[g] < 0 : w[g] > (int)REC_MASK);
            P[g] = __ballot(SUB ? w[g] == 0 : w[g] == (int)REC_MASK);
        }
#pragma unroll
        for (int g = 0; g < REC_GROUP; g++) {
            const int l = base + 64 * g + lane;
            const unsigned long long A = G[g] | P[g], S1 = A + G[g], S2 = S1 + cin;
            cin = (S1 < A || S2 < S1) ? 1ull : 0ull;
            const int unit = (int)(((S2 ^ P[g]) >> lane) & 1ull);
            const int d = (SUB ? w[g] - unit : w[g] + unit) & (int)REC_MASK;
            if (l >= lo && l < hi_store) x[l] = d;
            const unsigned long long nz = __ballot(l >= lo && d != 0);
            if (nz) {
                const int high = base + 64 * g + 64 - (int)__builtin_clzll(nz);
                len = high > len ? high : len;
            }
            a[g] = an[g];
            t[g] = tn[g];
        }
    }
    rec_wave_fence();
    return prev63 != 0 || cin != 0 || len > hi_store ? -1 : len;
}

// r0 <- r0 - c 2^(24 s) r1 (rec_submul).  Returns the new length of r0, -1 when the result would be negative.
__device__ inline int rec_wave_submul(int32_t *r0, int l0, int c, int s, const int32_t *r1, int l1, int lane) {
    if (l0 < l1 + s) return -1;
    if (l0 == l1 + s && (((unsigned long long)(unsigned)c * (unsigned)r1[l1 - 1]) >> REC_DIGIT_BITS) != 0) return -1;     // the product has a limb more than r0
    const int len = rec_wave_pass<true>(r0, s, l0, l0, l0, c, s, r1, l1, 0, lane);
    return len != 0 ? len : rec_wave_length(r0, s < l0 ? s : l0, lane);                   // (nothing left from s up: the length lies in the limbs below)
}

// u0 <- u0 + c 2^(24 s) u1 in a row of cap limbs (rec_addmul).  Returns the new length, -1 when the sum does not fit.
__device__ inline int rec_wave_addmul(int32_t *u0, int l0, int cap, int c, int s, const int32_t *u1, int l1, int lane) {
    if (l1 == 0) return l0;
    const int start = s < l0 ? s : l0, end = l1 + s + 2 > l0 + 1 ? l1 + s + 2 : l0 + 1;
    return rec_wave_pass<false>(u0, start, l0 < cap ? l0 : cap, cap, end, c, s, u1, l1, l0, lane);
}

// v mod p for a row of length len: every lane sums its limbs times pw[l] (at most 512 products below 2^47), then the wave
__device__ inline int rec_wave_residue(const int32_t *v, int len, const int32_t *__restrict__ pw, int p, int lane) {
    unsigned long long acc = 0;
    for (int l = lane; l < len; l += 64) acc += (unsigned long long)(unsigned)v[l] * (unsigned long long)(unsigned)pw[l];
    acc %= (unsigned long long)p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return (int)(acc % (unsigned long long)p);
}

// Entry i0 + w of the chunk: x = sum_k X[k, i] p^k into row 1 of its four workspace rows (cap limbs each), normalised, its length into xlen[w], and
// (xout != null) its digits into xout[i, 0 .. nx), nx >= Lm.
__global__ __launch_bounds__(REC_NT) void k_rec_horner(const int32_t *__restrict__ X, int n, int i0, int nc, int K, int p, int pbits, int Lm, int cap,
                                                       int32_t *__restrict__ ws, int32_t *__restrict__ xlen, int nx, int32_t *__restrict__ xout) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * REC_WAVES + (threadIdx.x >> 6);
    if (w >= nc) return;                                                                  // (wave-uniform)
    const int i = i0 + w;
    int32_t *v = ws + ((size_t)w * 4 + 1) * cap;
    for (int l = lane; l < cap; l += 64) v[l] = 0;
    int dig = 0;
    for (int j = 0; j < K; j++) {
        if ((j & 63) == 0) {                                                              // the next 64 digits, one per lane
            const int k = K - 1 - j - lane;
            dig = k >= 0 ? X[(size_t)k * n + i] : 0;
        }
        int hi_prev = __shfl(dig, j & 63, 64);                                            // the digit enters limb 0
        const int nbound = ((j + 1) * pbits + REC_DIGIT_BITS - 1) / REC_DIGIT_BITS;      // the value stays below p^(j+1) < 2^((j+1) pbits)
        const int nout = nbound < Lm ? nbound : Lm;
        for (int base = 0; base < nout; base += 64) {
            const int l = base + lane;
            const unsigned a = l < nout ? (unsigned)v[l] : 0u;                            // below 2^25
            const unsigned long long t = (unsigned long long)a * (unsigned long long)(unsigned)p;   // below 2^48
            const int hi = (int)(t >> REC_DIGIT_BITS);
            int hp = __shfl_up(hi, 1, 64);
            if (lane == 0) hp = hi_prev;
            hi_prev = __shfl(hi, 63, 64);
            if (l < nout) v[l] = (int)(t & (unsigned long long)REC_MASK) + hp;
        }
    }
    int carry = 0, len = 0;
    for (int base = 0; base < Lm; base += 64) {
        const int l = base + lane;
        int d = l < Lm ? v[l] : 0;
        carry = rec_wave_carry(d, carry, lane);
        if (l < Lm) v[l] = d;
        const unsigned long long nz = __ballot(l < Lm && d != 0);
        if (nz) len = base + 64 - (int)__builtin_clzll(nz);
    }
    if (xout) {
        int32_t *xo = xout + (size_t)i * nx;
        for (int l = lane; l < nx; l += 64) xo[l] = l < Lm ? v[l] : 0;
    }
    if (lane == 0) xlen[w] = len;
}

// Entry i0 + w of the chunk: the half-extended Euclidean algorithm on (m, x) in its four workspace rows.  N, D, m with their lengths; pw[l] = 2^(24 l) mod p.
// num, den (n x nl), neg, status, cnt (the (c, s) steps taken) are per entry; *err counts the impossibilities (a negative remainder, a cofactor past its
// row, more than maxsteps steps).
__global__ __launch_bounds__(REC_NT) void k_rec_euclid(int i0, int nc, int Lm, int cap, int32_t *ws, const int32_t *__restrict__ m, const int32_t *__restrict__ Nl, int lN,
                                                       const int32_t *__restrict__ Dl, int lD, int p, const int32_t *__restrict__ pw, const int32_t *__restrict__ xlen,
                                                       int maxsteps, int nl, int32_t *__restrict__ num, int32_t *__restrict__ den, int32_t *__restrict__ neg,
                                                       int32_t *__restrict__ status, int32_t *__restrict__ cnt, int *__restrict__ err) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * REC_WAVES + (threadIdx.x >> 6);
    if (w >= nc) return;                                                                  // (wave-uniform)
    const int i = i0 + w;
    int32_t *r0 = ws + (size_t)w * 4 * cap, *r1 = r0 + cap, *u0 = r1 + cap, *u1 = u0 + cap;
    for (int l = lane; l < Lm; l += 64) r0[l] = m[l];
    if (lane == 0) u1[0] = 1;
    rec_wave_fence();
    int l0 = Lm, l1 = xlen[w], lu0 = 0, lu1 = 1, swaps = 0, steps = 0;
    bool bad = false;
    while (!bad && rec_wave_compare(r1, l1, Nl, lN, lane) > 0) {
        for (;;) {                                                                        // r0 <- r0 mod r1, u0 <- u0 + (r0 div r1) u1, in pieces
            int s;
            int c = rec_quotient_window(r0, l0, r1, l1, &s);                              // (every lane reads the same top limbs)
            if (c == 0) {
                if (rec_wave_compare(r0, l0, r1, l1, lane) < 0) break;
                c = 1;
                s = 0;
            }
            c = __builtin_amdgcn_readfirstlane(c);
            s = __builtin_amdgcn_readfirstlane(s);
            l0 = rec_wave_submul(r0, l0, c, s, r1, l1, lane);
            lu0 = l0 < 0 ? -1 : rec_wave_addmul(u0, lu0, cap, c, s, u1, lu1, lane);
            if (lu0 < 0 || ++steps > maxsteps) {
                bad = true;
                break;
            }
        }
        int32_t *t = r0; r0 = r1; r1 = t;
        t = u0; u0 = u1; u1 = t;
        int tl = l0; l0 = l1; l1 = tl;
        tl = lu0; lu0 = lu1; lu1 = tl;
        swaps++;
    }
    bool ok = !bad && lu1 > 0 && rec_wave_compare(u1, lu1, Dl, lD, lane) <= 0;
    if (ok) ok = !(rec_wave_residue(r1, l1, pw, p, lane) == 0 && rec_wave_residue(u1, lu1, pw, p, lane) == 0);
    for (int l = lane; l < nl; l += 64) {
        num[(size_t)i * nl + l] = ok && l < l1 ? r1[l] : 0;
        den[(size_t)i * nl + l] = ok && l < lu1 ? u1[l] : 0;
    }
    if (lane == 0) {
        status[i] = ok ? 0 : 1;
        neg[i] = ok && (swaps & 1) && l1 > 0 ? 1 : 0;
        cnt[i] = steps;
        if (bad) atomicAdd(err, 1);
    }
}

static thread_local double g_rec_ms[2] = {0.0, 0.0};

// the device times of this thread's last clrs_modp_dixon_reconstruct: milliseconds in k_rec_horner and in k_rec_euclid (for the measurements)
extern "C" int clrs_modp_dixon_reconstruct_times(double *horner_ms, double *euclid_ms) {
    if (!horner_ms || !euclid_ms) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct_times: null argument");
    *horner_ms = g_rec_ms[0];
    *euclid_ms = g_rec_ms[1];
    return 0;
}

// the length of a vector of digits, or -1 when one of them lies outside [0, 2^24)
static int rec_checked_length(const int32_t *v, int count) {
    for (int l = 0; l < count; l++)
        if (v[l] < 0 || v[l] >= REC_BASE) return -1;
    return rec_length(v, count);
}

extern "C" int clrs_modp_dixon_reconstruct(int device, int n, int p, int steps, const int32_t *X, int nN, const int32_t *N_limbs, int nD, const int32_t *D_limbs,
                                           int nl, int32_t *num, int32_t *den, int32_t *neg, int32_t *status, int nx, int32_t *x_limbs, int32_t *info) {
    if (n < 0 || n > LIFT_MAX_N) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: n must lie in [0, 32767]");
    if (steps < 1) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: steps must be at least 1");
    if (!modp_prime_ok(p)) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: p must be a prime with 2 <= p < 2^23");
    if (n == 0) {
        if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
        return 0;
    }
    if (!X || !N_limbs || !D_limbs || !num || !den || !neg || !status || !info) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: null argument");
    if (nN < 1 || nD < 1 || nl < 1 || nN > REC_MAX_LIMBS || nD > REC_MAX_LIMBS || nl > REC_MAX_LIMBS)
        return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: nN, nD and nl must lie in [1, 32767]");
    const int pbits = rec_bits((unsigned long long)p);
    if ((long long)steps * pbits > (long long)REC_DIGIT_BITS * (REC_MAX_LIMBS - 1))
        return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: p^steps has more than 32767 limbs");
    const int lN = rec_checked_length(N_limbs, nN), lD = rec_checked_length(D_limbs, nD);
    if (lN < 0 || lD < 0) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: a digit of N or D outside [0, 2^24)");
    if (nl < std::max(lN, lD)) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: nl is too small for max(N, D)");
    for (size_t o = 0; o < (size_t)steps * n; o++)
        if (X[o] < 0 || X[o] >= p) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: a residue outside [0, p)");
    const int bound = rec_power_limbs_bound(p, steps);
    std::vector<int32_t> m((size_t)2 * bound + 2), tmp((size_t)2 * bound + 2);
    const int Lm = rec_power(p, steps, m.data(), tmp.data());
    if (x_limbs && nx < Lm) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_reconstruct: nx is below the " + std::to_string(Lm) + " limbs of p^steps");
    const int cap = Lm + 1;                                            // |t| r <= m for every cofactor and the remainder before it: a cofactor has at most Lm limbs
    std::vector<int32_t> pw((size_t)cap);
    rec_power_table(p, cap, pw.data());
    const long long maxsteps = std::min<long long>(200ll * Lm + 1000, 0x7fffffff);   // (c, s) steps: at most one per 24 bits of a quotient and a few corrections

    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    const size_t rows = (size_t)4 * cap;                               // ints of workspace per entry
    const int chunk = (int)std::min<size_t>((size_t)n, std::max<size_t>(((size_t)1 << 28) / rows, 1));      // at most 1 GiB of rows at a time
    int32_t *d_X = nullptr, *d_ws = nullptr, *d_m = nullptr, *d_N = nullptr, *d_D = nullptr, *d_pw = nullptr, *d_xlen = nullptr, *d_num = nullptr, *d_den = nullptr,
            *d_neg = nullptr, *d_status = nullptr, *d_cnt = nullptr, *d_xout = nullptr;
    int *d_err = nullptr;
    MODPCHECK(bufs.get(&d_X, (size_t)steps * n)); MODPCHECK(bufs.get(&d_ws, rows * chunk)); MODPCHECK(bufs.get(&d_m, (size_t)Lm));
    MODPCHECK(bufs.get(&d_N, (size_t)lN)); MODPCHECK(bufs.get(&d_D, (size_t)lD)); MODPCHECK(bufs.get(&d_pw, (size_t)cap));
    MODPCHECK(bufs.get(&d_xlen, (size_t)chunk)); MODPCHECK(bufs.get(&d_num, (size_t)n * nl)); MODPCHECK(bufs.get(&d_den, (size_t)n * nl));
    MODPCHECK(bufs.get(&d_neg, (size_t)n)); MODPCHECK(bufs.get(&d_status, (size_t)n)); MODPCHECK(bufs.get(&d_cnt, (size_t)n)); MODPCHECK(bufs.get(&d_err, (size_t)1));
    if (x_limbs) MODPCHECK(bufs.get(&d_xout, (size_t)n * nx));
    MODPCHECK(hipMemcpy(d_X, X, (size_t)steps * n * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_m, m.data(), (size_t)Lm * sizeof(int32_t), hipMemcpyHostToDevice));
    if (lN > 0) MODPCHECK(hipMemcpy(d_N, N_limbs, (size_t)lN * sizeof(int32_t), hipMemcpyHostToDevice));
    if (lD > 0) MODPCHECK(hipMemcpy(d_D, D_limbs, (size_t)lD * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_pw, pw.data(), (size_t)cap * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_err, 0, sizeof(int)));
    ModpEvents ev(3);
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    double ms[2] = {0.0, 0.0};
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int nc = std::min(chunk, n - i0);
        const dim3 grid((unsigned)((nc + REC_WAVES - 1) / REC_WAVES));
        MODPCHECK(hipEventRecord(ev.e[0], nullptr));
        hipLaunchKernelGGL(k_rec_horner, grid, dim3(REC_NT), 0, nullptr, d_X, n, i0, nc, steps, p, pbits, Lm, cap, d_ws, d_xlen, nx, d_xout);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(k_rec_euclid, grid, dim3(REC_NT), 0, nullptr, i0, nc, Lm, cap, d_ws, d_m, d_N, lN, d_D, lD, p, d_pw, d_xlen, (int)maxsteps, nl, d_num, d_den,
                           d_neg, d_status, d_cnt, d_err);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[2], nullptr));
        MODPCHECK(hipEventSynchronize(ev.e[2]));
        float a = 0.f, b = 0.f;
        MODPCHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        ms[0] += a; ms[1] += b;
    }
    g_rec_ms[0] = ms[0]; g_rec_ms[1] = ms[1];
    int err = 0;
    std::vector<int32_t> cnt((size_t)n);
    MODPCHECK(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(cnt.data(), d_cnt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(num, d_num, (size_t)n * nl * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(den, d_den, (size_t)n * nl * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(neg, d_neg, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(status, d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (x_limbs) MODPCHECK(hipMemcpy(x_limbs, d_xout, (size_t)n * nx * sizeof(int32_t), hipMemcpyDeviceToHost));
    long long most = 0, total = 0;
    for (int32_t c : cnt) { most = std::max<long long>(most, c); total += c; }
    info[0] = Lm; info[1] = (int32_t)most; info[2] = (int32_t)std::min<long long>(total, 0x7fffffff); info[3] = err;
    if (err != 0)
        return modp_fail(CLRS_ERR_HIP, "modp_dixon_reconstruct: " + std::to_string(err) + " entries met a negative remainder, a cofactor past its row or too many steps");
    return 0;
}

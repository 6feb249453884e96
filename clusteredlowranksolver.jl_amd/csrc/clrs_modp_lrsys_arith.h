// clrs_modp_lrsys_arith.h -- the index arithmetic of the low-rank system assembly clrs_zz_lowrank_system (clrs_modp_lrsys.hip.h): the
// panels the digits of a row's terms are staged in, the digits p of U that meet output digit s inside a pair of panels, and the (term, digit) of a slot of the
// MFMA's k-extent.  One text for the kernel and for a g++ build (tests/mw_host/lrsys_host.cpp), like clrs_modp_zz_arith.h, whose flush and carry walk finish
// every entry.
//
// Output digit s of entry (a, b) of row i is S_s = sum_{t in row i} sum_{p + q = s} U[a, t]_p W[b, t]_q.  The pairs (t, p) are the k-extent: slot g of a
// panel of `tc` terms whose digit s takes np values of p from plo on is term g / np, digit plo + g % np; a step of the MFMA takes four slots, one per
// lane >> 4, and slots at or past tc np load zeros.
#pragma once
#include "clrs_modp_zz_arith.h"

#define LRSYS_TILE 16                            // side of a tile of (a, b): one v_mfma_f64_16x16x4 accumulator
#define LRSYS_ROW_CAP 160                        // doubles of one row of a staged panel (terms x digits), before padding: 2 x 16 x 162 x 8 = 41472 bytes of LDS
#define LRSYS_FLUSH_MFMAS ZZ_FLUSH_MFMAS         // MFMAs an accumulator takes between two flushes
#define LRSYS_MAX_K (1 << 14)                    // max_i r_i min(ndu, ndw) stays below this: |S_s| <= K 2^46 < 2^60, doubled below 2^62

// the panels of a call: at most *tp terms, *dp digits of U and *dq digits of W are staged at a time, (*tp) max(*dp, *dq) <= LRSYS_ROW_CAP; rmax >= 1 is the
// largest number of terms of a row
ZZF void lrsys_panels(int rmax, int ndu, int ndw, int *tp, int *dp, int *dq) {
    const int nd = ndu > ndw ? ndu : ndw;
    if ((long long)rmax * nd <= LRSYS_ROW_CAP) {
        *tp = rmax; *dp = ndu; *dq = ndw;
    } else if (nd <= LRSYS_ROW_CAP) {
        *tp = LRSYS_ROW_CAP / nd; *dp = ndu; *dq = ndw;
    } else {
        *tp = 1;
        *dp = ndu < LRSYS_ROW_CAP ? ndu : LRSYS_ROW_CAP;
        *dq = ndw < LRSYS_ROW_CAP ? ndw : LRSYS_ROW_CAP;
    }
}

// the row stride (doubles) of a staged panel of `len` doubles per row: the least stride >= len that is 2 mod 32, so that the 16 rows of an operand fall on
// the 16 even residues mod 32 and a half of 32 lanes on 32 different pairs of banks (the rule of clrs_modp_tile.hip.h)
ZZF int lrsys_stride(int len) { return len + ((2 - len) % 32 + 32) % 32; }

// the digits p of U in the panel [p0, p0 + dp) whose partner q = s - p lies in the panel [q0, q0 + dq) of W: *plo <= p <= *phi; returns their number (0: none)
ZZF int lrsys_p_range(int s, int p0, int dp, int q0, int dq, int *plo, int *phi) {
    const int lo = s - (q0 + dq - 1), hi = s - q0;
    *plo = lo > p0 ? lo : p0;
    *phi = hi < p0 + dp - 1 ? hi : p0 + dp - 1;
    return *phi >= *plo ? *phi - *plo + 1 : 0;
}

// slot g of a digit with np >= 1 values of p: term *tt (relative to the panel), digit offset *pp in [0, np)
ZZF void lrsys_slot(int g, int np, int *tt, int *pp) {
    *tt = g / np;
    *pp = g - *tt * np;
}

// four slots further on (the next step of the same lane), without a division
ZZF void lrsys_slot_next(int np, int *tt, int *pp) {
    *pp += 4;
    while (*pp >= np) {
        *pp -= np;
        *tt += 1;
    }
}

// the int64 a flushed accumulator pair stands for, doubled for an entry off the diagonal
ZZF long long lrsys_value(double lo, double hi, int doubled) {
    const long long v = (long long)lo + (long long)hi * (1ll << ZZ_DIGIT_BITS);
    return doubled ? 2 * v : v;
}

// clrs_mw_zi_panels.h -- host only, nothing from HIP: how k_mwi_Zi (clrs_mw_ipm.hip.h) is launched.  A block of n rows is split into zs column panels,
// one workgroup of T threads each; MWI_ZL lanes form one entry, so one pass of the workgroup holds T / MWI_ZL entries.  The kernel gives panel y the
// columns [y pc0, min(n, (y + 1) pc0)) with pc0 = ceil(n / zs) and keeps two n x pc0 matrices of K limbs in LDS.
#pragma once
#include <algorithm>
#include <cstddef>

#define MWI_ZS 4
#ifndef MWI_ZL
#define MWI_ZL 8          // (16 lanes per entry with two-column panels -- one term per lane and product -- is slower: 0.4178 against 0.4150 ms per iteration)
#endif
#define MWI_ZT_WIDE 512      // threads of the wide form (MW_PT): two waves on every SIMD of the compute unit
#define MWI_ZT_NARROW 256    // threads of the narrow form: one wave per SIMD
// The narrow form doubles the workgroups of the launch.  It pays while every workgroup still has a compute unit of its own (the chip has 256): a product is
// then issued once per SIMD instead of twice over.  Beyond that two narrow workgroups share a compute unit, which is the wide form again with every operand
// matrix read twice.  The bound is the largest launch that was timed (whole solves, narrow against wide, at 21, 32, 64 and 96
// workgroups, 2.8-3.4 % per iteration faster each); it leaves more than half the chip to the other stream's launches.
#define MWI_ZI_NARROW_MAX_WGS 96

struct MwZiPanels {
    int zs;              // workgroups (column panels) per block: gridDim.y
    int threads;         // blockDim.x
    int pc;              // columns of a panel that fill one pass: max(1, (threads / MWI_ZL) / maxn_inv)
    int narrow;          // the narrow form was chosen
    std::size_t sm;      // dynamic LDS in bytes
};

// today's rule of the wide form: panels of one pass (want) while the launch stays near one workgroup per compute unit (320 / NB), never fewer than
// MWI_ZS panels or panels of more than eight columns (with many blocks a panel then takes several passes)
static inline int mw_zi_wide_zs(int maxn_inv, int NB) {
    const int n = std::max(maxn_inv, 1);
    const int pc = std::max(1, (MWI_ZT_WIDE / MWI_ZL) / n), want = (maxn_inv + pc - 1) / pc;
    const int old_rule = std::max(MWI_ZS, (maxn_inv + 7) / 8);
    return std::max(old_rule, std::min(want, 320 / std::max(NB, 1)));
}
// maxn_inv: largest block with an inverse factor; NB: blocks of the launch (gridDim.x); K: limbs; allow_narrow: clrs_config_set("mw_zi_narrow", ..)
static inline MwZiPanels mw_zi_panels(int maxn_inv, int NB, int K, bool allow_narrow) {
    MwZiPanels r;
    const int n = std::max(maxn_inv, 1);
    r.pc = std::max(1, (MWI_ZT_NARROW / MWI_ZL) / n);
    r.zs = (n + r.pc - 1) / r.pc;
    r.threads = MWI_ZT_NARROW;
    r.narrow = allow_narrow && maxn_inv > 0 && (long)std::max(NB, 1) * r.zs <= MWI_ZI_NARROW_MAX_WGS;
    if (!r.narrow) {
        r.pc = std::max(1, (MWI_ZT_WIDE / MWI_ZL) / n);
        r.zs = mw_zi_wide_zs(maxn_inv, NB);
        r.threads = MWI_ZT_WIDE;
    }
    r.sm = (std::size_t)2 * maxn_inv * ((maxn_inv + r.zs - 1) / r.zs) * K * 8;
    return r;
}

// The launch rule of k_mwi_Zi (csrc/clrs_mw_zi_panels.h: host only, nothing from HIP) for the host, and the columns and LDS extent of one panel written as
// the kernel's own index arithmetic (mwi_Zi_body, csrc/clrs_mw_ipm.hip.h).  Test infrastructure; compiled by tests/test_mw_zi_panel_rule_cpu.py (g++ -O2 -std=c++17).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_zi_panels.h"

// out: zs, threads, pc, narrow, sm
extern "C" void mwz_rule(int maxn_inv, int NB, int K, int allow_narrow, long *out) {
    const MwZiPanels r = mw_zi_panels(maxn_inv, NB, K, allow_narrow != 0);
    out[0] = r.zs; out[1] = r.threads; out[2] = r.pc; out[3] = r.narrow; out[4] = (long)r.sm;
}
extern "C" int mwz_lanes(void) { return MWI_ZL; }
extern "C" int mwz_narrow_max_wgs(void) { return MWI_ZI_NARROW_MAX_WGS; }

// workgroup y of zs on a block of n rows, as the kernel computes it: out = first column c0, columns pc, columns of the LDS panels pc0, passes of the
// product loops with `threads` threads, doubles of LDS the kernel addresses (M and M2: K planes of n x pc0 each)
extern "C" void mwz_kernel_panel(int n, int zs, int y, int threads, int K, long *out) {
    const int pc0 = (n + zs - 1) / zs, c0 = y * pc0, pc = std::max(0, std::min(pc0, n - c0));
    const long np = (long)n * pc0;
    int passes = 0;
    for (int e0 = 0; e0 < n * pc; e0 += threads / MWI_ZL) passes++;
    out[0] = c0; out[1] = pc; out[2] = pc0; out[3] = passes; out[4] = 2 * (long)K * np;
}

// Host restatement of the index map of the kernel-vector scatter (csrc/clrs_mw_kernel_vectors.hip.h): the SAME kv_entry the kernel k_mw_kv_scatter calls, and
// the scatter of one block written as the kernel's loop.  Test infrastructure; compiled by tests/test_kernel_vectors_cpu.py (g++ -O2 -std=c++17 -ffp-contract=off).
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_kernel_vectors.hip.h"
using namespace mwa;

extern "C" int mw_kv_entry(int branch, const int *perm, int r, int v, int j, int *row, long *widx) { return kv_entry(branch, perm, r, v, j, *row, *widx); }

extern "C" double mw_kv_max(double m, double x) { return kv_max(m, x); }

// V (planar, plane n * count, column-major n x count) from (perm, r, W) of one block (W planar, plane wplane); returns the stores made
extern "C" long mw_kv_scatter_host(int K, int branch, int n, int r, const int *perm, const double *W, long wplane, double *V) {
    const int count = branch == MW_KV_DUAL ? r : n - r;
    const long plane = (long)n * count;
    long stores = 0;
    for (long e = 0; e < plane; e++) {
        const int j = (int)(e % n), v = (int)(e / n);
        int row;
        long widx;
        const int f = kv_entry(branch, perm, r, v, j, row, widx);
        if (row < 0 || row >= n) return -1;
        for (int l = 0; l < K; l++) {
            double x;
            if (widx < 0) x = l == 0 ? (double)f : 0.0;
            else { const double w = W[l * wplane + widx]; x = f < 0 ? -w : w; }
            V[l * plane + row + (long)v * n] = x;
        }
        stores++;
    }
    return stores;
}

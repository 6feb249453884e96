// Host restatement of the multi-word SPD solve (clrs_mw_posv, csrc/clrs_mw_posv.hip.h): the SAME plan (mw_posv_plan) walked launch by launch, the product
// launches by the entry functions of k_mw_gemm (as tests/mw_host/mw_gemm_host.cpp), the diagonal blocks by the SAME text mw_posv_diag_block the kernel
// k_mw_posv_diag compiles, its lanes as loops -- so the result is the device's bit for bit.
// Test infrastructure; compiled by tests/posv_util.py (g++ -O2 -std=c++17 -ffp-contract=off).  The refusals are those of the library entry.
#include <cstdint>
#include <cstring>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_posv.hip.h"
using namespace mwa;

template <int K>
static void gemm_tiles(const MwPosvPlan &q, const MwPosvLaunch &ln, double *pool) {
    const long pl = (long)q.plane;
    for (int t = ln.tile0; t < ln.tile0 + ln.ntiles; t++) {
        const MwGemmJob &j = q.jobs[q.tiles[3 * t]];
        const int ti = q.tiles[3 * t + 1], tj = q.tiles[3 * t + 2];
        for (int gj = tj * MW_GEMM_T; gj < j.n && gj < (tj + 1) * MW_GEMM_T; gj++)
            for (int gi = ti * MW_GEMM_T; gi < j.m && gi < (ti + 1) * MW_GEMM_T; gi++) {
                acc<K + 1> s;
                acc_zero<K + 1>(s);
                const double *a = pool + j.a_off + (j.transa ? (long)gi * j.lda : (long)gi);
                const double *b = pool + j.b_off + (j.transb ? (long)gj : (long)gj * j.ldb);
                gemm_entry_accum<K>(s, j.k, a, pl, j.transa ? 1l : (long)j.lda, b, pl, j.transb ? (long)j.ldb : 1l, (double)j.alpha);
                gemm_entry_finish<K>(s, j.beta, pool + j.c_off + gi + (long)gj * j.ldc, pl);
            }
    }
}

template <int K>
static void diag(const MwPosvPlan &q, int p, double *pool, int32_t *status) {
    constexpr int T = MW_POSV_T, PL = MW_POSV_PL;
    const int n = q.n, c0 = p * T, nb = n - c0 < T ? n - c0 : T;
    const long long s = q.s_off + c0 + (long long)c0 * n, lo = q.l_off + c0 + (long long)c0 * n, w = q.w_off + (long long)p * PL;
    static thread_local double M[K * PL], W[K * PL], scr[2 * K * T];
    for (int c = 0; c < nb; c++)
        for (int i = 0; i < nb; i++)
            for (int l = 0; l < K; l++) M[l * PL + i + c * T] = i >= c ? pool[l * q.plane + s + i + (long long)c * n] : 0.0;
    int fail = 0;
    if (*status == 0) {
        fail = mw_posv_diag_block<K, double *>(M, W, scr, nb, 0, 1);
        if (fail) *status = c0 + fail;
    }
    const bool dead = *status != 0;
    for (int c = 0; c < nb; c++)
        for (int i = 0; i < nb; i++)
            for (int l = 0; l < K; l++) {
                if (i >= c) pool[l * q.plane + lo + i + (long long)c * n] = dead ? 0.0 : M[l * PL + i + c * T];
                pool[l * q.plane + w + i + c * T] = dead ? 0.0 : W[l * PL + i + c * T];
            }
}

template <int K>
static void run(int n, int nrhs, const double *A, long ap, const double *B, long bp, double *X, long xp, int32_t *info) {
    const MwPosvPlan q = mw_posv_plan(n, nrhs);
    std::vector<double> pool((size_t)q.plane * K, 0.0);
    const size_t nn = (size_t)n * n, nr = (size_t)n * nrhs;
    for (int l = 0; l < K; l++) {
        memcpy(pool.data() + (size_t)l * q.plane + q.s_off, A + (size_t)l * ap, nn * sizeof(double));
        memcpy(pool.data() + (size_t)l * q.plane + q.b_off, B + (size_t)l * bp, nr * sizeof(double));
    }
    int32_t status = 0;
    for (const MwPosvLaunch &ln : q.launches) {
        if (ln.diag) diag<K>(q, ln.panel, pool.data(), &status);
        else gemm_tiles<K>(q, ln, pool.data());
    }
    info[0] = status;
    info[1] = q.npanels;
    for (int l = 0; l < K; l++) {
        if (status) memset(X + (size_t)l * xp, 0, nr * sizeof(double));
        else memcpy(X + (size_t)l * xp, pool.data() + (size_t)l * q.plane + q.x_off, nr * sizeof(double));
    }
}

extern "C" int mw_posv_host(int K, int n, int nrhs, const double *A, int ap, const double *B, int bp, double *X, int xp, int32_t *info) {
    if (K != 4 && K != 5 && K != 6 && K != 8 && K != 10) return -1;
    if (n < 0 || nrhs < 0) return -1;
    if ((long long)ap < (long long)n * n || (long long)bp < (long long)n * nrhs || (long long)xp < (long long)n * nrhs) return -1;
    if (n == 0 || nrhs == 0) return 0;
    if (!A || !B || !X || !info) return -1;
    switch (K) {
    case 4: run<4>(n, nrhs, A, ap, B, bp, X, xp, info); return 0;
    case 5: run<5>(n, nrhs, A, ap, B, bp, X, xp, info); return 0;
    case 6: run<6>(n, nrhs, A, ap, B, bp, X, xp, info); return 0;
    case 8: run<8>(n, nrhs, A, ap, B, bp, X, xp, info); return 0;
    case 10: run<10>(n, nrhs, A, ap, B, bp, X, xp, info); return 0;
    }
    return -1;
}

// Host restatement of the batched multi-word product (csrc/clrs_mw_gemm.hip.h): a loop over the jobs and the entries of every C that calls the
// SAME entry functions the kernel k_mw_gemm calls (gemm_entry_accum / gemm_entry_finish), so its results are the device's bit for bit.
// Test infrastructure; compiled by tests/test_mw_gemm_cpu.py (g++ -O2 -std=c++17 -ffp-contract=off).  The caller checks the job list.
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_gemm.hip.h"
using namespace mwa;

template <int K>
static void run(int njobs, const MwGemmJob *jobs, const double *A, long ap, const double *B, long bp, double *C, long cp) {
    for (int t = 0; t < njobs; t++) {
        const MwGemmJob &q = jobs[t];
        for (int j = 0; j < q.n; j++)
            for (int i = 0; i < q.m; i++) {
                acc<K + 1> s;
                acc_zero<K + 1>(s);
                const double *a = A + q.a_off + (q.transa ? (long)i * q.lda : (long)i);
                const double *b = B + q.b_off + (q.transb ? (long)j : (long)j * q.ldb);
                gemm_entry_accum<K>(s, q.k, a, ap, q.transa ? 1l : (long)q.lda, b, bp, q.transb ? (long)q.ldb : 1l, (double)q.alpha);
                gemm_entry_finish<K>(s, q.beta, C + q.c_off + i + (long)j * q.ldc, cp);
            }
    }
}

extern "C" int mw_gemm_host(int K, int njobs, const MwGemmJob *jobs, const double *A, long ap, const double *B, long bp, double *C, long cp) {
    switch (K) {
    case 4: run<4>(njobs, jobs, A, ap, B, bp, C, cp); return 0;
    case 5: run<5>(njobs, jobs, A, ap, B, bp, C, cp); return 0;
    case 6: run<6>(njobs, jobs, A, ap, B, bp, C, cp); return 0;
    case 8: run<8>(njobs, jobs, A, ap, B, bp, C, cp); return 0;
    case 10: run<10>(njobs, jobs, A, ap, B, bp, C, cp); return 0;
    }
    return -1;
}

// clrs_modp_liftm.hip.h -- Dixon's p-adic lifting of an integer system A X = B with a MATRIX of right-hand sides (clrs_modp_dixon_lift_multi, include/clrs_hip.h;
// DESIGN.md section 19): the exact solve behind the inverse over QQ of the reference's basis_transformations (src/rounding.jl:836).  Included at the end of
// clrs_modp.hip behind clrs_modp_zz_gemm.hip.h: it uses the buffers of clrs_modp.hip, the inverse mod p and k_lift_gather of clrs_modp_lift.hip.h, the tile loop and k_zz_gemm.
//
// Per column j the result is by definition that of clrs_modp_dixon_lift on b = B[:, j].  What changes is the shape of the work: with m columns side by side
// the two products of a step are matrix products whose operands are reused from LDS, not m matrix-vector products that each read A and A^-1 mod p once.
//
//   setup      lift_inverse_modp of clrs_modp_lift.hip.h ([A mod p | I] by k_lift_residues, modp_eliminate), then k_lift_gather writes the right half in pivot-row
//              order as fp64: Cd = A^-1 mod p (n x n).
//              The digit planes of A are widened once to fp64, A' = [A_0; ...; A_{nd-1}] ((nd n) x n, the planes as they lie).
//   per chunk of columns (mc of them):  R_0 = B[:, chunk] as limbs [(nrl + 1)][n][mc], Rbar = R_0 mod p as fp64 (n x mc), and per step k, three launches:
//     k_liftm_x    X_k = Cd Rbar mod p           the hot path: the tile loop of clrs_modp_tile.hip.h (a tiled fp64 GEMM on v_mfma_f64_16x16x4), as in k_zz_gemm;
//                                                writes X_k as int32 (row k of the chunk's X) and as fp64 (Xd)
//     k_zz_gemm    P = A' Xd as (lo, hi) pairs   (nd n) x mc, unchanged
//     k_liftm_r    R <- (R - A X_k) / p          one thread per entry: liftm_entry (clrs_modp_lift_arith.h); leaves Rbar = R mod p for the next step
//   on one stream with no host synchronisation between the steps.
//
// Exactness of k_liftm_x: both operands are residues in [0, p), p < 2^23, so a product is below 2^46 and one MFMA adds four of them.  An accumulator that holds
// a residue (below 2^23) plus 4 F products stays below 2^23 + F 2^48 <= 2^53 - 2^48 + 2^23 < 2^53 for F <= 31: every partial sum is an integer below 2^53 and the
// fp64 sum is exact in any order.  Every accumulator is reduced by modp_reduce after LIFTM_REDUCE_STEPS steps of k-extent 16 (28 MFMAs) and once at the end.
//
// The lifting of a column does not depend on the other columns: m is cut into chunks so that P, Xd, Rbar and the chunk's R stay below LIFTM_CHUNK_BYTES (256 MiB;
// clrs_config_set("liftm_chunk_bytes", b) lowers it, for the tests; a chunk is never less than one column); the chunks run one after the other and share the setup.
#pragma once

#define LIFTM_NT 256
#define LIFTM_REDUCE_MFMAS 28                                        // MFMAs an accumulator of k_liftm_x takes between two reductions: seven steps
#define LIFTM_REDUCE_STEPS (LIFTM_REDUCE_MFMAS / (ZZ_BK / 4))
#define LIFTM_CHUNK_BYTES ((size_t)256 << 20)

// a residue below 2^23 plus four products of residues (each below 2^46) per MFMA must stay below 2^53 between two reductions
static_assert(LIFTM_REDUCE_STEPS >= 1 && (1ll << MODP_MAX_PRIME_BITS) + 4ll * LIFTM_REDUCE_STEPS * (ZZ_BK / 4) * (1ll << (2 * MODP_MAX_PRIME_BITS)) < (1ll << 53),
              "an accumulator of k_liftm_x must stay below 2^53 between two reductions");

extern int g_cfg_liftm_chunk_bytes;            // clrs_hip.hip, clrs_config_set("liftm_chunk_bytes", bytes): 0 = LIFTM_CHUNK_BYTES

// X[r, c] = sum_kk A[r, kk] B[kk, c] mod p for r < M, c < N; A is M x K residues (row stride K), B is K x N residues (row stride N); the result as int32 into Xi
// and as fp64 into Xd (both M x N).  The main loop is zz_tile_loop (clrs_modp_tile.hip.h), reduced mod p every LIFTM_REDUCE_STEPS steps; a flat grid of `colblocks` workgroups
// per row of tiles.  One code path: rows >= M, columns >= N and k >= K load zeros, stores are masked.
__global__ __launch_bounds__(LIFTM_NT) void k_liftm_x(const double *__restrict__ A, int M, int K, const double *__restrict__ B, int N, int p_int,
                                                      int32_t *__restrict__ Xi, double *__restrict__ Xd, int colblocks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int by = blockIdx.x / colblocks, bx = blockIdx.x - by * colblocks;
    const int row0 = by * ZZ_BM, col0 = bx * ZZ_BN;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const double p = (double)p_int, pinv = 1.0 / p;
    modp_v4d acc[2][2];
    zz_tile_loop<LIFTM_REDUCE_STEPS>(A, M, K, B, N, 0, N, row0, col0, acc, [&](modp_v4d (&t)[2][2]) {
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 2; tj++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) t[ti][tj][reg] = modp_reduce(t[ti][tj][reg], p, pinv);
    });
    // accumulator: column l & 15, row (l >> 4) + 4 reg
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r = row0 + wr + 16 * ti + l4 + 4 * reg, c = col0 + wc + 16 * tj + l15;
                const double x = modp_reduce(acc[ti][tj][reg], p, pinv);                   // (a residue reduces to itself)
                if (r < M && c < N) {
                    Xi[(size_t)r * N + c] = (int32_t)x;
                    Xd[(size_t)r * N + c] = x;
                }
            }
}

// Entry e = i mc + j of R <- (R - A X_k) / p from P = A' Xd ((nd n) x mc pairs; plane l of A at rows l n ...): liftm_entry, then rbar[e] = R[e] mod p as fp64.
// cnt[0] counts divisions that left a remainder, cnt[1] entries whose result does not fit in nrl limbs: both must stay 0.
__global__ __launch_bounds__(LIFTM_NT) void k_liftm_r(const double2 *__restrict__ P, size_t entries, int nd, int nrl, int p, const int32_t *__restrict__ pw,
                                                      int32_t *__restrict__ r, double *__restrict__ rbar, int *__restrict__ cnt) {
    const size_t e = (size_t)blockIdx.x * LIFTM_NT + threadIdx.x;
    if (e >= entries) return;
    int flags;
    rbar[e] = (double)liftm_entry((const double *)(P + e), entries, nd, r + e, entries, nrl, p, pw, &flags);
    if (flags & 1) atomicAdd(cnt, 1);
    if (flags & 2) atomicAdd(cnt + 1, 1);
}

static thread_local double g_liftm_ms[4] = {0.0, 0.0, 0.0, 0.0};

// the device times of this thread's last clrs_modp_dixon_lift_multi: milliseconds in k_liftm_x, in k_zz_gemm and in k_liftm_r over all steps and chunks, and from
// the first upload to the last download (device events)
extern "C" int clrs_modp_dixon_lift_multi_times(double *x_ms, double *gemm_ms, double *r_ms, double *whole_ms) {
    if (!x_ms || !gemm_ms || !r_ms || !whole_ms) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_lift_multi_times: null argument");
    *x_ms = g_liftm_ms[0];
    *gemm_ms = g_liftm_ms[1];
    *r_ms = g_liftm_ms[2];
    *whole_ms = g_liftm_ms[3];
    return 0;
}

extern "C" int clrs_modp_dixon_lift_multi(int device, int n, int m, int p, int nd, const int32_t *A_digits, int nbl, const int32_t *B_limbs, int steps, int32_t *X,
                                          int32_t *R_limbs, int32_t *info) {
    const char *who = "modp_dixon_lift_multi";
    if (int code = lift_check_sizes(who, n, m, nd, nbl, steps, p)) return code;
    const int nrl = std::max(nbl, nd + 1) + 1, nt = nrl + 1;
    const unsigned long long lim = 1ull << 31, nm = (unsigned long long)n * (unsigned long long)m;
    if ((unsigned long long)nd * n * n >= lim || (unsigned long long)nbl * nm >= lim || (unsigned long long)steps * nm >= lim || (unsigned long long)nt * nm >= lim)
        return modp_fail(CLRS_ERR_INVALID, "modp_dixon_lift_multi: an operand or a result has 2^31 elements or more");
    if (n == 0 || m == 0) {                                    // nothing to lift: zeros, without a device (the rank of A is not examined)
        if (info) { info[0] = 0; info[1] = steps; info[2] = 0; info[3] = 0; info[4] = 0; info[5] = 0; }
        g_liftm_ms[0] = g_liftm_ms[1] = g_liftm_ms[2] = g_liftm_ms[3] = 0.0;
        return 0;
    }
    if (!A_digits || !B_limbs || !R_limbs || !info || (!X && steps > 0)) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_lift_multi: null argument");
    const size_t nn = (size_t)n * n;
    if (int code = lift_check_digits(who, "a digit of A", A_digits, (size_t)nd * nn)) return code;
    if (int code = lift_check_digits(who, "a limb of B", B_limbs, (size_t)nbl * (size_t)nm)) return code;
    std::vector<int32_t> pw((size_t)std::max(nd, nt));
    lift_power_table(p, (int)pw.size(), pw.data());
    // the columns of a chunk: P (16 nd n bytes per column), Xd and Rbar (8 n each) and the limbs of R (4 (nrl + 1) n) stay below the bound
    const size_t bound = modp_chunk_bound(g_cfg_liftm_chunk_bytes, LIFTM_CHUNK_BYTES);
    const size_t percol = (size_t)n * ((size_t)nd * sizeof(double2) + 2 * sizeof(double) + (size_t)nt * sizeof(int32_t));
    const int mc_max = (int)std::min<size_t>((size_t)m, std::max<size_t>(bound / percol, 1));

    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    ModpEvents ev((size_t)3 * steps + 3);                      // [0], [1]: the whole call; [2 + 3 k + t]: before launch t of step k, [2 + 3 steps]: after the last
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    hipEvent_t *step_ev = ev.e.data() + 2;
    int32_t *d_Ai = nullptr, *d_pw = nullptr, *d_r = nullptr, *d_X = nullptr;
    double *d_M = nullptr, *d_Cd = nullptr, *d_Ap = nullptr, *d_Xd = nullptr, *d_rbar = nullptr;
    double2 *d_P = nullptr;
    int *d_order = nullptr, *d_cnt = nullptr;                           // cnt: [0] remainders, [1] limb overflows, [2] impossible GEMM pairs
    MODPCHECK(hipEventRecord(ev.e[0], nullptr));
    MODPCHECK(bufs.get(&d_Ai, (size_t)nd * nn)); MODPCHECK(bufs.get(&d_pw, pw.size()));
    MODPCHECK(hipMemcpy(d_Ai, A_digits, (size_t)nd * nn * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_pw, pw.data(), pw.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    int rank = 0;
    if (int code = lift_inverse_modp(d_Ai, n, n, nd, p, d_pw, bufs, &d_M, &d_order, &rank)) return code;      // (row pitch n: the planes as they lie)
    if (rank < n) {
        info[0] = rank; info[1] = 0; info[2] = 0; info[3] = 0; info[4] = 0; info[5] = 0;
        g_liftm_ms[0] = g_liftm_ms[1] = g_liftm_ms[2] = g_liftm_ms[3] = 0.0;
        return 0;
    }
    MODPCHECK(bufs.get(&d_Cd, nn)); MODPCHECK(bufs.get(&d_Ap, (size_t)nd * nn));
    hipLaunchKernelGGL(k_lift_gather<double>, modp_flat_grid(nn, LIFT_NT), dim3(LIFT_NT), 0, nullptr, d_M, n, n, d_order, d_Cd);
    MODPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_modp_widen, modp_flat_grid((size_t)nd * nn, MODP_NT), dim3(MODP_NT), 0, nullptr, d_Ai, d_Ap, (size_t)nd * nn);
    MODPCHECK(hipGetLastError());
    MODPCHECK(bufs.drop(d_M)); MODPCHECK(bufs.drop(d_Ai));     // (hipFree waits for the gather and the widening)
    d_M = nullptr; d_Ai = nullptr;

    const size_t ce_max = (size_t)n * mc_max;                  // entries of a chunk
    MODPCHECK(bufs.get(&d_r, (size_t)nt * ce_max)); MODPCHECK(bufs.get(&d_rbar, ce_max)); MODPCHECK(bufs.get(&d_Xd, ce_max));
    MODPCHECK(bufs.get(&d_P, (size_t)nd * ce_max)); MODPCHECK(bufs.get(&d_X, (size_t)steps * ce_max)); MODPCHECK(bufs.get(&d_cnt, (size_t)3));
    MODPCHECK(hipMemset(d_cnt, 0, 3 * sizeof(int)));
    std::vector<int32_t> r0((size_t)nt * ce_max);
    std::vector<double> rbar0(ce_max);
    const int xrowtiles = (n + ZZ_BM - 1) / ZZ_BM, prowtiles = (int)(((size_t)nd * n + ZZ_BM - 1) / ZZ_BM);
    double ms[3] = {0.0, 0.0, 0.0};
    int chunks = 0;
    for (int j0 = 0; j0 < m; j0 += mc_max) {
        const int mc = std::min(mc_max, m - j0);
        const size_t ce = (size_t)n * mc;
        // R_0 = B[:, j0 .. j0 + mc) and its residues
        std::fill(r0.begin(), r0.begin() + (size_t)nt * ce, 0);
        for (int l = 0; l < nbl; l++)
            for (int i = 0; i < n; i++)
                std::copy(B_limbs + ((size_t)l * n + i) * m + j0, B_limbs + ((size_t)l * n + i) * m + j0 + mc, r0.begin() + (size_t)l * ce + (size_t)i * mc);
        for (size_t e = 0; e < ce; e++) rbar0[e] = (double)lift_residue(r0.data() + e, ce, nrl, pw.data(), p);
        MODPCHECK(hipMemcpy(d_r, r0.data(), (size_t)nt * ce * sizeof(int32_t), hipMemcpyHostToDevice));
        MODPCHECK(hipMemcpy(d_rbar, rbar0.data(), ce * sizeof(double), hipMemcpyHostToDevice));
        const int colblocks = (mc + ZZ_BN - 1) / ZZ_BN;
        for (int k = 0; k < steps; k++) {
            MODPCHECK(hipEventRecord(step_ev[3 * k], nullptr));
            hipLaunchKernelGGL(k_liftm_x, dim3((unsigned)xrowtiles * (unsigned)colblocks), dim3(LIFTM_NT), 0, nullptr, d_Cd, n, n, d_rbar, mc, p, d_X + (size_t)k * ce,
                               d_Xd, colblocks);
            MODPCHECK(hipEventRecord(step_ev[3 * k + 1], nullptr));
            hipLaunchKernelGGL(k_zz_gemm, dim3((unsigned)prowtiles * (unsigned)colblocks), dim3(ZZ_NT), 0, nullptr, d_Ap, nd * n, n, d_Xd, (size_t)mc, (size_t)0, mc,
                               d_P, colblocks, d_cnt + 2);
            MODPCHECK(hipEventRecord(step_ev[3 * k + 2], nullptr));
            hipLaunchKernelGGL(k_liftm_r, dim3((unsigned)((ce + LIFTM_NT - 1) / LIFTM_NT)), dim3(LIFTM_NT), 0, nullptr, d_P, ce, nd, nrl, p, d_pw, d_r, d_rbar, d_cnt);
            MODPCHECK(hipGetLastError());                      // (host side only: a refused launch ends the loop at its step)
        }
        MODPCHECK(hipEventRecord(step_ev[3 * steps], nullptr));
        MODPCHECK(hipStreamSynchronize(nullptr));
        for (int k = 0; k < steps; k++)
            for (int t = 0; t < 3; t++) {
                float a = 0.f;
                MODPCHECK(hipEventElapsedTime(&a, step_ev[3 * k + t], step_ev[3 * k + t + 1]));
                ms[t] += a;
            }
        if (steps > 0)
            MODPCHECK(hipMemcpy2D(X + j0, (size_t)m * sizeof(int32_t), d_X, (size_t)mc * sizeof(int32_t), (size_t)mc * sizeof(int32_t), (size_t)steps * n,
                                  hipMemcpyDeviceToHost));
        MODPCHECK(hipMemcpy2D(R_limbs + j0, (size_t)m * sizeof(int32_t), d_r, (size_t)mc * sizeof(int32_t), (size_t)mc * sizeof(int32_t), (size_t)nrl * n,
                              hipMemcpyDeviceToHost));
        chunks++;
    }
    int cnt[3] = {0, 0, 0};
    MODPCHECK(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    MODPCHECK(hipEventRecord(ev.e[1], nullptr));
    MODPCHECK(hipEventSynchronize(ev.e[1]));
    float whole = 0.f;
    MODPCHECK(hipEventElapsedTime(&whole, ev.e[0], ev.e[1]));
    g_liftm_ms[0] = ms[0]; g_liftm_ms[1] = ms[1]; g_liftm_ms[2] = ms[2]; g_liftm_ms[3] = whole;
    info[0] = rank; info[1] = steps; info[2] = cnt[0]; info[3] = cnt[1]; info[4] = chunks; info[5] = cnt[2];
    if (cnt[2] != 0) return modp_fail(CLRS_ERR_HIP, "modp_dixon_lift_multi: " + std::to_string(cnt[2]) + " accumulators of A X that are no integers below 2^53");
    if (cnt[0] != 0 || cnt[1] != 0)
        return modp_fail(CLRS_ERR_HIP, "modp_dixon_lift_multi: " + std::to_string(cnt[0]) + " divisions by p left a remainder and " + std::to_string(cnt[1]) +
                                           " residuals left their limbs: the lifting is not exact");
    return 0;
}

// clrs_modp_lrsys.hip.h -- the rows of the rational linear system of the rounding chain from low-rank constraint matrices (clrs_zz_lowrank_system,
// include/clrs_hip.h; the reference's partial_linearsystem, src/interface.jl:1354-1535, after the basis change and cleared of
// denominators): C[i, c] = 2^(a_c != b_c) sum_{t in row i} U[a_c, t] W[b_c, t] for long integers given in balanced base-2^24 digit planes.  No context, host
// pointers.  Included at the end of clrs_modp.hip behind clrs_modp_zz_gemm.hip.h, whose ZZ_NT and ZZ_MAX_DIGITS it uses beside ModpBufs, MODPCHECK, modp_fail.
//
//   k_lrsys_tile   the hot path: one workgroup of four waves per (row i, 16 x 16 tile of (a, b) that holds a selected column).  The digits of the 16 rows
//                  of U and of W for the terms of row i are staged in LDS as fp64 (in panels of terms and digits when they do not fit: lrsys_panels); the
//                  waves share the output digits s; per s the k-extent of v_mfma_f64_16x16x4 runs over the pairs (term, digit p of U) with the partner
//                  digit s - p of W (clrs_modp_lrsys_arith.h).  The accumulator is flushed after 28 MFMAs and at the end (clrs_modp_zz_arith.h), and
//                  lo + hi 2^24, doubled off the diagonal, is added to the int64 S[s][i][c].  A (row, tile, s) belongs to one wave and an entry to one
//                  lane of it, whatever the panel: plain loads and stores, no atomics but the counter of impossible pairs.
//   k_lrsys_carry  one thread per entry of C: zz_carry_walk upward through the planes of S.
//
// S takes 8 (ndu + ndw - 1) nc bytes per row: the rows are cut into chunks so that S stays below LRSYS_CHUNK_BYTES (256 MiB;
// clrs_config_set("lrsys_chunk_bytes", b) lowers it, for the tests; a chunk is never less than one row).  Rows do not meet, so the result does not depend on
// the chunks.
#pragma once

#include "clrs_modp_lrsys_arith.h"

#define LRSYS_CHUNK_BYTES ((size_t)256 << 20)

static_assert(LRSYS_FLUSH_MFMAS >= 1 && LRSYS_FLUSH_MFMAS <= ZZ_MAX_FLUSH_MFMAS, "an accumulator takes at most 31 MFMAs between two flushes");
static_assert(ZZ_NT == 256 && LRSYS_TILE == 16, "k_lrsys_tile: four waves, one 16 x 16 accumulator each");

extern int g_cfg_lrsys_chunk_bytes;            // clrs_hip.hip, clrs_config_set("lrsys_chunk_bytes", bytes): 0 = LRSYS_CHUNK_BYTES

// Workgroup blockIdx.x = il ntiles + tile: row i = i0 + il of the system, tile (tiles[2 tile], tiles[2 tile + 1]) of (a, b).  U is [ndu][n][T], W [ndw][n][T];
// map[a n + b] is the column of S of the pair (a, b) or -1; S is [ndu + ndw - 1][rows of the chunk][nc], zero before the launch.  tp, dp, dq: lrsys_panels.
// Dynamic LDS: 16 (lrsys_stride(tp dp) + lrsys_stride(tp dq)) doubles.
__global__ __launch_bounds__(ZZ_NT) void k_lrsys_tile(int n, int T, const int32_t *__restrict__ rowptr, int i0, int rows, int ndu, const int32_t *__restrict__ U,
                                                      int ndw, const int32_t *__restrict__ W, const int32_t *__restrict__ tiles, int ntiles,
                                                      const int32_t *__restrict__ map, int nc, long long *__restrict__ S, int tp, int dp, int dq,
                                                      int *__restrict__ err) {
    extern __shared__ double lrsys_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int il = blockIdx.x / ntiles, tile = blockIdx.x - il * ntiles;
    const int t_begin = rowptr[i0 + il], t_end = rowptr[i0 + il + 1];
    const int a0 = tiles[2 * tile] * LRSYS_TILE, b0 = tiles[2 * tile + 1] * LRSYS_TILE;
    const int ldu = lrsys_stride(tp * dp), ldw = lrsys_stride(tp * dq);
    double *Us = lrsys_lds, *Ws = lrsys_lds + LRSYS_TILE * ldu;
    // the columns of S of this lane's four entries: row a0 + l4 + 4 reg, column b0 + l15 (the accumulator layout of clrs_modp_tile.hip.h)
    int col[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int a = a0 + l4 + 4 * reg, b = b0 + l15;
        col[reg] = (a < n && b < n) ? map[(size_t)a * n + b] : -1;
    }
    int bad = 0;
    for (int t0 = t_begin; t0 < t_end; t0 += tp) {
        const int tc = t_end - t0 < tp ? t_end - t0 : tp;
        for (int p0 = 0; p0 < ndu; p0 += dp) {
            const int dpc = ndu - p0 < dp ? ndu - p0 : dp;
            for (int q0 = 0; q0 < ndw; q0 += dq) {
                const int dqc = ndw - q0 < dq ? ndw - q0 : dq;
                __syncthreads();                                                           // the panels before are read
                // Us[r][tt dp + pp] = U[p0 + pp][a0 + r][t0 + tt], Ws[r][tt dq + qq] = W[q0 + qq][b0 + r][t0 + tt]; rows >= n are zero
                for (int e = tid; e < LRSYS_TILE * tc * dpc; e += ZZ_NT) {
                    const int tt = e % tc, rest = e / tc, r = rest % LRSYS_TILE, pp = rest / LRSYS_TILE;
                    Us[r * ldu + tt * dp + pp] = a0 + r < n ? (double)U[((size_t)(p0 + pp) * n + a0 + r) * T + t0 + tt] : 0.0;
                }
                for (int e = tid; e < LRSYS_TILE * tc * dqc; e += ZZ_NT) {
                    const int tt = e % tc, rest = e / tc, r = rest % LRSYS_TILE, qq = rest / LRSYS_TILE;
                    Ws[r * ldw + tt * dq + qq] = b0 + r < n ? (double)W[((size_t)(q0 + qq) * n + b0 + r) * T + t0 + tt] : 0.0;
                }
                __syncthreads();
                for (int s = p0 + q0 + wave; s <= p0 + dpc - 1 + q0 + dqc - 1; s += ZZ_NT / 64) {      // (uniform in the wave)
                    int plo, phi;
                    const int np = lrsys_p_range(s, p0, dpc, q0, dqc, &plo, &phi);       // >= 1 for every s of this range
                    const int slots = tc * np;
                    modp_v4d acc = {0.0, 0.0, 0.0, 0.0}, hi = {0.0, 0.0, 0.0, 0.0};
                    int tt, pp, mfmas = 0;
                    lrsys_slot(l4, np, &tt, &pp);
                    for (int g0 = 0; g0 < slots; g0 += 4) {
                        // operands: lane l holds U[a0 + (l & 15), term, digit p] and W[b0 + (l & 15), term, digit s - p] of slot g0 + (l >> 4)
                        double av = 0.0, bv = 0.0;
                        if (g0 + l4 < slots) {
                            const int p = plo + pp;
                            av = Us[l15 * ldu + tt * dp + (p - p0)];
                            bv = Ws[l15 * ldw + tt * dq + (s - p - q0)];
                        }
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                        lrsys_slot_next(np, &tt, &pp);
                        if (++mfmas == LRSYS_FLUSH_MFMAS) {                                // (uniform)
                            mfmas = 0;
#pragma unroll
                            for (int reg = 0; reg < 4; reg++) {
                                double a = acc[reg], h = hi[reg];
                                zz_flush(&a, &h);
                                acc[reg] = a; hi[reg] = h;
                            }
                        }
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        double a = acc[reg], h = hi[reg];
                        zz_flush(&a, &h);
                        if (col[reg] >= 0) {
                            bad += zz_pair_bad(a, h);
                            long long *dst = S + ((size_t)s * rows + il) * nc + col[reg];
                            *dst += lrsys_value(a, h, a0 + l4 + 4 * reg != b0 + l15);
                        }
                    }
                }
            }
        }
    }
    if (bad) atomicAdd(err, bad);
}

// C[ndc][R][nc] for the rows [i0, i0 + rows) from S[ns][rows][nc]; entry (il, c) reads the column canon[c] of S; *over counts the entries that do not fit
__global__ __launch_bounds__(ZZ_NT) void k_lrsys_carry(const long long *__restrict__ S, int ns, int rows, int nc, const int32_t *__restrict__ canon, int i0, int R,
                                                       int32_t *__restrict__ C, int ndc, int *__restrict__ over) {
    const size_t e = (size_t)blockIdx.x * ZZ_NT + threadIdx.x;
    if (e >= (size_t)rows * nc) return;
    const size_t il = e / nc, c = e - il * nc;
    if (zz_carry_walk(S + il * nc + canon[c], (size_t)rows * nc, ns, C + ((size_t)i0 + il) * nc + c, (size_t)R * nc, ndc)) atomicAdd(over, 1);
}

static thread_local double g_lrsys_ms[3] = {0.0, 0.0, 0.0};

// the device times of this thread's last clrs_zz_lowrank_system: milliseconds in k_lrsys_tile, in k_lrsys_carry, and from the first upload to the last download
extern "C" int clrs_zz_lowrank_system_times(double *tile_ms, double *carry_ms, double *whole_ms) {
    if (!tile_ms || !carry_ms || !whole_ms) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system_times: null argument");
    *tile_ms = g_lrsys_ms[0];
    *carry_ms = g_lrsys_ms[1];
    *whole_ms = g_lrsys_ms[2];
    return 0;
}

extern "C" int clrs_zz_lowrank_system(int device, int n, int T, int R, const int32_t *rowptr, int ndu, const int32_t *U, int ndw, const int32_t *W, int nc,
                                      const int32_t *col_a, const int32_t *col_b, int ndc, int32_t *C, int32_t *info) {
    if (n < 0 || T < 0 || R < 0 || nc < 0) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: negative size");
    if (ndu < 1 || ndu > ZZ_MAX_DIGITS || ndw < 1 || ndw > ZZ_MAX_DIGITS || ndc < 1 || ndc > ZZ_MAX_DIGITS)
        return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: ndu, ndw and ndc must lie in [1, 32767]");
    const unsigned long long lim = 1ull << 31;
    const unsigned long long nu = (unsigned long long)ndu * n * T, nw = (unsigned long long)ndw * n * T, nout = (unsigned long long)ndc * R * nc;
    const int ns = ndu + ndw - 1;
    if (nu >= lim || nw >= lim || nout >= lim || (unsigned long long)n * n >= lim || (unsigned long long)ns * nc >= lim || (unsigned long long)n + LRSYS_TILE >= lim)
        return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: an operand, the result, the map of pairs or a row of sums has 2^31 elements or more");
    if (!info || !rowptr || (nu && !U) || (nw && !W) || (nc && (!col_a || !col_b)) || (nout && !C)) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: null argument");
    if (rowptr[0] != 0 || rowptr[R] != T) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: rowptr must start at 0 and end at T");
    int rmax = 0;
    for (int i = 0; i < R; i++) {
        if (rowptr[i + 1] < rowptr[i]) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: rowptr decreases");
        rmax = std::max(rmax, rowptr[i + 1] - rowptr[i]);
    }
    if ((long long)rmax * std::min(ndu, ndw) >= LRSYS_MAX_K) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: (terms of a row) * min(ndu, ndw) must be below 2^14");
    for (int c = 0; c < nc; c++)
        if (col_a[c] < 0 || col_a[c] > col_b[c] || col_b[c] >= n) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: a pair needs 0 <= a <= b < n");
    for (size_t o = 0; o < (size_t)nu; o++)
        if (U[o] < -(1 << 23) || U[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: a digit of U outside [-2^23, 2^23]");
    for (size_t o = 0; o < (size_t)nw; o++)
        if (W[o] < -(1 << 23) || W[o] > (1 << 23)) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: a digit of W outside [-2^23, 2^23]");
    if (R == 0 || nc == 0 || T == 0) {                                                     // nothing to sum: zeros, without a device
        std::fill(C, C + (size_t)nout, 0);
        info[0] = info[1] = info[2] = info[3] = 0;
        g_lrsys_ms[0] = g_lrsys_ms[1] = g_lrsys_ms[2] = 0.0;
        return 0;
    }
    // the map (a, b) -> column of S (the first column that selects the pair), the column of S of every column of C, and the tiles that hold a selected pair
    const int nt = (n + LRSYS_TILE - 1) / LRSYS_TILE;
    std::vector<int32_t> map((size_t)n * n, -1), canon((size_t)nc), tiles;
    std::vector<char> used((size_t)nt * nt, 0);
    for (int c = 0; c < nc; c++) {
        int32_t &slot = map[(size_t)col_a[c] * n + col_b[c]];
        if (slot < 0) slot = c;
        canon[c] = slot;
        used[(size_t)(col_a[c] / LRSYS_TILE) * nt + col_b[c] / LRSYS_TILE] = 1;
    }
    for (int ta = 0; ta < nt; ta++)
        for (int tb = ta; tb < nt; tb++)
            if (used[(size_t)ta * nt + tb]) { tiles.push_back(ta); tiles.push_back(tb); }
    const size_t ntiles = tiles.size() / 2;
    int tp, dp, dq;
    lrsys_panels(rmax, ndu, ndw, &tp, &dp, &dq);
    const size_t lds = (size_t)LRSYS_TILE * (lrsys_stride(tp * dp) + lrsys_stride(tp * dq)) * sizeof(double);
    const size_t bound = modp_chunk_bound(g_cfg_lrsys_chunk_bytes, LRSYS_CHUNK_BYTES);
    const int rc = (int)std::min<size_t>((size_t)R, std::max<size_t>(bound / ((size_t)ns * nc * sizeof(long long)), 1));        // rows per chunk
    if ((size_t)rc * ntiles >= (size_t)lim) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: a chunk of rows needs 2^31 workgroups or more");

    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    int32_t *d_U = nullptr, *d_W = nullptr, *d_C = nullptr, *d_rowptr = nullptr, *d_map = nullptr, *d_canon = nullptr, *d_tiles = nullptr;
    long long *d_S = nullptr;
    int *d_cnt = nullptr;                                                                  // [0] impossibilities, [1] entries that do not fit
    MODPCHECK(bufs.get(&d_U, (size_t)nu)); MODPCHECK(bufs.get(&d_W, (size_t)nw)); MODPCHECK(bufs.get(&d_C, (size_t)nout));
    MODPCHECK(bufs.get(&d_rowptr, (size_t)R + 1)); MODPCHECK(bufs.get(&d_map, map.size())); MODPCHECK(bufs.get(&d_canon, canon.size()));
    MODPCHECK(bufs.get(&d_tiles, tiles.size())); MODPCHECK(bufs.get(&d_S, (size_t)ns * rc * nc)); MODPCHECK(bufs.get(&d_cnt, (size_t)2));
    ModpEvents ev(5);
    for (hipEvent_t &x : ev.e) MODPCHECK(hipEventCreate(&x));
    MODPCHECK(hipEventRecord(ev.e[3], nullptr));
    MODPCHECK(hipMemcpy(d_U, U, (size_t)nu * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_W, W, (size_t)nw * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_rowptr, rowptr, ((size_t)R + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_canon, canon.data(), canon.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_cnt, 0, 2 * sizeof(int)));
    double ms[2] = {0.0, 0.0};
    long long launched = 0;
    int chunks = 0;
    for (int i0 = 0; i0 < R; i0 += rc) {
        const int rows = std::min(rc, R - i0);
        MODPCHECK(hipMemsetAsync(d_S, 0, (size_t)ns * rows * nc * sizeof(long long), nullptr));
        MODPCHECK(hipEventRecord(ev.e[0], nullptr));
        hipLaunchKernelGGL(k_lrsys_tile, dim3((unsigned)((size_t)rows * ntiles)), dim3(ZZ_NT), lds, nullptr, n, T, d_rowptr, i0, rows, ndu, d_U, ndw, d_W, d_tiles,
                           (int)ntiles, d_map, nc, d_S, tp, dp, dq, d_cnt);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(k_lrsys_carry, dim3((unsigned)(((size_t)rows * nc + ZZ_NT - 1) / ZZ_NT)), dim3(ZZ_NT), 0, nullptr, d_S, ns, rows, nc, d_canon, i0, R, d_C,
                           ndc, d_cnt + 1);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipEventRecord(ev.e[2], nullptr));
        MODPCHECK(hipEventSynchronize(ev.e[2]));
        float a = 0.f, b = 0.f;
        MODPCHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); MODPCHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        ms[0] += a; ms[1] += b;
        launched += (long long)((size_t)rows * ntiles);
        chunks++;
    }
    int cnt[2] = {0, 0};
    std::vector<int32_t> h_C((size_t)nout);                                                // the caller's array is written only by a call that succeeds
    MODPCHECK(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy(h_C.data(), d_C, (size_t)nout * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipEventRecord(ev.e[4], nullptr));
    MODPCHECK(hipEventSynchronize(ev.e[4]));
    float whole = 0.f;
    MODPCHECK(hipEventElapsedTime(&whole, ev.e[3], ev.e[4]));
    g_lrsys_ms[0] = ms[0]; g_lrsys_ms[1] = ms[1]; g_lrsys_ms[2] = whole;
    info[0] = cnt[1]; info[1] = chunks; info[2] = (int32_t)std::min<long long>(launched, 0x7fffffffll); info[3] = cnt[0];
    if (cnt[0] != 0) return modp_fail(CLRS_ERR_HIP, "zz_lowrank_system: " + std::to_string(cnt[0]) + " accumulators that are no integers below 2^53");
    if (cnt[1] != 0) return modp_fail(CLRS_ERR_INVALID, "zz_lowrank_system: " + std::to_string(cnt[1]) + " entries of the system do not fit in ndc digits");
    std::copy(h_C.begin(), h_C.end(), C);
    return 0;
}

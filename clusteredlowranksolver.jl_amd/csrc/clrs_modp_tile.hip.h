// clrs_modp_tile.hip.h -- the main loop of the exact fp64 MFMA products of this unit, one text for k_zz_gemm (clrs_modp_zz_gemm.hip.h) and
// k_liftm_x (clrs_modp_liftm.hip.h; section 19).  Included by clrs_modp.hip before both, whose modp_v4d it uses.
//
// A workgroup of four waves takes a 64 x 64 tile of P = A B, a wave 32 x 32 of it as 2 x 2 tiles of 16 x 16 on v_mfma_f64_16x16x4 (the builtin and the operand /
// accumulator layout of k_modp_update).  The operand panels of a step of k-extent 16 (64 x 16 of A, 16 x 64 of B) are staged in LDS; the next step's panels are
// already in flight in registers.  After every PERIOD steps the caller's `every(acc)` runs on the accumulators: what keeps them below 2^53 (a flush into a second
// accumulator, a reduction mod p) is the caller's, and so are the bound on PERIOD and the epilogue.  One code path: rows >= M, columns >= N and k >= K load zeros.
//
// LDS layout against the bank rule (64 banks of 4 bytes for ds_read_b64, conflicts counted within a half of 32 lanes): the A-side operand of lane l is
// As[row (l & 15)][4 kk + (l >> 4)] with row stride ZZ_LDA = 18 doubles: within a half the double index is 18 (l & 15) + (l >> 4) + const, and 18 r mod 32 takes
// the 16 even values once each, so the 32 lanes fall on 32 different pairs of banks; lanes l and l + 16 are neighbours.  The B-side operand is
// Bs[4 kk + (l >> 4)][col (l & 15)] with row stride ZZ_LDB = 80 = 16 mod 32: lanes l + 16 read 16 doubles further on, again 32 different pairs of banks.
#pragma once

#define ZZ_BM 64                      // tile of P per workgroup
#define ZZ_BN 64
#define ZZ_BK 16                      // k-extent of a step: four MFMAs per accumulator
#define ZZ_LDA (ZZ_BK + 2)            // row stride of the A panel in LDS (doubles)
#define ZZ_LDB (ZZ_BN + 16)           // row stride of the B panel in LDS (doubles)

// acc = sum_kk A[r, kk] B[kk, c0 + c] over the tile at (row0, col0), for a workgroup of 256 threads: A is M x K (row stride K), B has row stride ldb, r < M and
// c < N.  Lane l of the wave at (wr, wc) = (32 (wave >> 1), 32 (wave & 1)) holds in acc[ti][tj][reg] row row0 + wr + 16 ti + (l >> 4) + 4 reg, column
// col0 + wc + 16 tj + (l & 15).  `every` is not called after the last step unless PERIOD divides the number of steps: the caller's epilogue does it once more.
// ldb and c0 keep the caller's integer type Ld (size_t in k_zz_gemm, int in k_liftm_x) and are widened where they are used, as each kernel's own loop did:
// widened once at the call, k_liftm_x compiled to other code around the loop and ran 1 % slower at n = 1024 (profiles/rounding/tile_loop_times.json).
template <int PERIOD, class Ld, class Every>
__device__ __forceinline__ void zz_tile_loop(const double *__restrict__ A, int M, int K, const double *__restrict__ B, Ld ldb, Ld c0, int N, int row0,
                                             int col0, modp_v4d (&acc)[2][2], Every every) {
    __shared__ double As[ZZ_BM * ZZ_LDA], Bs[ZZ_BK * ZZ_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    // the loads of a step: A panel row a_r + 16 i, column a_k; B panel row b_k + 4 i, column b_c
    const int a_r = tid >> 4, a_k = tid & 15, b_k = tid >> 6, b_c = tid & 63;
    double ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = row0 + a_r + 16 * i, ka = k0 + a_k, kb = k0 + b_k + 4 * i, c = col0 + b_c;
            ra[i] = (r < M && ka < K) ? A[(size_t)r * K + ka] : 0.0;
            rb[i] = (kb < K && c < N) ? B[(size_t)kb * ldb + c0 + c] : 0.0;
        }
    };
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) acc[ti][tj][reg] = 0.0;
    const int nsteps = (K + ZZ_BK - 1) / ZZ_BK;
    fetch(0);
    for (int step = 0; step < nsteps; step++) {
        __syncthreads();                                                                   // the panels of the step before are read
#pragma unroll
        for (int i = 0; i < 4; i++) {
            As[(a_r + 16 * i) * ZZ_LDA + a_k] = ra[i];
            Bs[(b_k + 4 * i) * ZZ_LDB + b_c] = rb[i];
        }
        __syncthreads();
        if (step + 1 < nsteps) fetch((step + 1) * ZZ_BK);                                  // (uniform) in flight while this step multiplies
#pragma unroll
        for (int kk = 0; kk < ZZ_BK / 4; kk++) {
            // operands: A-side lane l holds A[row (l & 15), 4 kk + (l >> 4)], B-side lane l holds B[4 kk + (l >> 4), column (l & 15)]
            double av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                av[t] = As[(wr + 16 * t + l15) * ZZ_LDA + 4 * kk + l4];
                bv[t] = Bs[(4 * kk + l4) * ZZ_LDB + wc + 16 * t + l15];
            }
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
        }
        if ((step + 1) % PERIOD == 0) every(acc);                                          // (uniform)
    }
}

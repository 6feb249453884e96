// clrs_modp_lift.hip.h -- the exact solution of an integer system A x = b by Dixon's p-adic lifting (clrs_modp_dixon_lift, include/clrs_hip.h; DESIGN.md
// section 15): what the reference's project_to_affine_space asks of Nemo._solve_dixon (src/rounding.jl:274, 351, 360), on the device.  Included at the end of
// clrs_modp.hip, whose elimination (modp_eliminate) and buffers (ModpBufs) it uses.
//
//   C = A^-1 mod p      lift_inverse_modp (shared with clrs_modp_liftm.hip.h): k_lift_residues builds [A mod p | I] (n x 2n fp64 residues) from the digit
//                       planes of A, modp_eliminate reduces it with the pivots sought in the first n columns; then k_lift_gather writes the right half in
//                       pivot-row order as int32.  rank < n: the call ends here.
//   r_0 = b, and per step k:   x_k = C (r_k mod p) mod p             k_lift_x
//                              r_{k+1} = (r_k - A x_k) / p, exactly   k_lift_r   (which also leaves r_{k+1} mod p for the next k_lift_x)
//
// Integers are balanced base-2^24 digits (clrs_modp_lift_arith.h).  Device layout: every row of C and of the digit planes of A is padded with zeros to
// `ld` = n rounded up to a multiple of 4 ints, x and rbar likewise, so that the lanes read 16 bytes at a time with no tail.  r is (nrl + 1) x ld: its limbs
// and one working limb on top for r_k - A x_k before the division.
//
// Both lifting kernels: one wave per row, four waves per workgroup, the lanes stride the columns, int32 x int32 + int64 (v_mad_i64_i32), a wave reduction of
// the int64 sums, then lane 0 does what is left of the row.  A digit times a residue is below 2^46 and n <= 32767, so every row sum is below 2^61: exact in
// any order.  x and rbar (n ints, at most 128 KiB) are read through the cache by every wave beside its row of (1 + nd) n ints.  No barrier, no LDS.
// The two kernels of a step follow each other on one stream, 2 * steps launches back to back, no host synchronisation in between.
#pragma once
#include "clrs_modp_lift_arith.h"

#define LIFT_NT 256                   // four waves per workgroup
#define LIFT_ROWS (LIFT_NT / 64)      // one row per wave
#define LIFT_MAX_N 32767              // [A | I] stays below 2^31 entries and a row sum below 2^61

__device__ inline long long lift_wave_sum(long long s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// M (n x 2n fp64): [A mod p | I]; A mod p = sum_j a_j (2^(24 j) mod p) mod p, non-negative.  |a_j pw[j]| < 2^46, reduced as it is added.
__global__ __launch_bounds__(LIFT_NT) void k_lift_residues(const int32_t *__restrict__ Ad, int n, int ld, int nd, int p, const int32_t *__restrict__ pw,
                                                           double *__restrict__ M) {
    const size_t count = (size_t)n * n, plane = (size_t)n * ld;
    for (size_t o = (size_t)blockIdx.x * LIFT_NT + threadIdx.x; o < count; o += (size_t)gridDim.x * LIFT_NT) {
        const size_t i = o / n, c = o - i * n;
        long long acc = 0;
        for (int j = 0; j < nd; j++) acc = (acc + (long long)Ad[(size_t)j * plane + i * ld + c] * (long long)pw[j]) % (long long)p;
        if (acc < 0) acc += p;
        M[i * 2 * n + c] = (double)acc;
        M[i * 2 * n + n + c] = i == c ? 1.0 : 0.0;
    }
}

// C[j, c] = M[pivot row j, n + c] as T (int32 for k_lift_x, fp64 for k_liftm_x), n x ld, the padding columns zero
template <class T>
__global__ __launch_bounds__(LIFT_NT) void k_lift_gather(const double *__restrict__ M, int n, int ld, const int *__restrict__ order, T *__restrict__ Cinv) {
    const size_t count = (size_t)n * ld;
    for (size_t o = (size_t)blockIdx.x * LIFT_NT + threadIdx.x; o < count; o += (size_t)gridDim.x * LIFT_NT) {
        const size_t j = o / ld, c = o - j * ld;
        Cinv[o] = c < (size_t)n ? (T)M[(size_t)order[j] * 2 * n + n + c] : (T)0;
    }
}

// x[i] = sum_c C[i, c] rbar[c] mod p, also into Xk (row k of X).  Both factors lie in [0, p): the sum is non-negative and below n 2^46.
__global__ __launch_bounds__(LIFT_NT) void k_lift_x(const int32_t *__restrict__ Cinv, const int32_t *__restrict__ rbar, int n, int ld, int p, int32_t *__restrict__ x,
                                                    int32_t *__restrict__ Xk) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * LIFT_ROWS + (threadIdx.x >> 6);
    if (i >= n) return;                                                                   // (wave-uniform)
    const int4 *row = (const int4 *)(Cinv + (size_t)i * ld), *vec = (const int4 *)rbar;
    long long s = 0;
    for (int c = lane; c < ld / 4; c += 64) {
        const int4 a = row[c], v = vec[c];
        s += (long long)a.x * v.x + (long long)a.y * v.y + (long long)a.z * v.z + (long long)a.w * v.w;
    }
    s = lift_wave_sum(s);
    if (lane == 0) {
        const int32_t xi = (int32_t)((unsigned long long)s % (unsigned long long)p);
        x[i] = xi;
        Xk[i] = xi;
    }
}

// Row i of r <- (r - A x) / p.  Limb by limb from the bottom, the wave forms s_l = sum_c a_l[i, c] x[c] (l < nd) and lane 0 takes r_l - s_l plus the carry
// into a balanced digit, through the working limb on top; then lane 0 divides by p from the top limb, brings the quotient back to balanced digits and leaves
// rbar[i] = r_i mod p.  cnt[0] counts divisions that left a remainder, cnt[1] rows whose result does not fit in nrl limbs: both must stay 0.
__global__ __launch_bounds__(LIFT_NT) void k_lift_r(const int32_t *__restrict__ Ad, const int32_t *__restrict__ x, int n, int ld, int nd, int nrl, int p,
                                                    const int32_t *__restrict__ pw, int32_t *__restrict__ r, int32_t *__restrict__ rbar, int *__restrict__ cnt) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * LIFT_ROWS + (threadIdx.x >> 6);
    if (i >= n) return;                                                                   // (wave-uniform)
    const int4 *vec = (const int4 *)x;
    const size_t plane = (size_t)n * ld;
    const int nt = nrl + 1;
    long long carry = 0;
    for (int l = 0; l < nt; l++) {
        long long s = 0;
        if (l < nd) {
            const int4 *row = (const int4 *)(Ad + (size_t)l * plane + (size_t)i * ld);
            for (int c = lane; c < ld / 4; c += 64) {
                const int4 a = row[c], v = vec[c];
                s += (long long)a.x * v.x + (long long)a.y * v.y + (long long)a.z * v.z + (long long)a.w * v.w;
            }
            s = lift_wave_sum(s);
        }
        if (lane == 0) {
            int32_t d;
            carry = lift_carry(carry + (l < nrl ? (long long)r[(size_t)l * ld + i] : 0ll) - s, &d);
            r[(size_t)l * ld + i] = d;
        }
    }
    if (lane == 0) {
        int flags;
        rbar[i] = lift_finish_row(r + i, (size_t)ld, nrl, p, pw, carry, &flags);
        if (flags & 1) atomicAdd(cnt, 1);
        if (flags & 2) atomicAdd(cnt + 1, 1);
    }
}

// The refusals clrs_modp_dixon_lift and clrs_modp_dixon_lift_multi (`who`; m = its columns, 1 for the former) share, in the order both make them
static int lift_check_sizes(const std::string &who, int n, int m, int nd, int nbl, int steps, int p) {
    if (n < 0 || n > LIFT_MAX_N) return modp_fail(CLRS_ERR_INVALID, who + ": n must lie in [0, 32767]");
    if (m < 0) return modp_fail(CLRS_ERR_INVALID, who + ": m must not be negative");
    if (nd < 1 || nbl < 1 || steps < 0) return modp_fail(CLRS_ERR_INVALID, who + ": nd and nbl must be at least 1 and steps at least 0");
    if (nd > LIFT_MAX_N || nbl > LIFT_MAX_N) return modp_fail(CLRS_ERR_INVALID, who + ": more than 32767 limbs");
    if (!modp_prime_ok(p)) return modp_fail(CLRS_ERR_INVALID, who + ": p must be a prime with 2 <= p < 2^23");
    return 0;
}

// `what` ("a digit of A", "a limb of b") outside [-2^23, 2^23) among the `count` of v
static int lift_check_digits(const std::string &who, const char *what, const int32_t *v, size_t count) {
    for (size_t o = 0; o < count; o++)
        if (v[o] < -LIFT_HALF || v[o] >= LIFT_HALF) return modp_fail(CLRS_ERR_INVALID, who + ": " + what + " outside [-2^23, 2^23)");
    return 0;
}

// The inverse mod p, from the digit planes of A on the device (d_Ad: nd planes of n rows of `ld` ints; d_pw[j] = 2^(24 j) mod p): *d_M (n x 2n fp64, from
// `bufs`) becomes [A mod p | I] and is left reduced with the pivots sought in the first n columns; *rank is the rank of A mod p.  rank == n: *d_order[j] is the
// row of M that is pivot row j, so the right half of M in that order is A^-1 mod p (work may still be in flight).  rank < n: the stream is synchronised and
// there is no *d_order; the caller ends its call.
static int lift_inverse_modp(const int32_t *d_Ad, int n, int ld, int nd, int p, const int32_t *d_pw, ModpBufs &bufs, double **d_M, int **d_order, int *rank) {
    int *d_flag = nullptr;
    MODPCHECK(bufs.get(d_M, 2 * (size_t)n * n));
    hipLaunchKernelGGL(k_lift_residues, modp_flat_grid((size_t)n * n, LIFT_NT), dim3(LIFT_NT), 0, nullptr, d_Ad, n, ld, nd, p, d_pw, *d_M);
    MODPCHECK(hipGetLastError());
    std::vector<int32_t> found;
    const int code = modp_eliminate(*d_M, n, 2 * n, n, p, bufs, &d_flag, found);
    if (code != 0) return code;
    *rank = (int)found.size();
    if (*rank < n) {                                           // singular mod p: no error, the caller takes another prime
        MODPCHECK(hipStreamSynchronize(nullptr));
        return 0;
    }
    MODPCHECK(bufs.get(d_order, (size_t)n));
    hipLaunchKernelGGL(k_modp_order, dim3((unsigned)((n + MODP_NT - 1) / MODP_NT)), dim3(MODP_NT), 0, nullptr, d_flag, n, *d_order);
    MODPCHECK(hipGetLastError());
    return 0;
}

extern "C" int clrs_modp_dixon_lift(int device, int n, int p, int nd, const int32_t *A_digits, int nbl, const int32_t *b_limbs, int steps, int32_t *X,
                                    int32_t *r_limbs, int32_t *info) {
    const char *who = "modp_dixon_lift";
    if (int code = lift_check_sizes(who, n, 1, nd, nbl, steps, p)) return code;
    if (n == 0) {
        if (info) { info[0] = 0; info[1] = steps; info[2] = 0; info[3] = 0; }
        return 0;
    }
    if (!A_digits || !b_limbs || !r_limbs || !info || (!X && steps > 0)) return modp_fail(CLRS_ERR_INVALID, "modp_dixon_lift: null argument");
    if (int code = lift_check_digits(who, "a digit of A", A_digits, (size_t)nd * n * n)) return code;
    if (int code = lift_check_digits(who, "a limb of b", b_limbs, (size_t)nbl * n)) return code;
    const int nrl = std::max(nbl, nd + 1) + 1, nt = nrl + 1, ld = (n + 3) & ~3;
    std::vector<int32_t> pw((size_t)std::max(nd, nt));
    lift_power_table(p, (int)pw.size(), pw.data());

    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    int32_t *d_Ad = nullptr, *d_pw = nullptr, *d_C = nullptr, *d_x = nullptr, *d_rbar = nullptr, *d_r = nullptr, *d_X = nullptr;
    double *d_M = nullptr;
    int *d_order = nullptr, *d_cnt = nullptr;
    const size_t plane = (size_t)n * ld;
    MODPCHECK(bufs.get(&d_Ad, (size_t)nd * plane)); MODPCHECK(bufs.get(&d_pw, pw.size()));
    MODPCHECK(hipMemset(d_Ad, 0, (size_t)nd * plane * sizeof(int32_t)));
    MODPCHECK(hipMemcpy2D(d_Ad, (size_t)ld * sizeof(int32_t), A_digits, (size_t)n * sizeof(int32_t), (size_t)n * sizeof(int32_t), (size_t)nd * n, hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_pw, pw.data(), pw.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    int rank = 0;
    if (int code = lift_inverse_modp(d_Ad, n, ld, nd, p, d_pw, bufs, &d_M, &d_order, &rank)) return code;
    if (rank < n) {
        info[0] = rank; info[1] = 0; info[2] = 0; info[3] = 0;
        return 0;
    }
    MODPCHECK(bufs.get(&d_C, plane));
    hipLaunchKernelGGL(k_lift_gather<int32_t>, modp_flat_grid(plane, LIFT_NT), dim3(LIFT_NT), 0, nullptr, d_M, n, ld, d_order, d_C);
    MODPCHECK(hipGetLastError());
    MODPCHECK(bufs.drop(d_M));                                 // 16 n^2 bytes the lifting does not need (hipFree waits for the gather)
    d_M = nullptr;

    // r_0 = b and its residues, padded
    std::vector<int32_t> r0((size_t)nt * ld, 0), rbar0((size_t)ld, 0);
    for (int l = 0; l < nbl; l++)
        for (int i = 0; i < n; i++) r0[(size_t)l * ld + i] = b_limbs[(size_t)l * n + i];
    for (int i = 0; i < n; i++) rbar0[i] = lift_residue(r0.data() + i, (size_t)ld, nrl, pw.data(), p);
    MODPCHECK(bufs.get(&d_r, r0.size())); MODPCHECK(bufs.get(&d_rbar, (size_t)ld)); MODPCHECK(bufs.get(&d_x, (size_t)ld));
    MODPCHECK(bufs.get(&d_X, (size_t)steps * n)); MODPCHECK(bufs.get(&d_cnt, (size_t)2));
    MODPCHECK(hipMemcpy(d_r, r0.data(), r0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemcpy(d_rbar, rbar0.data(), rbar0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MODPCHECK(hipMemset(d_x, 0, (size_t)ld * sizeof(int32_t)));
    MODPCHECK(hipMemset(d_cnt, 0, 2 * sizeof(int)));
    const dim3 rows((unsigned)((n + LIFT_ROWS - 1) / LIFT_ROWS));
    for (int k = 0; k < steps; k++) {
        hipLaunchKernelGGL(k_lift_x, rows, dim3(LIFT_NT), 0, nullptr, d_C, d_rbar, n, ld, p, d_x, d_X + (size_t)k * n);
        hipLaunchKernelGGL(k_lift_r, rows, dim3(LIFT_NT), 0, nullptr, d_Ad, d_x, n, ld, nd, nrl, p, d_pw, d_r, d_rbar, d_cnt);
        MODPCHECK(hipGetLastError());                          // (host side only: a refused launch ends the loop at its step)
    }
    MODPCHECK(hipStreamSynchronize(nullptr));
    int cnt[2] = {0, 0};
    MODPCHECK(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    if (steps > 0) MODPCHECK(hipMemcpy(X, d_X, (size_t)steps * n * sizeof(int32_t), hipMemcpyDeviceToHost));
    MODPCHECK(hipMemcpy2D(r_limbs, (size_t)n * sizeof(int32_t), d_r, (size_t)ld * sizeof(int32_t), (size_t)n * sizeof(int32_t), (size_t)nrl, hipMemcpyDeviceToHost));
    info[0] = rank; info[1] = steps; info[2] = cnt[0]; info[3] = cnt[1];
    if (cnt[0] != 0 || cnt[1] != 0)
        return modp_fail(CLRS_ERR_HIP, "modp_dixon_lift: " + std::to_string(cnt[0]) + " divisions by p left a remainder and " + std::to_string(cnt[1]) +
                                           " residuals left their limbs: the lifting is not exact");
    return 0;
}

// clrs_modp.hip -- reduced row-echelon form of an integer matrix over the field of integers mod a prime p < 2^23 (clrs_modp_rref, include/clrs_hip.h;
// DESIGN.md section 14): what the reference's find_pivots_modular (src/rounding.jl:313-333) asks of Nemo.rref, on the device.  No context, host pointers.
//
// The residues live in HBM as fp64 (exact integers in [0, p)), row-major, and the rows never move: `flag[i]` is -1 or the position of row i among the pivot
// rows.  A blocked right-looking Gauss-Jordan elimination, MODP_W columns per panel:
//
//   k_modp_panel   one workgroup.  Copies the panel to a workspace P (global memory: the panel is NOT limited to LDS), walks its columns in order -- the
//                  lowest-indexed row that is no pivot row yet and is non-zero there becomes the pivot row, the column is cleared from every other row of P
//                  -- and leaves: the k <= MODP_W pivots, G = the inverse of the k x k block (pivot rows x pivot columns) of the panel as it stood BEFORE the
//                  step, and the multipliers Mn (nrows x MODP_W): Mn[i, t] = -A[i, pivot column t] (before the step) for the rows that are no new pivot
//                  rows, the unit vector e_s for the new pivot row s.  P, now final, goes back into A.
//   k_modp_pivot_rows   U = G A[new pivot rows, trailing columns] (k x ntrail, rows k .. MODP_W - 1 zero): one thread per column.
//   k_modp_update  A[i, c] <- (keep_i A[i, c] + sum_t Mn[i, t] U[t, c]) mod p over the trailing columns, keep_i = 0 for the new pivot rows (they become
//                  their row of U) and 1 for every other row, earlier pivot rows included: one 16 x 16 tile per wave, four v_mfma_f64_16x16x4, ONE
//                  reduction per entry.  16 products of residues plus one residue stay below 2^53 (clrs_modp_arith.h), so the sum is exact in any order.
//   k_modp_gather  R[j, :] = A[pivot row j, :] as int32, rows >= rank zero.
//
// The host reads k and the pivot columns after each panel and stops when the columns are exhausted or rank == nrows (the trailing columns are then final).
// The panel loop is modp_eliminate, on a matrix already on the device; clrs_modp_rref is its caller, and so is clrs_modp_dixon_lift (clrs_modp_lift.hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_modp_arith.h"

extern "C" void clrs_set_last_error(const char *msg);   // clrs_hip.hip: the library keeps one thread-local message

#define MODP_W 16             // panel width = k-extent of the trailing update
#define MODP_PANEL_NT 1024    // threads of the one workgroup of k_modp_panel
#define MODP_NT 256

typedef double modp_v4d __attribute__((ext_vector_type(4)));

static int modp_fail(int code, const std::string &msg) {
    clrs_set_last_error(msg.c_str());
    return code;
}
#define MODPCHECK(expr)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return modp_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// int32 residues -> fp64
__global__ __launch_bounds__(MODP_NT) void k_modp_widen(const int32_t *__restrict__ src, double *__restrict__ dst, size_t count) {
    for (size_t o = (size_t)blockIdx.x * MODP_NT + threadIdx.x; o < count; o += (size_t)gridDim.x * MODP_NT) dst[o] = (double)src[o];
}

// info: [0] = k, [1 + t] = pivot column t (relative to c0), [1 + MODP_W + t] = pivot row t; flag[i]: -1 or the position of row i among the pivot rows
__global__ __launch_bounds__(MODP_PANEL_NT) void k_modp_panel(double *__restrict__ A, int nrows, int ncols, int c0, int w, int rank0, int p_int, double *__restrict__ P,
                                                              int *__restrict__ flag, double *__restrict__ Mn, double *__restrict__ G, int *__restrict__ info) {
    __shared__ int s_row;
    __shared__ int s_k;
    __shared__ int s_pcol[MODP_W], s_prow[MODP_W];
    __shared__ double s_piv[MODP_W];
    __shared__ double s_B[MODP_W][2 * MODP_W + 1];
    __shared__ double s_inv;
    const int tid = threadIdx.x, lane16 = tid & 15, sub = tid >> 4;          // sub: one of 64 row slots, lane16: the column within the panel
    const double p = (double)p_int, pinv = 1.0 / p;
    constexpr int SLOTS = MODP_PANEL_NT / 16;
    if (tid == 0) s_k = 0;
    // the panel as it stands, columns >= w zero
    for (long long r = sub; r < nrows; r += SLOTS) P[(size_t)r * MODP_W + lane16] = lane16 < w ? A[(size_t)r * ncols + c0 + lane16] : 0.0;
    __syncthreads();
    for (int j = 0; j < w; j++) {
        if (tid == 0) s_row = nrows;
        __syncthreads();
        int best = nrows;
        for (long long r = tid; r < nrows; r += MODP_PANEL_NT)                             // (64-bit: nrows may be within a trip of 2^31)
            if (flag[r] < 0 && P[(size_t)r * MODP_W + j] != 0.0) { best = (int)r; break; }         // ascending: the first hit is this thread's lowest
        if (best < nrows) atomicMin(&s_row, best);
        __syncthreads();
        const int prow = s_row;
        if (prow == nrows) {                                                                 // (uniform) no pivot in this column
            __syncthreads();                                                                 // s_row is written again at the top
            continue;
        }
        const int k = s_k;
        if (tid == 0) s_inv = modp_inv(P[(size_t)prow * MODP_W + j], p_int);
        __syncthreads();
        if (tid < MODP_W) {
            const double v = modp_mul(P[(size_t)prow * MODP_W + tid], s_inv, p, pinv);
            s_piv[tid] = v;
            P[(size_t)prow * MODP_W + tid] = v;
        }
        if (tid == 0) {
            s_pcol[k] = j;
            s_prow[k] = prow;
            flag[prow] = rank0 + k;
            s_k = k + 1;
        }
        __syncthreads();
        // clear column j from every other row: 16 lanes per row, the factor from the lane that holds column j (rows are whole within a wave)
        // (four rows per lane and trip, so that their loads are in flight together)
        const double pv = s_piv[lane16];
        for (long long r0 = 0; r0 < nrows; r0 += 4 * SLOTS) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const long long r = r0 + u * SLOTS + sub;
                v[u] = r < nrows ? P[(size_t)r * MODP_W + lane16] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const long long r = r0 + u * SLOTS + sub;
                const double f = __shfl(v[u], j, 16);
                if (r < nrows && r != prow && f != 0.0) P[(size_t)r * MODP_W + lane16] = modp_reduce(v[u] + (p - f) * pv, p, pinv);
            }
        }
        __syncthreads();
    }
    const int k = s_k;
    // the multipliers, from A (still as it stood before the step), and the k x k block with the identity beside it
    for (long long r = sub; r < nrows; r += SLOTS) {
        const int f = flag[r];
        double m = 0.0;
        if (lane16 < k) m = f >= rank0 ? (f - rank0 == lane16 ? 1.0 : 0.0) : modp_neg(A[(size_t)r * ncols + c0 + s_pcol[lane16]], p);
        Mn[(size_t)r * MODP_W + lane16] = m;
    }
    if (tid < MODP_W * MODP_W) {
        const int s = tid >> 4, t = tid & 15;
        s_B[s][t] = s < k && t < k ? A[(size_t)s_prow[s] * ncols + c0 + s_pcol[t]] : (s == t ? 1.0 : 0.0);
        s_B[s][MODP_W + t] = s == t ? 1.0 : 0.0;
    }
    __syncthreads();
    // G = B^-1 by Gauss-Jordan without exchanges: the pivot rows were found in this order, so every leading block of B is invertible
    for (int s = 0; s < k; s++) {
        if (tid == 0) s_inv = modp_inv(s_B[s][s], p_int);
        __syncthreads();
        if (tid < 2 * MODP_W) s_B[s][tid] = modp_mul(s_B[s][tid], s_inv, p, pinv);
        __syncthreads();
        double f = 0.0, v0 = 0.0, v1 = 0.0;
        const int r = tid >> 4, t = tid & 15;
        if (tid < MODP_W * MODP_W && r != s) {
            f = s_B[r][s];
            v0 = s_B[r][t];
            v1 = s_B[r][MODP_W + t];
        }
        __syncthreads();
        if (tid < MODP_W * MODP_W && r != s && f != 0.0) {
            s_B[r][t] = modp_reduce(v0 + (p - f) * s_B[s][t], p, pinv);
            s_B[r][MODP_W + t] = modp_reduce(v1 + (p - f) * s_B[s][MODP_W + t], p, pinv);
        }
        __syncthreads();
    }
    if (tid < MODP_W * MODP_W) {
        const int s = tid >> 4, t = tid & 15;
        G[s * MODP_W + t] = s < k && t < k ? s_B[s][MODP_W + t] : 0.0;
    }
    // the panel is final
    for (long long r = sub; r < nrows; r += SLOTS)
        if (lane16 < w) A[(size_t)r * ncols + c0 + lane16] = P[(size_t)r * MODP_W + lane16];
    if (tid == 0) info[0] = k;
    if (tid < MODP_W) {
        info[1 + tid] = tid < k ? s_pcol[tid] : -1;
        info[1 + MODP_W + tid] = tid < k ? s_prow[tid] : -1;
    }
}

// U[s, c] = sum_t G[s, t] A[prow[t], c] mod p for the trailing columns c >= c1; U is MODP_W x ncols (rows >= k zero)
__global__ __launch_bounds__(MODP_NT) void k_modp_pivot_rows(const double *__restrict__ A, int ncols, int c1, int k, int p_int, const double *__restrict__ G,
                                                             const int *__restrict__ info, double *__restrict__ U) {
    __shared__ double s_G[MODP_W * MODP_W];
    __shared__ int s_prow[MODP_W];
    if (threadIdx.x < MODP_W * MODP_W) s_G[threadIdx.x] = G[threadIdx.x];
    if (threadIdx.x < MODP_W) s_prow[threadIdx.x] = info[1 + MODP_W + threadIdx.x];
    __syncthreads();
    const int c = c1 + blockIdx.x * MODP_NT + threadIdx.x;
    if (c >= ncols) return;
    const double p = (double)p_int, pinv = 1.0 / p;
    double a[MODP_W];
#pragma unroll
    for (int t = 0; t < MODP_W; t++) a[t] = t < k ? A[(size_t)s_prow[t] * ncols + c] : 0.0;
#pragma unroll
    for (int s = 0; s < MODP_W; s++) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < MODP_W; t++) acc = fma(s_G[s * MODP_W + t], a[t], acc);              // exact: 16 products below 2^46
        U[(size_t)s * ncols + c] = modp_reduce(acc, p, pinv);
    }
}

// one 16 x 16 tile of the trailing matrix per wave (four tiles side by side per workgroup); rows of tile blockIdx.y, columns from c1
// (a flat grid: either extent of the matrix may exceed what gridDim.y holds), `colblocks` workgroups per row of tiles.  Launched only where columns
// trail a panel, ncols > MODP_W, so nrows < 2^27 and the row arithmetic stays far inside int
__global__ __launch_bounds__(MODP_NT) void k_modp_update(double *__restrict__ A, int nrows, int ncols, int c1, int rank0, int p_int, int colblocks,
                                                         const int *__restrict__ flag, const double *__restrict__ Mn, const double *__restrict__ U) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int by = blockIdx.x / colblocks, bx = blockIdx.x - by * colblocks;
    const int row0 = by * 16, col0 = c1 + (bx * (MODP_NT / 64) + wave) * 16;
    if (col0 >= ncols) return;                                                            // (wave-uniform)
    const double p = (double)p_int, pinv = 1.0 / p;
    // operands: A-side lane l holds Mn[row0 + (l & 15), 4 kk + (l >> 4)], B-side lane l holds U[4 kk + (l >> 4), col0 + (l & 15)]
    const int ar = row0 + l15, bc = col0 + l15;
    double av[4], bv[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
        av[kk] = ar < nrows ? Mn[(size_t)ar * MODP_W + 4 * kk + l4] : 0.0;
        bv[kk] = bc < ncols ? U[(size_t)(4 * kk + l4) * ncols + bc] : 0.0;
    }
    // accumulator: column l & 15, row (l >> 4) + 4 reg
    modp_v4d acc;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = row0 + l4 + 4 * reg;
        acc[reg] = (r < nrows && bc < ncols && flag[r] < rank0) ? A[(size_t)r * ncols + bc] : 0.0;
    }
#pragma unroll
    for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bv[kk], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = row0 + l4 + 4 * reg;
        if (r < nrows && bc < ncols) A[(size_t)r * ncols + bc] = modp_reduce(acc[reg], p, pinv);
    }
}

// order[i]: the row of A that is pivot row i (i < rank)
__global__ __launch_bounds__(MODP_NT) void k_modp_order(const int *__restrict__ flag, int nrows, int *__restrict__ order) {
    const long long r = (long long)blockIdx.x * MODP_NT + threadIdx.x;
    if (r < nrows && flag[r] >= 0) order[flag[r]] = (int)r;
}

__global__ __launch_bounds__(MODP_NT) void k_modp_gather(const double *__restrict__ A, int nrows, int ncols, int rank, const int *__restrict__ order,
                                                         int32_t *__restrict__ R) {
    const size_t count = (size_t)nrows * ncols;
    for (size_t o = (size_t)blockIdx.x * MODP_NT + threadIdx.x; o < count; o += (size_t)gridDim.x * MODP_NT) {
        const size_t i = o / ncols, c = o - i * ncols;
        R[o] = (int)i < rank ? (int32_t)A[(size_t)order[i] * ncols + c] : 0;
    }
}

namespace {
struct ModpBufs {                      // every device buffer of a call, released on every path
    std::vector<void *> p;
    ~ModpBufs() { for (void *x : p) (void)hipFree(x); }
    template <class T>
    hipError_t get(T **d, size_t count) {
        hipError_t e = hipMalloc((void **)d, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*d);
        return e;
    }
    hipError_t drop(void *d) {         // release one buffer early (hipFree waits for the work that uses it)
        p.erase(std::remove(p.begin(), p.end(), d), p.end());
        return hipFree(d);
    }
};
struct ModpEvents {                    // the device events of a call: `count` null slots for the caller's hipEventCreate, destroyed on every path
    std::vector<hipEvent_t> e;
    explicit ModpEvents(size_t count) : e(count, nullptr) {}
    ~ModpEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

// the grid of a kernel that strides `count` elements with workgroups of nt threads
static dim3 modp_flat_grid(size_t count, int nt) { return dim3((unsigned)std::min<size_t>((count + nt - 1) / nt, 65536)); }

static bool modp_prime_ok(int p) { return p >= 2 && p < (1 << MODP_MAX_PRIME_BITS) && modp_is_prime(p); }

// the byte bound of a chunk: what clrs_config_set gave (for the tests), else the default
static size_t modp_chunk_bound(int cfg, size_t dflt) { return cfg > 0 ? (size_t)cfg : dflt; }

// The elimination itself, on a matrix of fp64 residues already on the device (row-major, nrows x ncols), which it leaves there in reduced form: pivots are
// sought in the columns below `pcols` only (pcols = ncols: the reduced row-echelon form; pcols < ncols: the columns behind are carried along, as the
// identity beside A is for an inverse, clrs_modp_lift.hip.h).  `found` receives the pivot columns, ascending; *d_flag_out the device array of flag[i]
// (-1 or the position of row i among the pivot rows).  The workspaces come from `bufs`.  Synchronises once per panel; work may still be in flight on return.
static int modp_eliminate(double *d_A, int nrows, int ncols, int pcols, int p, ModpBufs &bufs, int **d_flag_out, std::vector<int32_t> &found) {
    double *d_P = nullptr, *d_Mn = nullptr, *d_G = nullptr, *d_U = nullptr;
    int *d_flag = nullptr, *d_info = nullptr;
    MODPCHECK(bufs.get(&d_P, (size_t)nrows * MODP_W)); MODPCHECK(bufs.get(&d_Mn, (size_t)nrows * MODP_W));
    MODPCHECK(bufs.get(&d_G, (size_t)MODP_W * MODP_W)); MODPCHECK(bufs.get(&d_U, (size_t)MODP_W * ncols));
    MODPCHECK(bufs.get(&d_flag, (size_t)nrows)); MODPCHECK(bufs.get(&d_info, (size_t)1 + 2 * MODP_W));
    MODPCHECK(hipMemset(d_flag, 0xff, (size_t)nrows * sizeof(int)));
    *d_flag_out = d_flag;
    int rk = 0, info[1 + 2 * MODP_W];
    for (int c0 = 0; c0 < pcols && rk < nrows; c0 += MODP_W) {
        const int w = std::min(MODP_W, pcols - c0), c1 = c0 + w;
        hipLaunchKernelGGL(k_modp_panel, dim3(1), dim3(MODP_PANEL_NT), 0, nullptr, d_A, nrows, ncols, c0, w, rk, p, d_P, d_flag, d_Mn, d_G, d_info);
        MODPCHECK(hipGetLastError());
        MODPCHECK(hipMemcpy(info, d_info, sizeof(info), hipMemcpyDeviceToHost));          // (synchronises: the pivot count decides what follows)
        const int k = info[0];
        if (k < 0 || k > w || rk + k > nrows) return modp_fail(CLRS_ERR_HIP, "modp_rref: the panel step returned an impossible pivot count");
        for (int t = 0; t < k; t++) found.push_back(c0 + info[1 + t]);
        if (k > 0 && c1 < ncols) {
            const int ntrail = ncols - c1;
            hipLaunchKernelGGL(k_modp_pivot_rows, dim3((ntrail + MODP_NT - 1) / MODP_NT), dim3(MODP_NT), 0, nullptr, d_A, ncols, c1, k, p, d_G, d_info, d_U);
            MODPCHECK(hipGetLastError());
            const int per_wg = 16 * (MODP_NT / 64);
            const int colblocks = (ntrail + per_wg - 1) / per_wg, rowtiles = (nrows + 15) / 16;      // (nrows < 2^27 here; rowtiles * colblocks < 2^27)
            hipLaunchKernelGGL(k_modp_update, dim3((unsigned)colblocks * (unsigned)rowtiles), dim3(MODP_NT), 0, nullptr, d_A, nrows, ncols, c1, rk, p, colblocks,
                               d_flag, d_Mn, d_U);
            MODPCHECK(hipGetLastError());
        }
        rk += k;
    }
    return 0;
}

extern "C" int clrs_modp_rref(int device, int nrows, int ncols, int p, const int32_t *A, int32_t *pivots, int32_t *rank, int32_t *R) {
    if (nrows < 0 || ncols < 0) return modp_fail(CLRS_ERR_INVALID, "modp_rref: negative size");
    if ((long long)nrows * (long long)ncols >= (1ll << 31)) return modp_fail(CLRS_ERR_INVALID, "modp_rref: nrows * ncols must be below 2^31");
    if (!modp_prime_ok(p)) return modp_fail(CLRS_ERR_INVALID, "modp_rref: p must be a prime with 2 <= p < 2^23");
    const size_t count = (size_t)nrows * (size_t)ncols;
    if (count == 0) {
        if (rank) *rank = 0;
        return 0;
    }
    if (!A || !pivots || !rank) return modp_fail(CLRS_ERR_INVALID, "modp_rref: null argument");
    for (size_t o = 0; o < count; o++)
        if (A[o] < 0 || A[o] >= p) return modp_fail(CLRS_ERR_INVALID, "modp_rref: a residue outside [0, p)");
    MODPCHECK(hipSetDevice(device));
    ModpBufs bufs;
    int32_t *d_I = nullptr;
    double *d_A = nullptr;
    int *d_flag = nullptr, *d_order = nullptr;
    MODPCHECK(bufs.get(&d_I, count)); MODPCHECK(bufs.get(&d_A, count));
    MODPCHECK(hipMemcpy(d_I, A, count * sizeof(int32_t), hipMemcpyHostToDevice));
    const dim3 flat = modp_flat_grid(count, MODP_NT);
    hipLaunchKernelGGL(k_modp_widen, flat, dim3(MODP_NT), 0, nullptr, d_I, d_A, count);
    MODPCHECK(hipGetLastError());
    MODPCHECK(bufs.drop(d_I));                                // the int32 copy is needed again only for R: 8 bytes per entry during the elimination, not 12
    d_I = nullptr;
    std::vector<int32_t> found;
    const int code = modp_eliminate(d_A, nrows, ncols, ncols, p, bufs, &d_flag, found);
    if (code != 0) return code;
    const int rk = (int)found.size();
    if (R) {
        MODPCHECK(bufs.get(&d_I, count)); MODPCHECK(bufs.get(&d_order, (size_t)nrows));
        hipLaunchKernelGGL(k_modp_order, dim3((unsigned)(((long long)nrows + MODP_NT - 1) / MODP_NT)), dim3(MODP_NT), 0, nullptr, d_flag, nrows, d_order);
        MODPCHECK(hipGetLastError());
        hipLaunchKernelGGL(k_modp_gather, flat, dim3(MODP_NT), 0, nullptr, d_A, nrows, ncols, rk, d_order, d_I);
        MODPCHECK(hipGetLastError());
    }
    MODPCHECK(hipStreamSynchronize(nullptr));
    if (R) MODPCHECK(hipMemcpy(R, d_I, count * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int t = 0; t < rk; t++) pivots[t] = found[t];
    *rank = rk;
    return 0;
}

#include "clrs_modp_lift.hip.h"      // clrs_modp_dixon_lift: the inverse mod p by the elimination above, then the p-adic lifting loop
#include "clrs_modp_rec.hip.h"       // clrs_modp_dixon_reconstruct: Horner and the half-extended Euclid per entry of the lifted solution
#include "clrs_modp_minors.hip.h"    // clrs_modp_minors: the leading principal minors of a symmetric integer matrix mod many primes, one workgroup per prime
#include "clrs_modp_minors_field.hip.h"   // clrs_modp_minors_field, clrs_modp_field_frobenius: the same minors for a matrix over a number field, D residue matrices per prime
#include "clrs_modp_tile.hip.h"      // the 64 x 64 fp64 MFMA tile loop of the two exact products below
#include "clrs_modp_zz_gemm.hip.h"   // clrs_zz_gemm: the exact product of integer matrices given in digit planes, one fp64 MFMA GEMM of one-digit matrices
#include "clrs_modp_liftm.hip.h"     // clrs_modp_dixon_lift_multi: the lifting with a matrix of right-hand sides, both products of a step as fp64 MFMA GEMMs
#include "clrs_modp_lrsys.hip.h"     // clrs_zz_lowrank_system: the rows of the rational system from low-rank constraint matrices, the digit index in the MFMA's k-extent
#include "clrs_modp_field_adjugate.hip.h"   // clrs_modp_field_adjugate: determinant and adjugate of a matrix over a number field mod split primes, one workgroup per (prime, root)

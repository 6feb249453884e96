// clrs_zz_lll.hip -- LLL reduction of a batch of integer lattices on the device (clrs_zz_lll, include/clrs_hip.h): the step that keeps the
// kernel vectors of the rounding chain short and the basis change unimodular (the reference's simplify_kernelvectors / reduction_step, src/rounding.jl:860-1104,
// which asks FLINT for an HNF and an lll).  No context, host pointers.  A translation unit of its own, compiled with -ffp-contract=off: the K-limb arithmetic
// that steers the reduction is built from two_sum and two_prod.
//
// One workgroup of LLL_NT = 256 threads per lattice, grid = the batch.  The basis rows are long integers in balanced base-2^24 digit planes in global memory and
// change only by exact integer operations; the Gram-Schmidt data (mu, r) are K-limb floating point: rows below the current index in a global workspace, the
// current row and the diagonal in LDS.  A visit of index k (every visit starts from the basis as it stands, nothing is carried over from an earlier visit):
//
//   Gram row      G_kj = <b_k, b_j>, j <= k, over the first cols_gram columns: wave w takes j = w, w + 4, ...; a lane owns the columns lane, lane + 64, ...;
//                 the 64 partial sums meet in a fixed tree (offsets 32, 16, ..., 1)
//   Cholesky row  thread j owns s_j = G_kj; for i = 0 .. k - 1: thread i publishes r_ki = s_i and mu_ki = r_ki / r_ii, every thread j > i takes
//                 s_j <- s_j - mu_ji r_ki.  Thread k ends with r_kk and, one step earlier, with s_{k-1} of the Lovasz test
//   size reduction, lazily: while some |mu_kj| > eta: for j = k - 1 down to 0, X_j = rint(head mu_kj) and thread i < j takes mu_ki <- mu_ki - X_j mu_ji; then
//                 the exact b_k <- b_k - sum_j X_j b_j, one thread per column (all columns), and the Gram and Cholesky rows again
//   Lovasz        s_{k-1} < delta r_{k-1,k-1}: two entries of the order table change places and k goes down by one; otherwise row k of mu and r_kk are kept
//                 and k goes up by one.
//
// Every loop is bounded: LLL_MAX_PASSES passes per visit, max_swaps exchanges per lattice, and at most `launch_swaps` exchanges per launch, after which the
// lattice's state (order table, k, counters) is left in global memory and the host launches again.  A launch first recomputes the rows below k of the
// Gram-Schmidt data from the basis as it stands, by the same Gram and Cholesky rows in the same order -- which is how they were computed in the first place, so the
// result does not depend on where the launches were cut.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_zz_lll_arith.h"

extern "C" void clrs_set_last_error(const char *msg);   // clrs_hip.hip: the library keeps one thread-local message
extern int g_cfg_lll_launch_swaps;                       // clrs_hip.hip, clrs_config_set("lll_launch_swaps", n): 0 = LLL_LAUNCH_SWAPS

#define LLL_LAUNCH_SWAPS 1024
#define LLL_STATE 8                 // ints of state per lattice: status, swaps, passes, launches, k

using zlll::mw;

static int lll_fail(int code, const std::string &msg) {
    clrs_set_last_error(msg.c_str());
    return code;
}
#define LLLCHECK(expr)                                                                                    \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return lll_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct LllJob {
    long long dig_off;      // of the lattice's digit planes in the pools (working copy and output)
    long long mu_off;       // of its K d^2 doubles in the workspace of mu
    int32_t d, c, cg, pad;
};

template <int K>
__device__ __forceinline__ mw<K> lll_lds_get(const double (*a)[LLL_MAX_ROWS + 1], int i) {
    mw<K> v;
#pragma unroll
    for (int l = 0; l < K; l++) v.l[l] = a[l][i];
    return v;
}
template <int K>
__device__ __forceinline__ void lll_lds_put(double (*a)[LLL_MAX_ROWS + 1], int i, const mw<K> &v) {
#pragma unroll
    for (int l = 0; l < K; l++) a[l][i] = v.l[l];
}

template <int K>
__global__ __launch_bounds__(LLL_NT) void k_zz_lll(const LllJob *__restrict__ jobs, int32_t *__restrict__ Wpool, int32_t *__restrict__ Opool, double *__restrict__ MUpool,
                                                   int32_t *__restrict__ ORD, int32_t *__restrict__ STATE, int nd, double delta, double eta, int max_swaps,
                                                   int launch_swaps) {
    __shared__ double s_rd[K][LLL_MAX_ROWS + 1];       // r_ii
    __shared__ double s_r[K][LLL_MAX_ROWS + 1];        // the Gram row, then r_ki
    __shared__ double s_mu[K][LLL_MAX_ROWS + 1];       // mu_ki
    __shared__ double s_x[LLL_MAX_ROWS];
    __shared__ double s_max;
    __shared__ int32_t s_xd[LLL_XDIGITS * LLL_MAX_ROWS], s_sh[LLL_MAX_ROWS], s_ord[LLL_MAX_ROWS];
    __shared__ int s_any, s_bad, s_qbad, s_over, s_dec;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *st = STATE + (size_t)b * LLL_STATE;
    if (st[0] != LLL_RUNNING) return;                                        // (uniform: nothing below has written st yet)
    const LllJob job = jobs[b];
    const int d = job.d, c_total = job.c, cg = job.cg;
    int32_t *D = Wpool + job.dig_off;
    double *MU = MUpool + job.mu_off;                                        // limb l of mu_ij at MU[(l * d + i) * d + j]
    const size_t mu_plane = (size_t)d * d;
    int k_resume = st[4], swaps = st[1], passes = st[2];
    if (tid < d) s_ord[tid] = ORD[(size_t)b * LLL_MAX_ROWS + tid];
    if (tid == 0) { s_bad = 0; s_over = 0; }
    __syncthreads();

    int status = LLL_RUNNING, k = 0, swaps_here = 0;
    while (status == LLL_RUNNING && k < d) {
        const bool reduce = k >= k_resume;                                   // below: the rows a launch recomputes, already reduced
        if (reduce) k_resume = 0;
        int pass = 0;
        double prevmax = 0.0;
        mw<K> s = mwa::zero<K>(), s_km1 = mwa::zero<K>();
        for (;;) {
            // ---- the Gram row into s_r
            for (int j = wave; j <= k; j += LLL_WAVES) {
                mw<K> p = zlll::lll_lane_partial<K>(D, d, c_total, nd, s_ord[k], s_ord[j], cg, lane);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    mw<K> q;
#pragma unroll
                    for (int l = 0; l < K; l++) q.l[l] = __shfl_down(p.l[l], off, 64);
                    p = zlll::lll_tree_add<K>(p, q);
                }
                if (lane == 0) lll_lds_put<K>(s_r, j, p);
            }
            __syncthreads();
            // ---- the Cholesky row
            if (tid <= k) s = lll_lds_get<K>(s_r, tid);
            for (int i = 0; i < k; i++) {
                if (tid == i) {
                    lll_lds_put<K>(s_r, i, s);
                    lll_lds_put<K>(s_mu, i, zlll::lll_chol_mu<K>(s, lll_lds_get<K>(s_rd, i)));
                }
                __syncthreads();
                if (tid > i && tid <= k) {
                    if (tid == k && i == k - 1) s_km1 = s;
                    const mw<K> mji = tid < k ? mwa::ld<K>(MU, (long)mu_plane, (long)tid * d + i) : lll_lds_get<K>(s_mu, i);
                    s = zlll::lll_chol_sub<K>(s, mji, lll_lds_get<K>(s_r, i));
                }
            }
            __syncthreads();
            // ---- is the row size-reduced?  (thread 0 walks the heads)
            if (tid == 0) {
                int any = 0, bad = 0;
                double mx = 0.0;
                for (int j = 0; j < k; j++) {
                    const mw<K> m = lll_lds_get<K>(s_mu, j);
                    if (!zlll::lll_finite(m.l[0])) bad = 1;
                    if (zlll::lll_exceeds<K>(m, eta)) any = 1;
                    mx = fmax(mx, fabs(m.l[0]));
                }
                s_any = any;
                s_max = mx;
                s_qbad = 0;
                if (bad) s_bad = 1;
            }
            __syncthreads();
            if (s_bad) { status = LLL_ARITH; break; }
            if (!reduce || !s_any) break;
            if (pass >= LLL_MAX_PASSES) { status = LLL_CAP; break; }
            if (pass > 0 && !(s_max < prevmax)) { status = LLL_ARITH; break; }            // a quotient that did not shrink
            prevmax = s_max;
            pass++;
            passes++;
            // ---- the quotients, from j = k - 1 down, the row of mu following them
            mw<K> m = tid < k ? lll_lds_get<K>(s_mu, tid) : mwa::zero<K>();
            for (int j = k - 1; j >= 0; j--) {
                if (tid == j) {
                    const double X = zlll::lll_quotient<K>(m);
                    s_x[j] = X;
                    if (zlll::lll_quotient_split(X, s_xd + LLL_XDIGITS * j, s_sh + j)) s_qbad = 1;
                }
                __syncthreads();
                const double X = s_x[j];
                if (tid < j && X != 0.0) m = zlll::lll_mu_sub_x<K>(m, mwa::ld<K>(MU, (long)mu_plane, (long)j * d + tid), X);
            }
            __syncthreads();
            if (s_qbad) { status = LLL_ARITH; break; }
            // ---- the exact row operation, one thread per column
            for (int col = tid; col < c_total; col += LLL_NT)
                if (zlll::lll_row_update_column(D, d, c_total, nd, col, s_ord, k, s_xd, s_sh)) atomicOr(&s_over, 1);
            __syncthreads();
            if (s_over) { status = LLL_OVERFLOW; break; }
        }
        if (status != LLL_RUNNING) break;
        // ---- Lovasz: thread k decides
        if (tid == k) {
            int dec = 0;                                                       // 0: keep the row, 1: exchange, 2: the arithmetic gave up
            if (reduce && k > 0) {
                if (!zlll::lll_finite(s_km1.l[0])) dec = 2;
                else if (zlll::lll_lovasz_swap<K>(s_km1, lll_lds_get<K>(s_rd, k - 1), delta)) dec = 1;
            }
            if (dec == 0 && !zlll::lll_diag_ok<K>(s)) dec = 2;
            if (dec == 0) lll_lds_put<K>(s_rd, k, s);
            s_dec = dec;
        }
        __syncthreads();
        const int dec = s_dec;
        if (dec == 2) { status = LLL_ARITH; break; }
        if (dec == 0) {
            if (tid < k) mwa::st<K>(MU, (long)mu_plane, (long)k * d + tid, lll_lds_get<K>(s_mu, tid));
            k++;
            __syncthreads();                                                   // (row k of mu is read from global memory at the next index)
        } else {
            if (tid == 0) {
                const int32_t t = s_ord[k - 1];
                s_ord[k - 1] = s_ord[k];
                s_ord[k] = t;
            }
            k--;
            swaps++;
            swaps_here++;
            __syncthreads();
            if (swaps >= max_swaps) { status = LLL_CAP; break; }
            if (swaps_here >= launch_swaps) break;                             // the host launches again
        }
    }
    if (status == LLL_RUNNING && k >= d) status = LLL_OK;
    __syncthreads();
    if (status == LLL_OK) {                                                    // the rows in their final order
        int32_t *O = Opool + job.dig_off;
        const size_t per_plane = (size_t)d * c_total;
        for (size_t o = tid; o < per_plane * nd; o += LLL_NT) {
            const size_t sp = o / per_plane, rem = o - sp * per_plane;
            const int i = (int)(rem / c_total), col = (int)(rem - (size_t)i * c_total);
            O[o] = D[(sp * d + s_ord[i]) * c_total + col];
        }
    }
    if (tid < d) ORD[(size_t)b * LLL_MAX_ROWS + tid] = s_ord[tid];
    if (tid == 0) {
        st[1] = swaps;
        st[2] = passes;
        st[3] += 1;
        st[4] = k;
        st[0] = status;
    }
}

namespace {
struct LllBufs {                       // every device buffer of a call, released on every path
    std::vector<void *> p;
    ~LllBufs() { for (void *x : p) (void)hipFree(x); }
    template <class T>
    hipError_t get(T **dptr, size_t count) {
        hipError_t e = hipMalloc((void **)dptr, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*dptr);
        return e;
    }
};
struct LllEvents {
    std::vector<hipEvent_t> e;
    explicit LllEvents(size_t count) : e(count, nullptr) {}
    ~LllEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
thread_local double t_lll_kernel_ms = 0.0, t_lll_whole_ms = 0.0;
}  // namespace

// the device times of this thread's last clrs_zz_lll: milliseconds in k_zz_lll over all launches, and from the first upload to the last download
extern "C" int clrs_zz_lll_times(double *kernel_ms, double *whole_ms) {
    if (!kernel_ms || !whole_ms) return lll_fail(CLRS_ERR_INVALID, "zz_lll_times: null argument");
    *kernel_ms = t_lll_kernel_ms;
    *whole_ms = t_lll_whole_ms;
    return 0;
}

extern "C" int clrs_zz_lll(int device, int nb, const int32_t *rows, const int32_t *cols, const int32_t *cols_gram, int nd, const int32_t *in_digits,
                           int32_t *out_digits, double delta, double eta, int limbs, int max_swaps, int32_t *info) {
    t_lll_kernel_ms = t_lll_whole_ms = 0.0;
    if (nb < 0) return lll_fail(CLRS_ERR_INVALID, "zz_lll: negative batch size");
    if (nb == 0) return 0;
    if (!rows || !cols || !cols_gram || !info) return lll_fail(CLRS_ERR_INVALID, "zz_lll: null argument");
    if (nd < 1 || nd > LLL_MAX_ND) return lll_fail(CLRS_ERR_INVALID, "zz_lll: nd must lie in [1, " + std::to_string(LLL_MAX_ND) + "]");
    if (limbs != 2 && limbs != 4 && limbs != 6) return lll_fail(CLRS_ERR_INVALID, "zz_lll: limbs must be 2, 4 or 6");
    if (!(delta > 0.25 && delta <= 1.0) || !(eta >= 0.5 && eta * eta < delta)) return lll_fail(CLRS_ERR_INVALID, "zz_lll: 1/4 < delta <= 1 and 1/2 <= eta < sqrt(delta) are needed");
    if (max_swaps < 0) return lll_fail(CLRS_ERR_INVALID, "zz_lll: max_swaps must not be negative");
    std::vector<LllJob> jobs((size_t)nb);
    long long total = 0, mu_total = 0;
    int work = 0;
    for (int b = 0; b < nb; b++) {
        const int d = rows[b], c = cols[b], g = cols_gram[b];
        if (d < 0 || d > LLL_MAX_ROWS || c < 0 || c > LLL_MAX_COLS) return lll_fail(CLRS_ERR_INVALID, "zz_lll: a lattice has more than 128 rows or 256 columns, or a negative size");
        if (g < 0 || g > c) return lll_fail(CLRS_ERR_INVALID, "zz_lll: cols_gram must lie in [0, cols]");
        if (d > 0 && g < 1) return lll_fail(CLRS_ERR_INVALID, "zz_lll: a lattice with rows needs at least one Gram column");
        jobs[b] = LllJob{total, mu_total, d, c, g, 0};
        total += (long long)nd * d * c;
        mu_total += (long long)limbs * d * d;
        if (total >= (1ll << 31)) return lll_fail(CLRS_ERR_INVALID, "zz_lll: the digit planes must hold fewer than 2^31 elements");
        work += d > 0;
    }
    if (total > 0 && (!in_digits || !out_digits)) return lll_fail(CLRS_ERR_INVALID, "zz_lll: null argument");
    for (long long o = 0; o < total; o++)
        if (in_digits[o] < -(int32_t)ZZ_HALF || in_digits[o] > (int32_t)ZZ_HALF) return lll_fail(CLRS_ERR_INVALID, "zz_lll: a digit outside [-2^23, 2^23]");
    std::vector<int32_t> state((size_t)nb * LLL_STATE, 0), ord((size_t)nb * LLL_MAX_ROWS, 0);
    for (int b = 0; b < nb; b++) {
        state[(size_t)b * LLL_STATE] = rows[b] > 0 ? LLL_RUNNING : LLL_OK;
        for (int i = 0; i < LLL_MAX_ROWS; i++) ord[(size_t)b * LLL_MAX_ROWS + i] = i;
    }
    if (work > 0) {
        LLLCHECK(hipSetDevice(device));
        LllBufs bufs;
        LllEvents ev(4);
        for (auto &e : ev.e) LLLCHECK(hipEventCreate(&e));
        LllJob *d_jobs = nullptr;
        int32_t *d_W = nullptr, *d_O = nullptr, *d_ord = nullptr, *d_state = nullptr;
        double *d_MU = nullptr;
        LLLCHECK(bufs.get(&d_jobs, (size_t)nb)); LLLCHECK(bufs.get(&d_W, (size_t)total)); LLLCHECK(bufs.get(&d_O, (size_t)total));
        LLLCHECK(bufs.get(&d_MU, (size_t)mu_total)); LLLCHECK(bufs.get(&d_ord, ord.size())); LLLCHECK(bufs.get(&d_state, state.size()));
        LLLCHECK(hipEventRecord(ev.e[0], nullptr));
        LLLCHECK(hipMemcpy(d_jobs, jobs.data(), (size_t)nb * sizeof(LllJob), hipMemcpyHostToDevice));
        LLLCHECK(hipMemcpy(d_W, in_digits, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice));
        LLLCHECK(hipMemset(d_O, 0, (size_t)total * sizeof(int32_t)));
        LLLCHECK(hipMemset(d_MU, 0, (size_t)mu_total * sizeof(double)));
        LLLCHECK(hipMemcpy(d_ord, ord.data(), ord.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        LLLCHECK(hipMemcpy(d_state, state.data(), state.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        const int launch_swaps = g_cfg_lll_launch_swaps > 0 ? g_cfg_lll_launch_swaps : LLL_LAUNCH_SWAPS;
        const long long max_launches = (long long)max_swaps / launch_swaps + 2;          // a launch ends a lattice or takes launch_swaps exchanges from its budget
        for (long long it = 0; it < max_launches; it++) {
            LLLCHECK(hipEventRecord(ev.e[2], nullptr));
            if (limbs == 2) hipLaunchKernelGGL(k_zz_lll<2>, dim3((unsigned)nb), dim3(LLL_NT), 0, nullptr, d_jobs, d_W, d_O, d_MU, d_ord, d_state, nd, delta, eta, max_swaps, launch_swaps);
            else if (limbs == 4) hipLaunchKernelGGL(k_zz_lll<4>, dim3((unsigned)nb), dim3(LLL_NT), 0, nullptr, d_jobs, d_W, d_O, d_MU, d_ord, d_state, nd, delta, eta, max_swaps, launch_swaps);
            else hipLaunchKernelGGL(k_zz_lll<6>, dim3((unsigned)nb), dim3(LLL_NT), 0, nullptr, d_jobs, d_W, d_O, d_MU, d_ord, d_state, nd, delta, eta, max_swaps, launch_swaps);
            LLLCHECK(hipGetLastError());
            LLLCHECK(hipEventRecord(ev.e[3], nullptr));
            LLLCHECK(hipMemcpy(state.data(), d_state, state.size() * sizeof(int32_t), hipMemcpyDeviceToHost));      // (synchronises)
            float ms = 0.f;
            LLLCHECK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
            t_lll_kernel_ms += ms;
            bool running = false;
            for (int b = 0; b < nb; b++) running = running || state[(size_t)b * LLL_STATE] == LLL_RUNNING;
            if (!running) break;
        }
        std::vector<int32_t> out((size_t)total);
        LLLCHECK(hipMemcpy(out.data(), d_O, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
        LLLCHECK(hipEventRecord(ev.e[1], nullptr));
        LLLCHECK(hipEventSynchronize(ev.e[1]));
        float ms = 0.f;
        LLLCHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        t_lll_whole_ms = ms;
        for (int b = 0; b < nb; b++) {
            int32_t *st = &state[(size_t)b * LLL_STATE];
            if (st[0] == LLL_RUNNING) st[0] = LLL_CAP;                        // (cannot happen: the launches cover max_swaps)
            const size_t count = (size_t)nd * rows[b] * cols[b];
            if (st[0] == LLL_OK && count) std::memcpy(out_digits + jobs[b].dig_off, out.data() + jobs[b].dig_off, count * sizeof(int32_t));
        }
    }
    std::memcpy(info, state.data(), state.size() * sizeof(int32_t));
    return 0;
}

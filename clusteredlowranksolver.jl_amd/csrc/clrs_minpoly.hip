// clrs_minpoly.hip -- minimal polynomials of multi-word numbers by integer relations among their powers, on the device (clrs_mw_minpoly, include/clrs_hip.h;
// DESIGN.md section 27): the numeric core of find_field.  No context, host pointers.  A translation unit of its own, compiled with -ffp-contract=off: the
// arithmetic (clrs_minpoly_arith.h over clrs_mw_field_round_arith.h) is built from two_sum and two_prod.
//
// One lane per number, workgroups of one wave.  Everything a number keeps between rungs -- the digits of the fixed-point images of its powers, the exact
// integers U and c, the rung and the counters -- lives in a lane-strided global workspace (element e of lane i at e * count + i), the Gram-Schmidt data of a
// visit in registers.  A launch advances every lane by at most `field_round_launch_rungs` rungs and returns; the host launches again while a lane is still
// running.  Nothing but the workspace survives a rung, so the result does not depend on where the launches were cut.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_minpoly_arith.h"

extern "C" void clrs_set_last_error(const char *msg);   // clrs_hip.hip: the library keeps one thread-local message
extern int g_cfg_field_round_launch_rungs;               // clrs_hip.hip, clrs_config_set("field_round_launch_rungs", n): 0 = FR_LAUNCH_RUNGS

#define MP_NT 64

using mpoly::MpArgs;

static int mp_fail(int code, const std::string &msg) {
    clrs_set_last_error(msg.c_str());
    return code;
}
#define MPCHECK(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return mp_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// grid: ceil(count / MP_NT) workgroups of one wave, one lane per number; every pool is compact (plane = stride = count)
template <int K, int D>
__global__ __launch_bounds__(MP_NT) void k_mw_minpoly(MpArgs a, int first, int launch_rungs) {
    const long long i = (long long)blockIdx.x * MP_NT + threadIdx.x;
    if (i >= a.count) return;
    mpoly::mp_lane<K, D>(a, i, first, launch_rungs);
}

namespace {
struct MpBufs {                        // every device buffer of a call, released on every path
    std::vector<void *> p;
    ~MpBufs() { for (void *x : p) (void)hipFree(x); }
    template <class T>
    hipError_t get(T **dptr, size_t count) {
        hipError_t e = hipMalloc((void **)dptr, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*dptr);
        return e;
    }
};
struct MpEvents {
    std::vector<hipEvent_t> e;
    explicit MpEvents(size_t count) : e(count, nullptr) {}
    ~MpEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
thread_local double t_mp_kernel_ms = 0.0, t_mp_whole_ms = 0.0;

template <int K>
void mp_launch(int deg, unsigned grid, const MpArgs &a, int first, int launch_rungs) {
    if (deg == 1) hipLaunchKernelGGL((k_mw_minpoly<K, 2>), dim3(grid), dim3(MP_NT), 0, nullptr, a, first, launch_rungs);
    else if (deg == 2) hipLaunchKernelGGL((k_mw_minpoly<K, 3>), dim3(grid), dim3(MP_NT), 0, nullptr, a, first, launch_rungs);
    else if (deg == 3) hipLaunchKernelGGL((k_mw_minpoly<K, 4>), dim3(grid), dim3(MP_NT), 0, nullptr, a, first, launch_rungs);
    else hipLaunchKernelGGL((k_mw_minpoly<K, 5>), dim3(grid), dim3(MP_NT), 0, nullptr, a, first, launch_rungs);
}
}  // namespace

#define MP_BY_LIMBS(call)                  \
    do {                                   \
        if (limbs == 4) { call(4); }       \
        else if (limbs == 5) { call(5); }  \
        else if (limbs == 6) { call(6); }  \
        else if (limbs == 8) { call(8); }  \
        else { call(10); }                 \
    } while (0)

// the device times of this thread's last clrs_mw_minpoly: milliseconds in k_mw_minpoly over all launches, and from the first upload to the last download
extern "C" int clrs_mw_minpoly_times(double *kernel_ms, double *whole_ms) {
    if (!kernel_ms || !whole_ms) return mp_fail(CLRS_ERR_INVALID, "minpoly_times: null argument");
    *kernel_ms = t_mp_kernel_ms;
    *whole_ms = t_mp_whole_ms;
    return 0;
}

extern "C" int clrs_mw_minpoly(int device, int limbs, int deg, int count, const double *v, int plane, int bits, double errbound, int nd, int32_t *rel,
                               int32_t *status, int32_t *rung, double *err, int32_t *info) {
    t_mp_kernel_ms = t_mp_whole_ms = 0.0;
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return mp_fail(CLRS_ERR_INVALID, "minpoly: limbs must be 4, 5, 6, 8 or 10");
    if (deg < MP_MIN_DEG || deg > MP_MAX_DEG) return mp_fail(CLRS_ERR_INVALID, "minpoly: the degree must lie in [1, 4]");
    if (count < 0) return mp_fail(CLRS_ERR_INVALID, "minpoly: negative count");
    if (plane < count) return mp_fail(CLRS_ERR_INVALID, "minpoly: the numbers leave their plane");
    if (!(errbound > 0.0)) return mp_fail(CLRS_ERR_INVALID, "minpoly: errbound must be positive");
    if (bits < 1) return mp_fail(CLRS_ERR_INVALID, "minpoly: bits must be at least 1");
    if (nd < 1 || nd > LLL_MAX_ND) return mp_fail(CLRS_ERR_INVALID, "minpoly: nd must lie in [1, " + std::to_string(LLL_MAX_ND) + "]");
    if (count > 0 && (!v || !rel || !status || !rung || !err || !info)) return mp_fail(CLRS_ERR_INVALID, "minpoly: null argument");
    if (count == 0) return 0;
    const int D = deg + 1, P = frnd::fr_top_bits(bits, limbs), nw = frnd::fr_w_digits(P), elems = mpoly::mp_ws_elems(D, P, nd);
    const size_t n = (size_t)count;
    std::vector<double> hv((size_t)limbs * n);
    for (int l = 0; l < limbs; l++) std::memcpy(hv.data() + (size_t)l * n, v + (size_t)l * plane, n * sizeof(double));

    MPCHECK(hipSetDevice(device));
    MpBufs bufs;
    MpEvents ev(4);
    for (auto &e : ev.e) MPCHECK(hipEventCreate(&e));
    double *d_v = nullptr, *d_err = nullptr;
    int32_t *d_rel = nullptr, *d_status = nullptr, *d_rung = nullptr, *d_info = nullptr, *d_ws = nullptr;
    MPCHECK(bufs.get(&d_v, hv.size())); MPCHECK(bufs.get(&d_rel, (size_t)nd * D * n)); MPCHECK(bufs.get(&d_status, n));
    MPCHECK(bufs.get(&d_rung, n)); MPCHECK(bufs.get(&d_err, n)); MPCHECK(bufs.get(&d_info, 2 * n)); MPCHECK(bufs.get(&d_ws, (size_t)elems * n));
    MPCHECK(hipEventRecord(ev.e[0], nullptr));
    MPCHECK(hipMemcpy(d_v, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice));
    MpArgs a;
    a.v = d_v; a.plane_v = (long long)n;
    a.count = count; a.P = P; a.nw = nw; a.nd = nd; a.errbound = errbound;
    a.ws = d_ws; a.stride = (long long)n;
    a.rel = d_rel; a.status = d_status; a.rung = d_rung; a.err = d_err; a.info = d_info; a.plane = (long long)n;
    const int launch_rungs = g_cfg_field_round_launch_rungs > 0 ? g_cfg_field_round_launch_rungs : FR_LAUNCH_RUNGS;
    const int max_launches = frnd::fr_rungs(P) / launch_rungs + 2;          // a launch ends a lane or takes launch_rungs rungs off its ladder
    const unsigned grid = (unsigned)((n + MP_NT - 1) / MP_NT);
    std::vector<int32_t> head(n);
    double kernel_ms = 0.0;
    for (int it = 0; it < max_launches; it++) {
        MPCHECK(hipEventRecord(ev.e[2], nullptr));
#define MP_LAUNCH(Kc) mp_launch<Kc>(deg, grid, a, it == 0, launch_rungs)
        MP_BY_LIMBS(MP_LAUNCH);
#undef MP_LAUNCH
        MPCHECK(hipGetLastError());
        MPCHECK(hipEventRecord(ev.e[3], nullptr));
        MPCHECK(hipMemcpy(head.data(), d_ws, n * sizeof(int32_t), hipMemcpyDeviceToHost));          // the status row of the workspace (synchronises)
        float ms = 0.f;
        MPCHECK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
        kernel_ms += ms;
        bool running = false;
        for (size_t i = 0; i < n; i++) running = running || head[i] == FR_RUNNING;
        if (!running) break;
    }
    t_mp_kernel_ms = kernel_ms;
    for (size_t i = 0; i < n; i++)
        if (head[i] == FR_RUNNING) return mp_fail(CLRS_ERR_HIP, "minpoly: a number was still running after the last launch");   // (cannot happen: the launches cover the ladder)
    std::vector<int32_t> h_rel((size_t)nd * D * n), h_info(2 * n);
    MPCHECK(hipMemcpy(h_rel.data(), d_rel, h_rel.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MPCHECK(hipMemcpy(h_info.data(), d_info, h_info.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MPCHECK(hipMemcpy(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    MPCHECK(hipMemcpy(rung, d_rung, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    MPCHECK(hipMemcpy(err, d_err, n * sizeof(double), hipMemcpyDeviceToHost));
    MPCHECK(hipEventRecord(ev.e[1], nullptr));
    MPCHECK(hipEventSynchronize(ev.e[1]));
    float ms = 0.f;
    MPCHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    t_mp_whole_ms = ms;
    for (int r = 0; r < nd * D; r++) std::memcpy(rel + (size_t)r * plane, h_rel.data() + (size_t)r * n, n * sizeof(int32_t));
    for (int r = 0; r < 2; r++) std::memcpy(info + (size_t)r * plane, h_info.data() + (size_t)r * n, n * sizeof(int32_t));
    return 0;
}

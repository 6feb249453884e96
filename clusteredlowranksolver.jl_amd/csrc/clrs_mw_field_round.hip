// clrs_mw_field_round.hip -- rounding multi-word numbers to a number field of degree 2 .. 4 by integer relations on the device (clrs_mw_field_round,
// include/clrs_hip.h): the degree-d counterpart of clrs_mw_rationalize.  No context, host pointers.  A translation unit of its own,
// compiled with -ffp-contract=off: the arithmetic (clrs_mw_field_round_arith.h) is built from two_sum and two_prod.
//
// One lane per number, workgroups of one wave.  Everything a number keeps between rungs -- the digits of its fixed-point image, the exact integers U and c, the
// rung and the counters -- lives in a lane-strided global workspace (element e of lane i at e * count + i), the Gram-Schmidt data of a visit in registers.  A
// launch advances every lane by at most `field_round_launch_rungs` rungs and returns; the host launches again while a lane is still running.  Nothing but the
// workspace survives a rung, so the result does not depend on where the launches were cut.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_mw_field_round_arith.h"

extern "C" void clrs_set_last_error(const char *msg);   // clrs_hip.hip: the library keeps one thread-local message
extern int g_cfg_field_round_launch_rungs;               // clrs_hip.hip, clrs_config_set("field_round_launch_rungs", n): 0 = FR_LAUNCH_RUNGS

#define FR_NT 64

using frnd::FrArgs;

static int fr_fail(int code, const std::string &msg) {
    clrs_set_last_error(msg.c_str());
    return code;
}
#define FRCHECK(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fr_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// grid: ceil(count / FR_NT) workgroups of one wave, one lane per number; every pool is compact (plane = stride = count)
template <int K, int D>
__global__ __launch_bounds__(FR_NT) void k_mw_field_round(FrArgs a, int first, int launch_rungs) {
    const long long i = (long long)blockIdx.x * FR_NT + threadIdx.x;
    if (i >= a.count) return;
    frnd::fr_lane<K, D>(a, i, first, launch_rungs);
}

namespace {
struct FrBufs {                        // every device buffer of a call, released on every path
    std::vector<void *> p;
    ~FrBufs() { for (void *x : p) (void)hipFree(x); }
    template <class T>
    hipError_t get(T **dptr, size_t count) {
        hipError_t e = hipMalloc((void **)dptr, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*dptr);
        return e;
    }
};
struct FrEvents {
    std::vector<hipEvent_t> e;
    explicit FrEvents(size_t count) : e(count, nullptr) {}
    ~FrEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
thread_local double t_fr_kernel_ms = 0.0, t_fr_whole_ms = 0.0;

template <int K>
void fr_gw(const double *gpow, int deg, int P, int nw, int32_t *gw) {
    for (int k = 0; k < deg; k++) {
        double s[K];
        for (int l = 0; l < K; l++) s[l] = gpow[(size_t)l * deg + k];
        mwa::renorm<K>(s);
        mwa::mw<K> x;
        for (int l = 0; l < K; l++) x.l[l] = s[l];
        frnd::fr_fixed_point<K>(x, P, nw, gw + (size_t)k * nw, 1);
    }
}

template <int K>
void fr_launch(int deg, unsigned grid, const FrArgs &a, int first, int launch_rungs) {
    if (deg == 2) hipLaunchKernelGGL((k_mw_field_round<K, 3>), dim3(grid), dim3(FR_NT), 0, nullptr, a, first, launch_rungs);
    else if (deg == 3) hipLaunchKernelGGL((k_mw_field_round<K, 4>), dim3(grid), dim3(FR_NT), 0, nullptr, a, first, launch_rungs);
    else hipLaunchKernelGGL((k_mw_field_round<K, 5>), dim3(grid), dim3(FR_NT), 0, nullptr, a, first, launch_rungs);
}
}  // namespace

#define FR_BY_LIMBS(call)                  \
    do {                                   \
        if (limbs == 4) { call(4); }       \
        else if (limbs == 5) { call(5); }  \
        else if (limbs == 6) { call(6); }  \
        else if (limbs == 8) { call(8); }  \
        else { call(10); }                 \
    } while (0)

// the device times of this thread's last clrs_mw_field_round: milliseconds in k_mw_field_round over all launches, and from the first upload to the last download
extern "C" int clrs_mw_field_round_times(double *kernel_ms, double *whole_ms) {
    if (!kernel_ms || !whole_ms) return fr_fail(CLRS_ERR_INVALID, "field_round_times: null argument");
    *kernel_ms = t_fr_kernel_ms;
    *whole_ms = t_fr_whole_ms;
    return 0;
}

// The device part, shared with clrs_mw_kernel_vectors_field (clrs_mw.hip): d_v is a compact device pool [limbs][count], every output a compact device pool
// (rel [nd][deg + 1][count], status, rung, err [count], vq [limbs][count], info [2][count]); gpow is a host pointer.  The arguments are the caller's to check,
// but for the powers of g.  Returns synchronised; *kernel_ms: the milliseconds in k_mw_field_round over all launches.
int mw_field_round_on_device(int limbs, int deg, const double *gpow, int count, const double *d_v, int bits, double errbound, int nd, int32_t *d_rel,
                             int32_t *d_status, int32_t *d_rung, double *d_err, double *d_vq, int32_t *d_info, double *kernel_ms) {
    *kernel_ms = 0.0;
    for (int t = 0; t < limbs * deg; t++)
        if (!zlll::lll_finite(gpow[t]) || !(fabs(gpow[t]) < FR_V_LIMIT)) return fr_fail(CLRS_ERR_INVALID, "field_round: a power of g is not finite or not below 2^22");
    if (count == 0) return 0;
    const int D = deg + 1, P = frnd::fr_top_bits(bits, limbs), nw = frnd::fr_w_digits(P), elems = frnd::fr_ws_elems(D, P, nd);
    std::vector<int32_t> gw((size_t)deg * nw);
#define FR_GW(Kc) fr_gw<Kc>(gpow, deg, P, nw, gw.data())
    FR_BY_LIMBS(FR_GW);
#undef FR_GW
    const size_t n = (size_t)count;
    FrBufs bufs;
    FrEvents ev(2);
    for (auto &e : ev.e) FRCHECK(hipEventCreate(&e));
    double *d_g = nullptr;
    int32_t *d_gw = nullptr, *d_ws = nullptr;
    FRCHECK(bufs.get(&d_g, (size_t)limbs * deg)); FRCHECK(bufs.get(&d_gw, gw.size())); FRCHECK(bufs.get(&d_ws, (size_t)elems * n));
    FRCHECK(hipMemcpy(d_g, gpow, (size_t)limbs * deg * sizeof(double), hipMemcpyHostToDevice));
    FRCHECK(hipMemcpy(d_gw, gw.data(), gw.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    FrArgs a;
    a.v = d_v; a.plane_v = (long long)n; a.gpow = d_g; a.gw = d_gw;
    a.count = count; a.P = P; a.nw = nw; a.nd = nd; a.errbound = errbound;
    a.ws = d_ws; a.stride = (long long)n;
    a.rel = d_rel; a.status = d_status; a.rung = d_rung; a.err = d_err; a.vq = d_vq; a.info = d_info; a.plane = (long long)n;
    const int launch_rungs = g_cfg_field_round_launch_rungs > 0 ? g_cfg_field_round_launch_rungs : FR_LAUNCH_RUNGS;
    const int max_launches = frnd::fr_rungs(P) / launch_rungs + 2;          // a launch ends a lane or takes launch_rungs rungs off its ladder
    const unsigned grid = (unsigned)((n + FR_NT - 1) / FR_NT);
    std::vector<int32_t> head(n);
    for (int it = 0; it < max_launches; it++) {
        FRCHECK(hipEventRecord(ev.e[0], nullptr));
#define FR_LAUNCH(Kc) fr_launch<Kc>(deg, grid, a, it == 0, launch_rungs)
        FR_BY_LIMBS(FR_LAUNCH);
#undef FR_LAUNCH
        FRCHECK(hipGetLastError());
        FRCHECK(hipEventRecord(ev.e[1], nullptr));
        FRCHECK(hipMemcpy(head.data(), d_ws, n * sizeof(int32_t), hipMemcpyDeviceToHost));          // the status row of the workspace (synchronises)
        float ms = 0.f;
        FRCHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *kernel_ms += ms;
        bool running = false;
        for (size_t i = 0; i < n; i++) running = running || head[i] == FR_RUNNING;
        if (!running) break;
    }
    for (size_t i = 0; i < n; i++)
        if (head[i] == FR_RUNNING) return fr_fail(CLRS_ERR_HIP, "field_round: a number was still running after the last launch");   // (cannot happen: the launches cover the ladder)
    return 0;
}

extern "C" int clrs_mw_field_round(int device, int limbs, int deg, const double *gpow, int count, const double *v, int plane, int bits, double errbound, int nd,
                                   int32_t *rel, int32_t *status, int32_t *rung, double *err, double *vq, int32_t *info) {
    t_fr_kernel_ms = t_fr_whole_ms = 0.0;
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return fr_fail(CLRS_ERR_INVALID, "field_round: limbs must be 4, 5, 6, 8 or 10");
    if (deg < FR_MIN_DEG || deg > FR_MAX_DEG) return fr_fail(CLRS_ERR_INVALID, "field_round: the degree must lie in [2, 4]");
    if (count < 0) return fr_fail(CLRS_ERR_INVALID, "field_round: negative count");
    if (plane < count) return fr_fail(CLRS_ERR_INVALID, "field_round: the numbers leave their plane");
    if (!(errbound > 0.0)) return fr_fail(CLRS_ERR_INVALID, "field_round: errbound must be positive");
    if (bits < 1) return fr_fail(CLRS_ERR_INVALID, "field_round: bits must be at least 1");
    if (nd < 1 || nd > LLL_MAX_ND) return fr_fail(CLRS_ERR_INVALID, "field_round: nd must lie in [1, " + std::to_string(LLL_MAX_ND) + "]");
    if (count > 0 && (!gpow || !v || !rel || !status || !rung || !err || !vq || !info)) return fr_fail(CLRS_ERR_INVALID, "field_round: null argument");
    if (count == 0) return 0;
    for (int t = 0; t < limbs * deg; t++)
        if (!zlll::lll_finite(gpow[t]) || !(fabs(gpow[t]) < FR_V_LIMIT)) return fr_fail(CLRS_ERR_INVALID, "field_round: a power of g is not finite or not below 2^22");
    const int D = deg + 1;
    const size_t n = (size_t)count;
    std::vector<double> hv((size_t)limbs * n);
    for (int l = 0; l < limbs; l++) std::memcpy(hv.data() + (size_t)l * n, v + (size_t)l * plane, n * sizeof(double));

    FRCHECK(hipSetDevice(device));
    FrBufs bufs;
    FrEvents ev(2);
    for (auto &e : ev.e) FRCHECK(hipEventCreate(&e));
    double *d_v = nullptr, *d_err = nullptr, *d_vq = nullptr;
    int32_t *d_rel = nullptr, *d_status = nullptr, *d_rung = nullptr, *d_info = nullptr;
    FRCHECK(bufs.get(&d_v, hv.size())); FRCHECK(bufs.get(&d_rel, (size_t)nd * D * n)); FRCHECK(bufs.get(&d_status, n));
    FRCHECK(bufs.get(&d_rung, n)); FRCHECK(bufs.get(&d_err, n)); FRCHECK(bufs.get(&d_vq, (size_t)limbs * n)); FRCHECK(bufs.get(&d_info, 2 * n));
    FRCHECK(hipEventRecord(ev.e[0], nullptr));
    FRCHECK(hipMemcpy(d_v, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice));
    double kernel_ms = 0.0;
    const int rc = mw_field_round_on_device(limbs, deg, gpow, count, d_v, bits, errbound, nd, d_rel, d_status, d_rung, d_err, d_vq, d_info, &kernel_ms);
    t_fr_kernel_ms = kernel_ms;
    if (rc) return rc;
    std::vector<int32_t> h_rel((size_t)nd * D * n), h_info(2 * n);
    std::vector<double> h_vq((size_t)limbs * n);
    FRCHECK(hipMemcpy(h_rel.data(), d_rel, h_rel.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    FRCHECK(hipMemcpy(h_info.data(), d_info, h_info.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    FRCHECK(hipMemcpy(h_vq.data(), d_vq, h_vq.size() * sizeof(double), hipMemcpyDeviceToHost));
    FRCHECK(hipMemcpy(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    FRCHECK(hipMemcpy(rung, d_rung, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    FRCHECK(hipMemcpy(err, d_err, n * sizeof(double), hipMemcpyDeviceToHost));
    FRCHECK(hipEventRecord(ev.e[1], nullptr));
    FRCHECK(hipEventSynchronize(ev.e[1]));
    float ms = 0.f;
    FRCHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    t_fr_whole_ms = ms;
    for (int r = 0; r < nd * D; r++) std::memcpy(rel + (size_t)r * plane, h_rel.data() + (size_t)r * n, n * sizeof(int32_t));
    for (int r = 0; r < 2; r++) std::memcpy(info + (size_t)r * plane, h_info.data() + (size_t)r * n, n * sizeof(int32_t));
    for (int l = 0; l < limbs; l++) std::memcpy(vq + (size_t)l * plane, h_vq.data() + (size_t)l * n, n * sizeof(double));
    return 0;
}

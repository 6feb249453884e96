// minpoly_host.cpp -- csrc/clrs_minpoly_arith.h compiled for the host (g++ -ffp-contract=off), and clrs_mw_minpoly restated around it: the lanes become a
// loop, the workspace keeps its lane-strided layout, a launch is a call of mp_lane per lane -- every operation is the same function in the same order, so the
// device result equals this one digit for digit.  tests/minpoly_util.py builds and binds it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_minpoly_arith.h"

using mpoly::MpArgs;

namespace {
struct Run {
    int limbs, deg, count;
    std::vector<double> v, err;
    std::vector<int32_t> ws, rel, status, rung, info;
    MpArgs a;
    bool first = true;
};

template <int K>
void lanes(Run &r, int launch_rungs) {
    for (long long i = 0; i < r.count; i++) {
        if (r.deg == 1) mpoly::mp_lane<K, 2>(r.a, i, r.first, launch_rungs);
        else if (r.deg == 2) mpoly::mp_lane<K, 3>(r.a, i, r.first, launch_rungs);
        else if (r.deg == 3) mpoly::mp_lane<K, 4>(r.a, i, r.first, launch_rungs);
        else mpoly::mp_lane<K, 5>(r.a, i, r.first, launch_rungs);
    }
    r.first = false;
}

#define BY_LIMBS(r, call)                          \
    do {                                           \
        if ((r).limbs == 4) { call(4); }           \
        else if ((r).limbs == 5) { call(5); }      \
        else if ((r).limbs == 6) { call(6); }      \
        else if ((r).limbs == 8) { call(8); }      \
        else { call(10); }                         \
    } while (0)
}  // namespace

extern "C" {

// [FR_HDR, FR_LAUNCH_RUNGS, LLL_MAX_ND, top rung, rungs, nw, workspace elements] for (bits, limbs, deg, nd)
int minpoly_plan_host(int bits, int limbs, int deg, int nd, int32_t *out) {
    const int P = frnd::fr_top_bits(bits, limbs);
    const int32_t v[7] = {FR_HDR, FR_LAUNCH_RUNGS, LLL_MAX_ND, P, frnd::fr_rungs(P), frnd::fr_w_digits(P), mpoly::mp_ws_elems(deg + 1, P, nd)};
    std::memcpy(out, v, sizeof v);
    return 0;
}

// the state of one call: compact pools (plane = stride = count), nothing launched yet.  No validation: the caller passes what clrs_mw_minpoly accepts.
void *minpoly_open_host(int limbs, int deg, int count, const double *v, int plane, int bits, double errbound, int nd) {
    Run *r = new Run;
    const size_t n = (size_t)count;
    const int D = deg + 1;
    r->limbs = limbs; r->deg = deg; r->count = count;
    r->v.resize((size_t)limbs * n);
    for (int l = 0; l < limbs; l++) std::memcpy(r->v.data() + (size_t)l * n, v + (size_t)l * plane, n * sizeof(double));
    MpArgs &a = r->a;
    a.P = frnd::fr_top_bits(bits, limbs);
    a.nw = frnd::fr_w_digits(a.P);
    a.nd = nd;
    a.count = count;
    a.errbound = errbound;
    r->ws.assign((size_t)mpoly::mp_ws_elems(D, a.P, nd) * n, -7);
    r->rel.assign((size_t)nd * D * n, -7); r->status.assign(n, -7); r->rung.assign(n, -7); r->info.assign(2 * n, -7);
    r->err.assign(n, -7.0);
    a.v = r->v.data(); a.plane_v = (long long)n;
    a.ws = r->ws.data(); a.stride = (long long)n;
    a.rel = r->rel.data(); a.status = r->status.data(); a.rung = r->rung.data(); a.err = r->err.data(); a.info = r->info.data();
    a.plane = (long long)n;
    return r;
}

// one launch: every lane advances by at most launch_rungs rungs; returns the lanes still running
int minpoly_launch_host(void *h, int launch_rungs) {
    Run &r = *(Run *)h;
#define LANES(Kc) lanes<Kc>(r, launch_rungs)
    BY_LIMBS(r, LANES);
#undef LANES
    int running = 0;
    for (int i = 0; i < r.count; i++) running += r.ws[i] == FR_RUNNING;
    return running;
}

// the outputs, into pools of `plane` entries per row: entry i < count of every row and nothing behind them
int minpoly_close_host(void *h, int plane, int32_t *rel, int32_t *status, int32_t *rung, double *err, int32_t *info) {
    Run *r = (Run *)h;
    const size_t n = (size_t)r->count;
    const int D = r->deg + 1;
    if (rel) {
        for (int t = 0; t < r->a.nd * D; t++) std::memcpy(rel + (size_t)t * plane, r->rel.data() + (size_t)t * n, n * sizeof(int32_t));
        for (int t = 0; t < 2; t++) std::memcpy(info + (size_t)t * plane, r->info.data() + (size_t)t * n, n * sizeof(int32_t));
        std::memcpy(status, r->status.data(), n * sizeof(int32_t));
        std::memcpy(rung, r->rung.data(), n * sizeof(int32_t));
        std::memcpy(err, r->err.data(), n * sizeof(double));
    }
    delete r;
    return 0;
}
}

// Host build of the rational rounding (csrc/clrs_mw_rational.hip.h): the SAME mw_cf_round / mw_from_ratio the kernel k_mw_rationalize calls, over a planar
// pool as the kernel walks it.  Test infrastructure; compiled by tests/rationalize_util.py (g++ -O2 -std=c++17 -ffp-contract=off).
#include <cstdint>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_rational.hip.h"
using namespace mwa;

template <int K>
static void pool(int count, const double *v, long plane, double errbound, double *num, double *den, int32_t *status, double *vq) {
    for (long i = 0; i < count; i++) {
        double p, q;
        status[i] = mw_cf_round<K>(ld<K>(v, plane, i), errbound, p, q);
        num[i] = p;
        den[i] = q;
        st<K>(vq, plane, i, mw_from_ratio<K>(p, q));
    }
}

// v, vq planar [K][plane]; the first `count` entries of num, den, status and of every plane of vq are written.  Returns -1 for a limb count not on offer.
extern "C" int mw_rationalize_host(int K, int count, const double *v, long plane, double errbound, double *num, double *den, int32_t *status, double *vq) {
    switch (K) {
    case 4: pool<4>(count, v, plane, errbound, num, den, status, vq); return 0;
    case 5: pool<5>(count, v, plane, errbound, num, den, status, vq); return 0;
    case 6: pool<6>(count, v, plane, errbound, num, den, status, vq); return 0;
    case 8: pool<8>(count, v, plane, errbound, num, den, status, vq); return 0;
    case 10: pool<10>(count, v, plane, errbound, num, den, status, vq); return 0;
    }
    return -1;
}

// The host-only table builder of the multi-word contexts (csrc/clrs_mw_tables.h: mw_build_tables, mw_cut_digits) behind a thin C surface that copies
// the vectors out by name.  Test infrastructure; compiled by tests/test_mw_tables_cpu.py (g++ -O2 -std=c++17 -ffp-contract=off), no HIP anywhere.
#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_mw_tables.h"

#include <cstdio>

namespace {
struct View { const void *p; long n; int width; };      // n elements of `width` bytes
template <class T>
View view(const std::vector<T> &v) { return View{v.data(), (long)v.size(), (int)sizeof(T)}; }

bool find(const MwTables &t, const std::string &name, View &out) {
#define MWT_ARRAY(f) if (name == #f) { out = view(t.f); return true; }
    MWT_ARRAY(blk) MWT_ARRAY(clu) MWT_ARRAY(lr_list) MWT_ARRAY(dn_list) MWT_ARRAY(V) MWT_ARRAY(dA) MWT_ARRAY(st_lam) MWT_ARRAY(B) MWT_ARRAY(vrow)
    MWT_ARRAY(tptr) MWT_ARRAY(st_a) MWT_ARRAY(st_b) MWT_ARRAY(st_orig) MWT_ARRAY(st_p) MWT_ARRAY(st_war) MWT_ARRAY(st_wac) MWT_ARRAY(st_trl)
    MWT_ARRAY(st_trd) MWT_ARRAY(st_flag) MWT_ARRAY(ay_a) MWT_ARRAY(ay_b) MWT_ARRAY(ay_blk) MWT_ARRAY(dmap) MWT_ARRAY(dense_p) MWT_ARRAY(drow_ptr)
    MWT_ARRAY(drow_blk) MWT_ARRAY(drow_en)
#undef MWT_ARRAY
    return false;
}
}  // namespace

extern "C" {

// the tables of a description, or null with the code in *rc and the message in err
void *mwt_build(const clrs_sdp_desc *d, int data_limbs, int *rc, char *err, int errlen) {
    MwTables *t = new MwTables();
    std::string msg;
    *rc = mw_build_tables(d, data_limbs, *t, msg);
    std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
    if (*rc == 0) return t;
    delete t;
    return nullptr;
}
void mwt_free(void *h) { delete (MwTables *)h; }

long mwt_len(const void *h, const char *name) {
    View v;
    return find(*(const MwTables *)h, name, v) ? v.n : -1;
}
int mwt_width(const void *h, const char *name) {
    View v;
    return find(*(const MwTables *)h, name, v) ? v.width : -1;
}
int mwt_copy(const void *h, const char *name, void *dst) {
    View v;
    if (!find(*(const MwTables *)h, name, v)) return -1;
    if (v.n) std::memcpy(dst, v.p, (size_t)v.n * v.width);
    return 0;
}
// the sizes and counters, by name (all exact in a double)
double mwt_scalar(const void *h, const char *name_) {
    const MwTables &t = *(const MwTables *)h;
    const std::string name = name_;
#define MWT_SCALAR(f) if (name == #f) return (double)t.f;
    MWT_SCALAR(J) MWT_SCALAR(N) MWT_SCALAR(NB) MWT_SCALAR(DK) MWT_SCALAR(T) MWT_SCALAR(D) MWT_SCALAR(xlen) MWT_SCALAR(Slen) MWT_SCALAR(xylen)
    MWT_SCALAR(xrdlen) MWT_SCALAR(zlen) MWT_SCALAR(glen) MWT_SCALAR(sdlen) MWT_SCALAR(wlen) MWT_SCALAR(Vp) MWT_SCALAR(dAp) MWT_SCALAR(lamp) MWT_SCALAR(Bp)
    MWT_SCALAR(maxU) MWT_SCALAR(maxP) MWT_SCALAR(maxn) MWT_SCALAR(maxn_dense) MWT_SCALAR(maxTb) MWT_SCALAR(maxcnt) MWT_SCALAR(dn_big) MWT_SCALAR(sa_lanes)
    MWT_SCALAR(n_one_term) MWT_SCALAR(n_many_term) MWT_SCALAR(cnt_mul) MWT_SCALAR(cnt_factor) MWT_SCALAR(cnt_solve)
#undef MWT_SCALAR
    return -1e300;
}

int mwt_beta(void) { return MWS_BETA; }
int mwt_slices(int K) { return mws_slices(K); }
int mwt_exponent(double head) { return mwk::mws_exponent(head); }
// digits[s], s < S, of x0 + x1 at the window exponent e, as fp32 -- what the creation stages store
void mwt_cut(double x0, double x1, int e, int S, float *digits) {
    mw_cut_digits(x0, x1, e, S, [&](int s, float dgt) { digits[s] = dgt; });
}

}  // extern "C"

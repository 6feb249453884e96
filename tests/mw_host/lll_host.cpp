// lll_host.cpp -- csrc/clrs_zz_lll_arith.h compiled for the host (g++ -ffp-contract=off), and the whole reduction of clrs_zz_lll restated around it: the threads
// of the workgroup become loops, every floating-point operation is the same function applied in the same order (the 64 lane partials of a dot product and their
// tree, the Cholesky row with i ascending, the quotients with j descending), so the device result equals this one digit for digit.  tests/lll_util.py builds
// and binds it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../clusteredlowranksolver.jl_amd/csrc/clrs_zz_lll_arith.h"

using zlll::mw;

namespace {
struct Lattice {
    int d, c, cg, nd;
    int32_t *D;                 // working digits [nd][d][c]
    std::vector<double> MU;     // limb l of mu_ij at MU[(l * d + i) * d + j]
    int32_t ord[LLL_MAX_ROWS];
    int32_t st[8];              // status, swaps, passes, launches, k
};

template <int K>
mw<K> mu_get(const Lattice &L, int i, int j) { return mwa::ld<K>(L.MU.data(), (long)L.d * L.d, (long)i * L.d + j); }

// one launch of k_zz_lll on one lattice
template <int K>
void launch(Lattice &L, int32_t *O, double delta, double eta, int max_swaps, int launch_swaps) {
    if (L.st[0] != LLL_RUNNING) return;
    const int d = L.d, c_total = L.c, cg = L.cg, nd = L.nd;
    std::vector<mw<K>> rd(LLL_MAX_ROWS + 1), r(LLL_MAX_ROWS + 1), mu(LLL_MAX_ROWS + 1), s(LLL_MAX_ROWS + 1), m(LLL_MAX_ROWS + 1);
    int32_t xd[LLL_XDIGITS * LLL_MAX_ROWS], sh[LLL_MAX_ROWS];
    int k_resume = L.st[4], swaps = L.st[1], passes = L.st[2];
    int status = LLL_RUNNING, k = 0, swaps_here = 0;
    while (status == LLL_RUNNING && k < d) {
        const bool reduce = k >= k_resume;
        if (reduce) k_resume = 0;
        int pass = 0;
        double prevmax = 0.0;
        mw<K> s_km1 = mwa::zero<K>();
        for (;;) {
            for (int j = 0; j <= k; j++) {                                                   // the Gram row
                mw<K> p[64];
                for (int lane = 0; lane < 64; lane++) p[lane] = zlll::lll_lane_partial<K>(L.D, d, c_total, nd, L.ord[k], L.ord[j], cg, lane);
                for (int off = 32; off >= 1; off >>= 1)
                    for (int l = 0; l < off; l++) p[l] = zlll::lll_tree_add<K>(p[l], p[l + off]);
                s[j] = p[0];
            }
            for (int i = 0; i < k; i++) {                                                    // the Cholesky row
                r[i] = s[i];
                mu[i] = zlll::lll_chol_mu<K>(s[i], rd[i]);
                for (int j = i + 1; j <= k; j++) {
                    if (j == k && i == k - 1) s_km1 = s[k];
                    const mw<K> mji = j < k ? mu_get<K>(L, j, i) : mu[i];
                    s[j] = zlll::lll_chol_sub<K>(s[j], mji, r[i]);
                }
            }
            int any = 0, bad = 0;
            double mx = 0.0;
            for (int j = 0; j < k; j++) {
                if (!zlll::lll_finite(mu[j].l[0])) bad = 1;
                if (zlll::lll_exceeds<K>(mu[j], eta)) any = 1;
                mx = fmax(mx, fabs(mu[j].l[0]));
            }
            if (bad) { status = LLL_ARITH; break; }
            if (!reduce || !any) break;
            if (pass >= LLL_MAX_PASSES) { status = LLL_CAP; break; }
            if (pass > 0 && !(mx < prevmax)) { status = LLL_ARITH; break; }
            prevmax = mx;
            pass++;
            passes++;
            int qbad = 0;
            for (int i = 0; i < k; i++) m[i] = mu[i];
            for (int j = k - 1; j >= 0; j--) {                                               // the quotients
                const double X = zlll::lll_quotient<K>(m[j]);
                if (zlll::lll_quotient_split(X, xd + LLL_XDIGITS * j, sh + j)) qbad = 1;
                if (X != 0.0)
                    for (int i = 0; i < j; i++) m[i] = zlll::lll_mu_sub_x<K>(m[i], mu_get<K>(L, j, i), X);
            }
            if (qbad) { status = LLL_ARITH; break; }
            int over = 0;
            for (int col = 0; col < c_total; col++) over |= zlll::lll_row_update_column(L.D, d, c_total, nd, col, L.ord, k, xd, sh);
            if (over) { status = LLL_OVERFLOW; break; }
        }
        if (status != LLL_RUNNING) break;
        int dec = 0;
        if (reduce && k > 0) {
            if (!zlll::lll_finite(s_km1.l[0])) dec = 2;
            else if (zlll::lll_lovasz_swap<K>(s_km1, rd[k - 1], delta)) dec = 1;
        }
        if (dec == 0 && !zlll::lll_diag_ok<K>(s[k])) dec = 2;
        if (dec == 2) { status = LLL_ARITH; break; }
        if (dec == 0) {
            rd[k] = s[k];
            for (int j = 0; j < k; j++) mwa::st<K>(L.MU.data(), (long)d * d, (long)k * d + j, mu[j]);
            k++;
        } else {
            const int32_t t = L.ord[k - 1];
            L.ord[k - 1] = L.ord[k];
            L.ord[k] = t;
            k--;
            swaps++;
            swaps_here++;
            if (swaps >= max_swaps) { status = LLL_CAP; break; }
            if (swaps_here >= launch_swaps) break;
        }
    }
    if (status == LLL_RUNNING && k >= d) status = LLL_OK;
    if (status == LLL_OK)
        for (int sp = 0; sp < nd; sp++)
            for (int i = 0; i < d; i++)
                std::memcpy(O + ((size_t)sp * d + i) * c_total, L.D + ((size_t)sp * d + L.ord[i]) * c_total, (size_t)c_total * sizeof(int32_t));
    L.st[1] = swaps;
    L.st[2] = passes;
    L.st[3] += 1;
    L.st[4] = k;
    L.st[0] = status;
}
}  // namespace

extern "C" {

// [LLL_MAX_ROWS, LLL_MAX_COLS, LLL_MAX_ND, LLL_MAX_PASSES, LLL_XDIGITS, conversion digits at 2, 4, 6 limbs]
int lll_constants_host(int32_t *out) {
    const int32_t v[8] = {LLL_MAX_ROWS, LLL_MAX_COLS, LLL_MAX_ND, LLL_MAX_PASSES, LLL_XDIGITS, LLL_CONV_DIGITS(2), LLL_CONV_DIGITS(4), LLL_CONV_DIGITS(6)};
    std::memcpy(out, v, sizeof v);
    return 0;
}

// the K-limb image of `count` entries given as [nd][count] digits: limbs[l * count + e]
int lll_entry_host(int limbs, int nd, int count, const int32_t *digits, double *out) {
    for (int e = 0; e < count; e++) {
        if (limbs == 2) mwa::st<2>(out, count, e, zlll::lll_entry_to_mw<2>(digits + e, (size_t)count, nd));
        else if (limbs == 4) mwa::st<4>(out, count, e, zlll::lll_entry_to_mw<4>(digits + e, (size_t)count, nd));
        else if (limbs == 6) mwa::st<6>(out, count, e, zlll::lll_entry_to_mw<6>(digits + e, (size_t)count, nd));
        else return -1;
    }
    return 0;
}

// per value: X = rint(mu) and its split; xd [count][4], sh [count], bad [count]
int lll_split_host(int count, const double *mu, double *X, int32_t *xd, int32_t *sh, int32_t *bad) {
    for (int e = 0; e < count; e++) {
        mw<2> v = mwa::from_double<2>(mu[e]);
        X[e] = zlll::lll_quotient<2>(v);
        bad[e] = zlll::lll_quotient_split(X[e], xd + LLL_XDIGITS * e, sh + e);
    }
    return 0;
}

// the row operation b_k <- b_k - sum_{j < k} X_j b_j on digits D [nd][d][c] in place (the order table is the identity); returns the columns that overflowed
int lll_update_host(int d, int c, int nd, int32_t *D, int k, const double *X) {
    int32_t xd[LLL_XDIGITS * LLL_MAX_ROWS], sh[LLL_MAX_ROWS], ord[LLL_MAX_ROWS];
    for (int i = 0; i < LLL_MAX_ROWS; i++) ord[i] = i;
    for (int j = 0; j < k; j++)
        if (zlll::lll_quotient_split(X[j], xd + LLL_XDIGITS * j, sh + j)) return -1;
    int over = 0;
    for (int col = 0; col < c; col++) over += zlll::lll_row_update_column(D, d, c, nd, col, ord, k, xd, sh);
    return over;
}

// clrs_zz_lll on the host: the same arguments, plus the exchanges a launch may take.  No validation: the caller passes what clrs_zz_lll accepts.
int lll_reduce_host(int nb, const int32_t *rows, const int32_t *cols, const int32_t *cols_gram, int nd, const int32_t *in_digits, int32_t *out_digits, double delta,
                    double eta, int limbs, int max_swaps, int launch_swaps, int32_t *info) {
    if (limbs != 2 && limbs != 4 && limbs != 6) return -1;
    size_t off = 0;
    for (int b = 0; b < nb; b++) {
        const size_t count = (size_t)nd * rows[b] * cols[b];
        std::vector<int32_t> W(in_digits + off, in_digits + off + count), O(count, 0);
        Lattice L;
        L.d = rows[b]; L.c = cols[b]; L.cg = cols_gram[b]; L.nd = nd;
        L.D = W.data();
        L.MU.assign((size_t)limbs * L.d * L.d + 1, 0.0);
        for (int i = 0; i < LLL_MAX_ROWS; i++) L.ord[i] = i;
        std::memset(L.st, 0, sizeof L.st);
        L.st[0] = L.d > 0 ? LLL_RUNNING : LLL_OK;
        const long long max_launches = (long long)max_swaps / launch_swaps + 2;
        for (long long it = 0; it < max_launches && L.st[0] == LLL_RUNNING; it++) {
            if (limbs == 2) launch<2>(L, O.data(), delta, eta, max_swaps, launch_swaps);
            else if (limbs == 4) launch<4>(L, O.data(), delta, eta, max_swaps, launch_swaps);
            else launch<6>(L, O.data(), delta, eta, max_swaps, launch_swaps);
        }
        if (L.st[0] == LLL_RUNNING) L.st[0] = LLL_CAP;
        if (L.st[0] == LLL_OK && count) std::memcpy(out_digits + off, O.data(), count * sizeof(int32_t));
        std::memcpy(info + (size_t)b * 8, L.st, sizeof L.st);
        off += count;
    }
    return 0;
}
}

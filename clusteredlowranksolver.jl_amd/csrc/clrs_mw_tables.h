// clrs_mw_tables.h -- host only, no HIP: everything a multi-word context derives from the caller's description by plain arithmetic, before a
// device is involved (clrs_mw_create_opts, clrs_mw.hip; tests/test_mw_tables_cpu.py through tests/mw_host/mw_tables_host.cpp).
//
// mw_build_tables redoes the de-duplication of the sampled vectors (precompute_matrices_bilinear_pairings, src/solver.jl:985-1059) into ONE table
// of expanded unique vectors per PSD block -- a vector of sub-block r is stored with its delta entries at rows r*delta.. and zeros elsewhere,
// duplicates removed by exact equality as the reference does (src/tools.jl:128-145) -- so that both pairing matrices of a block are plain symmetric
// products V^T X^-1 V and V^T Y V, and the reference's pointers_left / pointers_right dictionaries become two integers per term.
// mw_cut_digits is the one digit cutter of the static operands of the exact-product kernels (clrs_mw_exact.hip.h).
#ifndef CLRS_MW_TABLES_H
#define CLRS_MW_TABLES_H

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_mw_slices.h"
#include "clrs_mw_types.h"

// What MwDev's table pointers point to (clrs_mw_kernels.hip.h names every array), the block and cluster records with every field that depends on
// neither LDS nor the limb count (MwBlk::inv, MwClu::lds stay 0), and the sizes the buffers are cut from.  Data arrays are planar, DK planes.
struct MwTables {
    int J = 0, N = 0, NB = 0, DK = 1;
    mwi64 T = 0, D = 0;                                      // low-rank terms, dense entries
    mwi64 xlen = 0, Slen = 0, xylen = 0, xrdlen = 0;         // stacked constraint rows, S layout, xy layout, reciprocal diagonals of the X blocks
    mwi64 zlen = 0, glen = 0, sdlen = 0, wlen = 0;           // Z / T, GX / GY, Sd, W scratch (0 when no block needs them)
    mwi64 Vp = 1, dAp = 1, lamp = 1, Bp = 1;                 // plane lengths of V, dA, st_lam, B (at least 1)
    std::vector<MwBlk> blk;
    std::vector<MwClu> clu;
    std::vector<int> lr_list, dn_list;
    std::vector<double> V, dA, st_lam, B;
    std::vector<int> vrow, tptr, st_a, st_b, st_orig, st_p, st_war, st_wac, st_trl, st_trd, st_flag, ay_a, ay_b, ay_blk;
    std::vector<int> dmap, dense_p, drow_ptr, drow_blk, drow_en;
    int maxU = 0, maxP = 0, maxn = 0, maxn_dense = 0, maxTb = 0, maxcnt = 0, dn_big = 0;
    int sa_lanes = 1;                                        // lanes per entry of k_mw_saccum: 1, 2 or 4 by the largest block count of a cluster
    int n_one_term = 0, n_many_term = 0;                     // clusters whose S_j goes through k_mw_saccum_one / through the general k_mw_saccum
    double cnt_mul = 0, cnt_factor = 0, cnt_solve = 0;       // algorithmic multi-word multiply-adds of one assembly / factorisation / solve
};

// 0, or CLRS_ERR_INVALID with the message in err (the first violation in the order of the checks below)
inline int mw_build_tables(const clrs_sdp_desc *d, int data_limbs, MwTables &o, std::string &err) {
    typedef mwi64 i64;
#define MWT_FAIL(msg) do { err = (msg); return CLRS_ERR_INVALID; } while (0)
    o = MwTables();
    const int DK = o.DK = data_limbs;
    const int J = o.J = d->n_clusters, N = o.N = d->n_free, NB = o.NB = d->n_blocks;
    if (J <= 0 || N < 0 || NB < 0) MWT_FAIL("bad sizes");
    // ---- clusters ----
    o.clu.resize(J);
    i64 xlen = 0, Slen = 0;
    for (int j = 0; j < J; j++) {
        MwClu &q = o.clu[j];
        q.P = d->cluster_P[j];
        if (q.P <= 0) MWT_FAIL("cluster without constraints");
        q.coff = xlen; q.Soff = Slen; q.b0 = NB; q.b1 = 0;
        xlen += q.P; Slen += (i64)q.P * q.P;
        o.maxP = std::max(o.maxP, q.P);
    }
    o.xlen = xlen; o.Slen = Slen;
    // ---- blocks, unique expanded vectors, term tables ----
    o.blk.resize(NB);
    const i64 T = o.T = NB ? d->term_ptr[NB] : 0, D = o.D = NB ? d->dense_ptr[NB] : 0;
    // planes of the description's data arrays (data_limbs planes each)
    const i64 vec_plane = T ? d->term_vec_ptr[T] : 0, dA_plane = D ? d->dense_A_ptr[D] : 0;
    const size_t T1 = (size_t)std::max<i64>(T, 1);
    o.st_a.resize(T1); o.st_b.resize(T1); o.ay_a.assign(T1, 0); o.ay_b.assign(T1, 0); o.ay_blk.assign(T1, -1);
    o.st_lam.resize(T1 * DK);
    // for the interior-point iteration around the path (clrs_mw_ipm.hip.h), sorted term order: original term, vs at sub-block r / ws at
    // sub-block s (compute_weighted_A!, src/solver.jl:1433-1459), ws at r / vs at s (trace_A, :1334-1341), and the flags s <= r, r != s
    o.st_orig.resize(T1); o.st_war.resize(T1); o.st_wac.resize(T1); o.st_trl.resize(T1); o.st_trd.resize(T1); o.st_flag.resize(T1); o.st_p.resize(T1);
    std::vector<std::tuple<i64, int, int>> drow_pairs;       // (stacked row, block, entry) of every dense matrix
    std::vector<std::vector<double>> hVl(DK), hdAl(DK);     // per limb
    i64 xyoff = 0, rdoff = 0, zoff = 0, goff = 0, sdoff = 0, woff = 0;
    for (int b = 0; b < NB; b++) {
        MwBlk &k = o.blk[b];
        std::memset(&k, 0, sizeof(k));
        k.j = d->block_cluster[b];
        if (k.j < 0 || k.j >= J || (b > 0 && k.j < o.blk[b - 1].j)) MWT_FAIL("block_cluster must be non-decreasing and within range");
        const int m = d->block_m[b];
        k.delta = d->block_delta[b];
        k.n = m * k.delta;
        k.kind = d->block_kind[b];
        k.m = m;
        k.P = o.clu[k.j].P;
        if (k.n <= 0 || (k.kind != 0 && m != 1)) MWT_FAIL("bad block shape");
        k.xyoff = xyoff; xyoff += (i64)k.n * k.n;
        k.rd_off = rdoff; rdoff += k.n;
        o.clu[k.j].b0 = std::min(o.clu[k.j].b0, b);
        o.clu[k.j].b1 = std::max(o.clu[k.j].b1, b + 1);
        o.maxn = std::max(o.maxn, k.n);
        if (k.kind != 0) o.maxn_dense = std::max(o.maxn_dense, k.n);
        const int P = k.P, n = k.n, dl = k.delta;
        if (k.kind == 0) {
            o.lr_list.push_back(b);
            const i64 t0 = d->term_ptr[b], t1 = d->term_ptr[b + 1];
            k.t0 = t0;
            o.maxTb = std::max(o.maxTb, (int)(t1 - t0));
            // unique expanded vectors: (sub-block, delta values), exact equality, first occurrence wins
            std::vector<std::pair<int, const double *>> uniq;      // (sub-block, pointer to limb 0 of the vector inside term_vs / term_ws)
            auto find_or_add = [&](int r, const double *v) -> int {
                for (size_t u = 0; u < uniq.size(); u++) {
                    if (uniq[u].first != r) continue;
                    bool eq = true;
                    for (int l = 0; l < DK && eq; l++)
                        for (int i = 0; i < dl && eq; i++) eq = uniq[u].second[(i64)l * vec_plane + i] == v[(i64)l * vec_plane + i];
                    if (eq) return (int)u;
                }
                uniq.push_back({r, v});
                return (int)uniq.size() - 1;
            };
            std::map<std::tuple<int, int, int, int>, i64> index;
            for (i64 t = t0; t < t1; t++) {
                if (d->term_p[t] < 0 || d->term_p[t] >= P || d->term_r[t] < 0 || d->term_r[t] >= m || d->term_s[t] < 0 || d->term_s[t] >= m)
                    MWT_FAIL("term index out of range");
                if (d->term_vec_ptr[t + 1] - d->term_vec_ptr[t] != dl) MWT_FAIL("term vectors must have delta entries");
                index[std::make_tuple(d->term_p[t], d->term_r[t], d->term_s[t], d->term_rank[t])] = t;
            }
            // R(t): vs of the term at sub-block r; Lself(t): ws of the term at sub-block r   (rightvecs[r] / leftvecs[r], src/solver.jl:1011, 1032)
            std::vector<int> Rt(t1 - t0), Ls(t1 - t0), Cs(t1 - t0), Ds(t1 - t0);
            std::vector<i64> partner(t1 - t0);
            for (i64 t = t0; t < t1; t++) {
                Rt[t - t0] = find_or_add(d->term_r[t], d->term_vs + d->term_vec_ptr[t]);
                Ls[t - t0] = find_or_add(d->term_r[t], d->term_ws + d->term_vec_ptr[t]);
                Cs[t - t0] = find_or_add(d->term_s[t], d->term_ws + d->term_vec_ptr[t]);
                Ds[t - t0] = find_or_add(d->term_s[t], d->term_vs + d->term_vec_ptr[t]);
                auto it = index.find(std::make_tuple(d->term_p[t], d->term_s[t], d->term_r[t], d->term_rank[t]));
                if (it == index.end()) MWT_FAIL("term without transposed partner: A[r,s][p] must equal A[s,r][p]^T");
                partner[t - t0] = it->second;
            }
            k.U = (int)uniq.size();
            o.maxU = std::max(o.maxU, k.U);
            k.v_off = (i64)hVl[0].size();
            k.vrow_off = (i64)o.vrow.size();
            for (int l = 0; l < DK; l++) hVl[l].resize(hVl[l].size() + (size_t)n * k.U, 0.0);
            for (int u = 0; u < k.U; u++) {
                o.vrow.push_back(uniq[u].first * dl);
                for (int l = 0; l < DK; l++)
                    for (int i = 0; i < dl; i++) hVl[l][k.v_off + (i64)u * n + uniq[u].first * dl + i] = uniq[u].second[(i64)l * vec_plane + i];
            }
            k.z_off = zoff; zoff += (i64)n * k.U;
            k.g_off = goff; goff += (i64)k.U * k.U;
            // terms sorted by constraint (stable), CSR over p
            std::vector<i64> order(t1 - t0);
            for (i64 t = t0; t < t1; t++) order[t - t0] = t;
            std::stable_sort(order.begin(), order.end(), [&](i64 a, i64 b2) { return d->term_p[a] < d->term_p[b2]; });
            k.tptr_off = (i64)o.tptr.size();
            o.tptr.resize(o.tptr.size() + P + 1, 0);
            int *tp = o.tptr.data() + k.tptr_off;
            for (i64 i = 0; i < t1 - t0; i++) tp[d->term_p[order[i]] + 1]++;
            tp[0] = (int)t0;
            for (int p = 0; p < P; p++) tp[p + 1] += tp[p];
            for (i64 i = 0; i < t1 - t0; i++) {
                const i64 t = order[i];
                o.st_a[t0 + i] = Ls[partner[t - t0] - t0];      // pointers_left[s][(r,p,k)] = ws of A[s,r][p]
                o.st_b[t0 + i] = Rt[t - t0];                    // pointers_right[r][(s,p,k)] = vs of A[r,s][p]
                for (int l = 0; l < DK; l++) o.st_lam[(size_t)l * T1 + t0 + i] = d->term_lambda[(i64)l * T + t];
                o.st_orig[t0 + i] = (int)t;
                o.st_p[t0 + i] = d->term_p[t];
                o.st_war[t0 + i] = Rt[t - t0]; o.st_wac[t0 + i] = Cs[t - t0];
                o.st_trl[t0 + i] = Ls[t - t0]; o.st_trd[t0 + i] = Ds[t - t0];
                o.st_flag[t0 + i] = (d->term_s[t] <= d->term_r[t] ? 1 : 0) | (d->term_s[t] != d->term_r[t] ? 2 : 0);
            }
            for (i64 t = t0; t < t1; t++) {                    // A_Y[r,s][idx] = bpY[r,s][left_r(s,p,k), right_s(r,p,k)]  (src/solver.jl:1162)
                o.ay_blk[t] = b;
                o.ay_a[t] = Ls[t - t0];
                o.ay_b[t] = Rt[partner[t - t0] - t0];
            }
            // algorithmic multi-word multiply-adds of the assembly of this block: T = Y V, Z = L^-1 V, GX, GY (lower triangles), S
            o.cnt_mul += (double)n * dl * k.U + 0.5 * (double)n * n * k.U + 0.5 * (double)k.U * k.U * (n + dl);
            for (int p = 0; p < P; p++)
                for (int q2 = p; q2 < P; q2++) o.cnt_mul += (double)(tp[p + 1] - tp[p]) * (tp[q2 + 1] - tp[q2]);
        } else {
            o.dn_list.push_back(b);
            const i64 d0 = d->dense_ptr[b], d1 = d->dense_ptr[b + 1];
            k.cnt = (int)(d1 - d0);
            k.d0 = d0;
            k.a_off = (i64)hdAl[0].size();
            k.dmap_off = (i64)o.dmap.size();
            o.dmap.resize(o.dmap.size() + P, -1);
            for (i64 e = d0; e < d1; e++) {
                const int p = d->dense_p[e];
                if (p < 0 || p >= P) MWT_FAIL("dense constraint index out of range");
                if (d->dense_A_ptr[e + 1] - d->dense_A_ptr[e] != (i64)n * n) MWT_FAIL("dense matrix must have n*n entries");
                for (int l = 0; l < DK; l++) {          // symmetric, as the reference's constructor makes them (src/interface.jl:1010-1017)
                    const double *Ae = d->dense_A + (i64)l * dA_plane + d->dense_A_ptr[e];
                    for (int cc = 0; cc < n; cc++)
                        for (int rr = cc + 1; rr < n; rr++)
                            if (Ae[rr + (i64)cc * n] != Ae[cc + (i64)rr * n]) MWT_FAIL("dense constraint matrices must be symmetric");
                }
                o.dmap[k.dmap_off + p] = (int)(e - d0);
                drow_pairs.push_back(std::make_tuple(o.clu[k.j].coff + p, b, (int)(e - d0)));
                for (int l = 0; l < DK; l++)
                    hdAl[l].insert(hdAl[l].end(), d->dense_A + (i64)l * dA_plane + d->dense_A_ptr[e], d->dense_A + (i64)l * dA_plane + d->dense_A_ptr[e + 1]);
            }
            k.sd_off = sdoff; sdoff += (i64)k.cnt * k.cnt;
            k.w_off = woff; woff += (i64)k.cnt * n * n;
            o.cnt_mul += (double)k.cnt * (2.0 * n * n * n + 0.5 * (double)k.cnt * n * n);
            o.maxcnt = std::max(o.maxcnt, k.cnt);
            if (n > 1) o.dn_big = 1;
        }
    }
    o.xylen = xyoff; o.xrdlen = rdoff; o.zlen = zoff; o.glen = goff; o.sdlen = sdoff; o.wlen = woff;
    for (int j = 0; j < J; j++)
        if (o.clu[j].b0 > o.clu[j].b1) { o.clu[j].b0 = o.clu[j].b1 = 0; }
    {
        int mostb = 1;
        for (int j = 0; j < J; j++) mostb = std::max(mostb, o.clu[j].b1 - o.clu[j].b0);
        o.sa_lanes = mostb >= 3 ? 4 : mostb;
        // (one lane per entry when the launch fills the chip anyway was tried at 2048 clusters: 30 M wave instructions instead of 90 M, and
        // 390 us instead of 245: the chains of dependent loads of a cluster's blocks, one after the other, cost more than the idle lanes)
        // clusters with at most four blocks and at most one low-rank term per (constraint, block): k_mw_saccum_one
        for (int j = 0; j < J; j++) {
            MwClu &cl = o.clu[j];
            bool one = J >= 32 && cl.b1 - cl.b0 >= 1 && cl.b1 - cl.b0 <= 4;      // (with a few clusters the launch is latency bound and a lane per block wins: 6.9 against 9.1 us on the named problem)
            for (int b = cl.b0; b < cl.b1 && one; b++) {
                const MwBlk &k = o.blk[b];
                if (k.kind != 0) continue;
                const int *tp = o.tptr.data() + k.tptr_off;
                for (int p = 0; p < cl.P && one; p++) one = tp[p + 1] - tp[p] <= 1;
            }
            cl.one_term = one ? 1 : 0;
            (one ? o.n_one_term : o.n_many_term)++;
        }
    }
    for (int j = 0; j < J; j++) {
        const double P = o.clu[j].P;
        o.cnt_factor += P * P * P / 6.0 + 0.5 * P * P * N + 0.5 * P * (double)N * N;
        o.cnt_solve += P * P + 2.0 * P * N;
    }
    o.cnt_factor += (double)N * N * N / 6.0;
    o.cnt_solve += (double)N * N;
    // ---- the data planes side by side; the dense entries per stacked constraint row ----
    o.Vp = std::max<i64>((i64)hVl[0].size(), 1); o.dAp = std::max<i64>((i64)hdAl[0].size(), 1); o.lamp = std::max<i64>(T, 1);
    o.V.assign((size_t)o.Vp * DK, 0.0);
    o.dA.assign((size_t)o.dAp * DK, 0.0);
    for (int l = 0; l < DK; l++) {
        std::copy(hVl[l].begin(), hVl[l].end(), o.V.begin() + (size_t)l * o.Vp);
        std::copy(hdAl[l].begin(), hdAl[l].end(), o.dA.begin() + (size_t)l * o.dAp);
    }
    o.dense_p.assign(d->dense_p, d->dense_p + D);
    std::sort(drow_pairs.begin(), drow_pairs.end());
    o.drow_ptr.assign((size_t)xlen + 1, 0);
    for (auto &t : drow_pairs) o.drow_ptr[(size_t)std::get<0>(t) + 1]++;
    for (i64 g = 0; g < xlen; g++) o.drow_ptr[(size_t)g + 1] += o.drow_ptr[(size_t)g];
    for (auto &t : drow_pairs) { o.drow_blk.push_back(std::get<1>(t)); o.drow_en.push_back(std::get<2>(t)); }
    // B arrives per cluster (P_j x N column-major, concatenated); the kernels read one stacked xlen x N matrix
    const i64 Bp = xlen * (i64)N;
    o.Bp = std::max<i64>(Bp, 1);
    o.B.assign((size_t)o.Bp * DK, 0.0);
    for (int l = 0; l < DK; l++) {
        i64 off = 0;
        for (int j = 0; j < J; j++) {
            const int P = o.clu[j].P;
            for (int a = 0; a < N; a++)
                for (int r = 0; r < P; r++) o.B[(size_t)l * o.Bp + o.clu[j].coff + r + (i64)a * xlen] = d->B[(i64)l * Bp + off + r + (i64)a * P];
            off += (i64)P * N;
        }
    }
    return 0;
#undef MWT_FAIL
}

// The digits of the double-double x0 + x1 relative to the window exponent e (|x| < 2^(e-2), mwk::mws_exponent): put(s, digit) for s = 0 .. S-1, every
// digit an integer of MWS_BETA bits (exact in fp32), x = 2^e sum_s digit[s] 2^-(s+1) MWS_BETA up to what lies below the last slice.  Slice by slice: the
// head's rounding to the slice's grid by add-and-subtract of 1.5 * 2^52 * grid, then one two_sum brings the tail up.  (Not mwk::mws_slice, which rounds
// limb by limb and sweeps carries afterwards: the two may choose different digits for the same value, and the kernels' slice counts come from these.)
template <class PUT>
inline void mw_cut_digits(double x0, double x1, int e, int S, PUT &&put) {
    double r0 = std::ldexp(x0, -e), r1 = std::ldexp(x1, -e);
    for (int s = 0; s < S; s++) {
        const double g = std::ldexp(1.0, -(s + 1) * MWS_BETA), C = 0x1.8p52 * g;
        volatile double tv = r0 + C;               // (no contraction or reassociation of the rounding trick on the host)
        const double t = tv - C;
        put(s, (float)(t * std::ldexp(1.0, (s + 1) * MWS_BETA)));
        r0 -= t;
        double sm, er;
        mwa::two_sum(r0, r1, sm, er);
        r0 = sm; r1 = er;
    }
}

#endif

// The stages of clrs_ctx_create (included by clrs_hip.hip, which runs them in the order of `CTX_STAGES` at the end of this file).
// Every stage returns 0 or the code of fail(...) / HIPCHECK; none of them cleans up: clrs_ctx_create owns the context and destroys it on
// the way out of a failed stage.  What lives only while the context is being created is in CtxBuild; inside it, one struct per assembly
// kernel holds exactly what that kernel's selection pass hands to its plan.
#define CLRS_RET(call) do { if (int rc_ = (call)) return rc_; } while (0)
struct CtxBuild {
    std::vector<int> ridx, lidx;                                     // per term: its vector among the unique ones of its sub-block row
    std::vector<i64> partner;                                        // per term: its transposed partner
    std::vector<std::vector<std::vector<i64>>> uniqR, uniqL;         // [block][r]: the terms that carry the unique vectors
    std::vector<int> cb;                                             // blocks of cluster j: [cb[j], cb[j + 1])
    i64 tyo = 0, go = 0, tto = 0, sdo = 0;                           // arena lengths (the solve arena's: c->solve_arena_len)
    std::vector<double> h_static, s_tlam;                            // the static arena; lambda of the sorted terms
    std::vector<i64> h_ayidx, perm;                                  // per term: its place in G for A_Y; the terms of a block sorted by constraint
    std::vector<std::vector<int>> h_tptr;                            // per block: CSR over the constraints into its sorted terms
    std::vector<int> s_tL, s_tR;                                     // per sorted term: left / right vector
    int *d_tL = nullptr, *d_tR = nullptr;                            // ... and their device copies
    double *d_tlam = nullptr;
    struct { std::vector<W3Block> blk; std::vector<int> cl_blk0, ay; std::vector<double> lam, vop; } w5;      // k_cluster_assemble_w5
    struct { std::vector<W3Block> blk; std::vector<W3Dense> dense; std::vector<int> cl_blk0, pmap, ay; std::vector<double> lam, vop; int nu = 0; } w4;      // k_cluster_assemble_w4
    struct {                          // k_cluster_assemble_w1 (wave per block)
        std::vector<WCluster> cl; std::vector<WBlock> bl; std::vector<int> pmap, ay; std::vector<double> lam;
        std::vector<size_t> ioff, cl_first;      // per WBlock: offset of its pmap / lam / ay entries in the packed arrays; per WCluster: its first WBlock
        int ut = 0, nwaves = 8, maxblocks = 0;
        size_t cluster_doubles = 0;
    } w1;
    struct {                          // k_cluster_assemble_w2 / _w3 (cluster per wave)
        std::vector<W2Cluster> cl; std::vector<W2Block> bl; std::vector<int> pmap, ay; std::vector<double> lam;
        std::vector<size_t> cl_pm, boff, bl_cl;
        int ut = 0;
    } w2;
    struct { std::vector<FCluster> cl; std::vector<SSlabSum> sum; std::vector<FBlock> bl; int nmax = 0; size_t lds = 0; } fu;      // k_cluster_assemble, whole clusters or split by blocks
};

static int raise_lds_limit(const void *kernel, size_t bytes) {      // dynamic LDS beyond 64 KiB has to be asked for
    if (bytes > 64 * 1024) HIPCHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
static int lds_square(int n) { const int n16 = (n + 15) & ~15; return (n16 + 2) * n16 + n16; }   // matrix + dinv, in doubles
static int cu_count(const clrs_ctx *c) {
    hipDeviceProp_t prop;
    return hipGetDeviceProperties(&prop, c->device) == hipSuccess ? prop.multiProcessorCount : 256;
}
static int ensure_stamps(clrs_ctx *c) {
    if (c->ftables.stamps) return 0;
    std::vector<unsigned long long> z(64, 0ull);
    return upload(c, z, &c->ftables.stamps);
}
// vectors (columns of V, leading dimension ld) in MFMA-operand order: `ntiles` tiles of 16 columns, `nq` groups of four rows (4: 16 rows, 8: 32 rows);
// entries beyond nrow x ncol keep the zero they have
static void pack_vop(const double *V, i64 ld, int nrow, int ncol, double *dst, int ntiles, int nq) {
    for (int t = 0; t < ntiles; t++)
        for (int q = 0; q < nq; q++)
            for (int ln = 0; ln < 64; ln++) {
                const int row = 4 * q + (ln >> 4), col = 16 * t + (ln & 15);
                if (row < nrow && col < ncol) dst[((t * (nq / 2) + (q >> 1)) * 64 + ln) * 2 + (q & 1)] = V[row + (i64)col * ld];
            }
}

static int ctx_device_objects(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    HIPCHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const void *gemm128[] = {(const void *)k_gemm_f64_t<128, 128, 0, 0>, (const void *)k_gemm_f64_t<128, 128, 0, 1>, (const void *)k_gemm_f64_t<128, 128, 1, 0>,
                             (const void *)k_gemm_f64_t<128, 128, 1, 1>};
    for (const void *k : gemm128) HIPCHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_lds_bytes(128, 128)));
    for (int i = 0; i < 10; i++) HIPCHECK(hipEventCreate(&c->ev[i]));
    return 0;
}

static int ctx_sizes(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &) {
    c->J = d->n_clusters; c->N = d->n_free; c->NB = d->n_blocks;
    if (c->J < 0 || c->N < 0 || c->NB < 0) return fail(CLRS_ERR_INVALID, "negative sizes");
    const int J = c->J;
    c->P.assign(d->cluster_P, d->cluster_P + J);
    c->coff.assign(J + 1, 0); c->Soff.assign(J + 1, 0);
    for (int j = 0; j < J; j++) {
        if (c->P[j] <= 0) return fail(CLRS_ERR_INVALID, "cluster with no constraints");
        c->coff[j + 1] = c->coff[j] + c->P[j];
        c->Soff[j + 1] = c->Soff[j] + (i64)c->P[j] * c->P[j];
    }
    c->xlen = c->coff[J]; c->Slen = c->Soff[J];
    c->T = d->term_ptr[c->NB]; c->D = d->dense_ptr[c->NB];
    c->cluster_fused.assign(J, 0);
    return 0;
}

// ---- blocks, de-duplication of the sampled vectors (src/solver.jl:985-1059) ----
static int ctx_blocks(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const int J = c->J, NB = c->NB;
    const i64 T = c->T;
    c->blk.resize(NB);
    B.ridx.resize(T); B.lidx.resize(T); B.partner.assign(T, -1);
    B.uniqR.resize(NB); B.uniqL.resize(NB); B.cb.assign(J + 1, 0);
    i64 xyoff = 0;
    int prevj = 0;
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        k.j = d->block_cluster[b]; k.m = d->block_m[b]; k.delta = d->block_delta[b]; k.kind = d->block_kind[b];
        k.n = k.m * k.delta;
        if (k.j < prevj || k.j >= J || k.m <= 0 || k.delta <= 0) return fail(CLRS_ERR_INVALID, "bad block description (clusters must be listed in order)");
        prevj = k.j;
        B.cb[k.j + 1]++;
        k.xyoff = xyoff; xyoff += (i64)k.n * k.n;
        k.t0 = d->term_ptr[b]; k.t1 = d->term_ptr[b + 1]; k.d0 = d->dense_ptr[b]; k.d1 = d->dense_ptr[b + 1];
        c->host_U_off.push_back((i64)c->host_UR.size());
        if (k.kind != 0) {
            if (k.m != 1) return fail(CLRS_ERR_INVALID, "dense blocks need m == 1");
            k.cnt = (int)(k.d1 - k.d0);
            for (i64 e = k.d0; e < k.d1; e++)
                if (d->dense_p[e] < 0 || d->dense_p[e] >= c->P[k.j]) return fail(CLRS_ERR_INVALID, "dense constraint index out of range");
            continue;
        }
        const int m = k.m, dl = k.delta;
        k.UR.assign(m, 0); k.UL.assign(m, 0); k.offR.assign(m + 1, 0); k.offL.assign(m + 1, 0);
        B.uniqR[b].resize(m); B.uniqL[b].resize(m);
        for (i64 t = k.t0; t < k.t1; t++) {
            int r = d->term_r[t], s = d->term_s[t], p = d->term_p[t];
            if (r < 0 || r >= m || s < 0 || s >= m || p < 0 || p >= c->P[k.j] || d->term_vec_ptr[t + 1] - d->term_vec_ptr[t] != dl)
                return fail(CLRS_ERR_INVALID, "bad term description");
            const double *v = d->term_vs + d->term_vec_ptr[t], *w = d->term_ws + d->term_vec_ptr[t];
            std::vector<i64> &uR = B.uniqR[b][r], &uL = B.uniqL[b][r];
            int f = -1;
            for (size_t u = 0; u < uR.size(); u++) if (vec_eq(d->term_vs + d->term_vec_ptr[uR[u]], v, dl)) { f = (int)u; break; }
            if (f < 0) { f = (int)uR.size(); uR.push_back(t); }
            B.ridx[t] = f;
            f = -1;
            for (size_t u = 0; u < uL.size(); u++) if (vec_eq(d->term_ws + d->term_vec_ptr[uL[u]], w, dl)) { f = (int)u; break; }
            if (f < 0) { f = (int)uL.size(); uL.push_back(t); }
            B.lidx[t] = f;
        }
        {   // transposed partner (p, s, r, rank) of every term; required by the convention src/solver.jl:1009
            std::map<std::array<int, 4>, i64> index;
            for (i64 t = k.t0; t < k.t1; t++) index[{d->term_p[t], d->term_r[t], d->term_s[t], d->term_rank[t]}] = t;
            for (i64 t = k.t0; t < k.t1; t++) {
                auto it = index.find({d->term_p[t], d->term_s[t], d->term_r[t], d->term_rank[t]});
                if (it == index.end()) return fail(CLRS_ERR_INVALID, "term without transposed partner: A[r,s][p] must equal A[s,r][p]^T");
                B.partner[t] = it->second;
            }
        }
        k.sym = true;
        for (int r = 0; r < m; r++) {
            k.UR[r] = (int)B.uniqR[b][r].size(); k.UL[r] = (int)B.uniqL[b][r].size();
            k.offR[r + 1] = k.offR[r] + k.UR[r]; k.offL[r + 1] = k.offL[r] + k.UL[r];
            c->host_UR.push_back(k.UR[r]); c->host_UL.push_back(k.UL[r]);
            if (k.UR[r] != k.UL[r]) k.sym = false;
            else
                for (int u = 0; u < k.UR[r] && k.sym; u++)
                    if (!vec_eq(d->term_vs + d->term_vec_ptr[B.uniqR[b][r][u]], d->term_ws + d->term_vec_ptr[B.uniqL[b][r][u]], dl)) k.sym = false;
        }
        k.URt = k.offR[m]; k.ULt = k.offL[m];
    }
    c->xylen = xyoff;
    for (int j = 0; j < J; j++) B.cb[j + 1] += B.cb[j];
    return 0;
}

// ---- arena layout ----
// "solve" arena: per low-rank block ZR (n x URt) [+ ZL (n x ULt) if not symmetric]; per dense block W (n x n*cnt).
// the static arena has the identical layout and holds the expanded vectors / the dense A stacks.
static int ctx_arenas(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const int NB = c->NB;
    i64 so = 0;
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        if (k.kind == 0) {
            k.zr_off = so; so += (i64)k.n * k.URt;
            if (k.sym) k.zl_off = k.zr_off; else { k.zl_off = so; so += (i64)k.n * k.ULt; }
            k.ty_off = B.tyo; B.tyo += (i64)k.n * k.URt;
            k.g_off = B.go; B.go += 2 * (i64)k.ULt * k.URt;
        } else {
            k.w_off = so; so += (i64)k.n * k.n * k.cnt;
            k.tt_off = B.tto; B.tto += (i64)k.n * k.n * k.cnt;
            k.sd_off = B.sdo; B.sdo += (i64)k.cnt * k.cnt;
        }
    }
    c->solve_arena_len = so;
    std::vector<double> &h_static = B.h_static;
    h_static.assign((size_t)std::max<i64>(so, 1), 0.0);
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        if (k.kind == 0) {
            const int dl = k.delta, n = k.n;
            for (int r = 0; r < k.m; r++) {
                for (int u = 0; u < k.UR[r]; u++) {
                    const double *v = d->term_vs + d->term_vec_ptr[B.uniqR[b][r][u]];
                    double *dst = h_static.data() + k.zr_off + (i64)(k.offR[r] + u) * n + (i64)r * dl;
                    std::memcpy(dst, v, sizeof(double) * dl);
                }
                if (!k.sym)
                    for (int u = 0; u < k.UL[r]; u++) {
                        const double *w = d->term_ws + d->term_vec_ptr[B.uniqL[b][r][u]];
                        double *dst = h_static.data() + k.zl_off + (i64)(k.offL[r] + u) * n + (i64)r * dl;
                        std::memcpy(dst, w, sizeof(double) * dl);
                    }
            }
        } else {
            for (i64 e = k.d0; e < k.d1; e++) {
                if (d->dense_A_ptr[e + 1] - d->dense_A_ptr[e] != (i64)k.n * k.n) return fail(CLRS_ERR_INVALID, "dense matrix has the wrong size");
                {   // the dense branch forms <A_i, X^-1 A_k Y> from lower tiles and transposed stores (k_dense_T32, pairing_tri): A_p must be
                    // symmetric, as the reference's constructor makes it (src/interface.jl:1010-1017 symmetrises a non-symmetric entry)
                    const double *Ae = d->dense_A + d->dense_A_ptr[e];
                    for (int cc = 0; cc < k.n; cc++)
                        for (int rr = cc + 1; rr < k.n; rr++)
                            if (Ae[rr + (i64)cc * k.n] != Ae[cc + (i64)rr * k.n]) return fail(CLRS_ERR_INVALID, "dense constraint matrices must be symmetric");
                }
                std::memcpy(h_static.data() + k.w_off + (e - k.d0) * (i64)k.n * k.n, d->dense_A + d->dense_A_ptr[e], sizeof(double) * k.n * k.n);
            }
        }
    }
    return 0;
}

static int ctx_buffers(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const int J = c->J, N = c->N;
    CLRS_RET(upload(c, B.h_static, &c->d_static));
    double **bufs[] = {&c->d_work, &c->d_Xc, &c->d_Y, &c->d_X, &c->d_TY, &c->d_G, &c->d_TT, &c->d_Sd, &c->d_S, &c->d_LB, &c->d_Q,
                       &c->d_t, &c->d_dy, &c->d_rhsy, &c->d_dx, &c->d_rhsx, &c->d_AY};
    const i64 lens[] = {c->solve_arena_len, c->xylen, c->xylen, c->xylen, B.tyo, B.go, B.tto, B.sdo, c->Slen, c->xlen * (i64)N, (i64)N * N + N,
                        c->xlen, N, N, c->xlen, c->xlen, c->T};
    for (size_t i = 0; i < sizeof(lens) / sizeof(lens[0]); i++)
        CLRS_RET(dmalloc(c, bufs[i], lens[i]));
    c->d_u = c->d_Q + (i64)N * N;      // u directly behind Q: a sharded caller sums both partials over the ranks with ONE collective
    {   // B stacked: rows = all constraints (cluster after cluster), columns = free variables; ld = xlen
        std::vector<double> hB((size_t)std::max<i64>(c->xlen * (i64)N, 1), 0.0);
        i64 boff = 0;
        for (int j = 0; j < J; j++) {
            for (int col = 0; col < N; col++)
                for (int r = 0; r < c->P[j]; r++) hB[(size_t)(c->coff[j] + r + (i64)col * c->xlen)] = d->B[boff + r + (i64)col * c->P[j]];
            boff += (i64)c->P[j] * N;
        }
        CLRS_RET(upload(c, hB, &c->d_B));
    }
    std::vector<int> hi(2, INFO_NONE);   // [0]: S_j / Q factorisations, [1]: Cholesky of the X blocks
    return upload(c, hi, &c->d_info);
}

// ---- per-term gather tables ----
static int ctx_term_tables(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const int NB = c->NB;
    const i64 T = c->T;
    B.h_ayidx.resize(T); B.perm.resize(T); B.h_tptr.resize(NB);
    // the kernel wants the terms of a block sorted by p (CSR over p); build a permutation per block
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        if (k.kind != 0) continue;
        std::vector<i64> idx;
        for (i64 t = k.t0; t < k.t1; t++) idx.push_back(t);
        std::stable_sort(idx.begin(), idx.end(), [&](i64 a, i64 bb) { return d->term_p[a] < d->term_p[bb]; });
        const int Pj = c->P[k.j];
        std::vector<int> &tptr = B.h_tptr[b];
        tptr.assign(Pj + 1, 0);
        for (size_t q = 0; q < idx.size(); q++) {
            i64 t = idx[q];
            B.perm[k.t0 + q] = t;
            tptr[d->term_p[t] + 1]++;
        }
        for (int p = 0; p < Pj; p++) tptr[p + 1] += tptr[p];
        for (i64 t = k.t0; t < k.t1; t++) {
            int r = d->term_r[t], s = d->term_s[t];
            // A_Y[t] = bpY[r,s][pointers_left[r][(s,p,k)], pointers_right[s][(r,p,k)]]  (src/solver.jl:1163)
            i64 gl = k.offL[r] + B.lidx[t], gr = k.offR[s] + B.ridx[B.partner[t]];
            if (g_cfg_pairing_tri && k.sym && k.m == 1 && k.ULt == k.URt && gl < gr) std::swap(gl, gr);   // only the lower triangle of the symmetric GY is formed
            B.h_ayidx[t] = k.g_off + (i64)k.ULt * k.URt + gl + gr * k.ULt;
        }
    }
    B.s_tL.resize(T); B.s_tR.resize(T); B.s_tlam.resize(T);
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        if (k.kind != 0) continue;
        for (i64 q = k.t0; q < k.t1; q++) {
            i64 t = B.perm[q];
            B.s_tL[q] = k.offL[d->term_s[t]] + B.lidx[B.partner[t]];   // pointers_left[s][(r,p,k)]
            B.s_tR[q] = k.offR[d->term_r[t]] + B.ridx[t];              // pointers_right[r][(s,p,k)]
            B.s_tlam[q] = d->term_lambda[t];
        }
    }
    CLRS_RET(upload(c, B.s_tL, &B.d_tL)); CLRS_RET(upload(c, B.s_tR, &B.d_tR)); CLRS_RET(upload(c, B.s_tlam, &B.d_tlam));
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        if (k.kind == 0) {
            if (k.t1 == k.t0) continue;
            for (int &v : B.h_tptr[b]) v += (int)k.t0;   // absolute positions in the sorted term arrays
            CLRS_RET(upload(c, B.h_tptr[b], &k.d_tptr));
        } else if (k.cnt > 0) {
            std::vector<int> dp(d->dense_p + k.d0, d->dense_p + k.d1);
            CLRS_RET(upload(c, dp, &k.d_tptr));
        }
    }
    return 0;
}

// ---- which assembly kernel takes which cluster?  First come, first served: w5, w4, w1 / w2, fused; what is left goes the staged way ----
static void mark_cluster(clrs_ctx *c, const CtxBuild &B, int j, char kernel) {
    c->cluster_fused[j] = kernel;
    for (int b = B.cb[j]; b < B.cb[j + 1]; b++) c->blk[b].fused = true;
}

// k_cluster_assemble_w5: clusters whose PSD blocks are all 2 x 2 blocks of 16 x 16 sub-blocks with constraint matrices E_rs (x) v_u v_u^T on the SAME
// U <= 32 vectors in (0,0), (1,1) and as the two terms (0,1) + (1,0): 3 U constraints, every (pair, u) once (Nsphere_packing; clrs_assemble_w5.hip.h)
static int select_w5(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    auto &w = B.w5;
    for (int j = 0; j < c->J && g_cfg_fused_assemble && g_cfg_wave_assemble && g_cfg_wave5_assemble; j++) {
        const int b_first = B.cb[j], b_end = B.cb[j + 1], Pj = c->P[j];
        if (Pj < 3 || Pj % 3 != 0 || Pj > 96) continue;
        const int U = Pj / 3;
        bool ok = true;
        int nlr = 0;
        std::vector<int> pm0;
        struct Blk5 { std::vector<int> ay; std::vector<double> lam; };
        std::vector<Blk5> b5;
        for (int bb = b_first; bb < b_end && ok; bb++) {
            const BlockInfo &k = c->blk[bb];
            if (k.kind != 0) { if (k.cnt > 0) ok = false; continue; }
            const int Tn = (int)(k.t1 - k.t0);
            if (Tn == 0) continue;
            if (k.m != 2 || k.delta != 16 || !k.sym || Tn != 4 * U || (int)k.UR.size() != 2 || k.UR[0] != U || k.UR[1] != U) { ok = false; break; }
            // the same vectors in both sub-blocks
            const double *V = B.h_static.data() + k.zr_off;
            for (int u = 0; u < U && ok; u++)
                for (int i2 = 0; i2 < 16; i2++)
                    if (V[i2 + (i64)(k.offR[0] + u) * k.n] != V[16 + i2 + (i64)(k.offR[1] + u) * k.n]) { ok = false; break; }
            if (!ok) break;
            Blk5 e;
            e.ay.assign(4 * 32, -1);
            e.lam.assign(3 * U, 0.0);
            std::vector<int> pm(3 * U, -1), seen_terms(4 * U, 0);
            for (i64 q = k.t0; q < k.t1 && ok; q++) {
                const i64 t = B.perm[q];
                const int r = d->term_r[t], s2 = d->term_s[t];
                if (r < 0 || r > 1 || s2 < 0 || s2 > 1) { ok = false; break; }
                const int uR = B.s_tR[q] - k.offR[r], uL = B.s_tL[q] - k.offL[s2];
                if (uR != uL || uR < 0 || uR >= U) { ok = false; break; }
                const int pair = r + s2;                              // 0: (0,0); 1: (0,1) and (1,0); 2: (1,1)
                const int vi = pair * U + uR, ti2 = (2 * r + s2) * U + uR;
                if (seen_terms[ti2]++) { ok = false; break; }
                const int pc = d->term_p[t];
                const double lm = d->term_lambda[t];
                if (pm[vi] < 0) { pm[vi] = pc; e.lam[vi] = lm; }
                else if (pm[vi] != pc || e.lam[vi] != lm) { ok = false; break; }      // the two terms of an off-diagonal pair: one constraint, one lambda
                e.ay[(2 * r + s2) * 32 + uR] = (int)t;
            }
            if (!ok) break;
            for (int i2 = 0; i2 < 4 * U; i2++) if (seen_terms[i2] != 1) ok = false;
            std::vector<int> seen(pm);
            std::sort(seen.begin(), seen.end());
            for (int i2 = 0; i2 < 3 * U && ok; i2++) if (seen[i2] != i2) ok = false;      // a permutation of the cluster's constraints
            if (!ok) break;
            if (pm0.empty()) pm0 = pm;
            else if (pm != pm0) { ok = false; break; }
            b5.push_back(e);
            nlr++;
        }
        if (!ok || nlr == 0) continue;
        if (!std::is_sorted(pm0.begin(), pm0.end())) continue;      // (pm0 is a permutation.  Constraints in pair-major vector order only: a table lookup per stored entry costs the kernel its registers)
        w.cl_blk0.push_back((int)w.blk.size());
        int ilr = 0;
        for (int bb = b_first; bb < b_end; bb++) {
            const BlockInfo &k = c->blk[bb];
            if (k.kind != 0 || k.t1 == k.t0) continue;
            W3Block k5;
            std::memset(&k5, 0, sizeof(k5));
            k5.xyoff = k.xyoff; k5.n = k.n; k5.U = U; k5.pmap_identity = 1;
            k5.ndense = ilr == 0 ? 1 : 0;              // (first block of its cluster: it stores S_j, the others add to it)
            k5.S_off = c->Soff[j];                     // (every block of the cluster writes S_j: it accumulates in memory)
            k5.lam_off = (int)w.lam.size();
            w.lam.insert(w.lam.end(), b5[ilr].lam.begin(), b5[ilr].lam.end());
            k5.ay_base = (int)w.ay.size();
            w.ay.insert(w.ay.end(), b5[ilr].ay.begin(), b5[ilr].ay.end());
            ilr++;
            k5.vop_off = (int)(w.vop.size() / 512);
            w.vop.resize(w.vop.size() + 512, 0.0);
            pack_vop(B.h_static.data() + k.zr_off + (i64)k.offR[0] * k.n, k.n, 16, U, w.vop.data() + (size_t)k5.vop_off * 512, 2, 4);
            w.blk.push_back(k5);
        }
        W3Block &kl = w.blk.back();
        kl.last = 1; kl.S_off = c->Soff[j];
        mark_cluster(c, B, j, 5);
    }
    c->n_wave5_clusters = (int)w.cl_blk0.size();
    return 0;
}

// k_cluster_assemble_w4: clusters whose low-rank blocks are all "simple" (one sub-block, rank-1 symmetric terms, one term per constraint, U = P, the
// same constraint order in every block) with n <= 32 and P <= 64, dense blocks 1 x 1, and at least one block beyond the reach of
// k_cluster_assemble_w3 (n > 16 or P > 32): the register-resident kernel of clrs_assemble_w4.hip.h
static int select_w4(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    auto &w = B.w4;
    for (int j = 0; j < c->J && g_cfg_fused_assemble && g_cfg_wave_assemble && g_cfg_wave4_assemble; j++) {
        const int b_first = B.cb[j], b_end = B.cb[j + 1], Pj = c->P[j];
        if (Pj < 1 || Pj > 64 || c->cluster_fused[j] != 0) continue;
        bool ok = true, beyond_w3 = Pj > 32;
        int nlr = 0;
        std::vector<int> pm0;
        std::vector<std::vector<int>> ays;
        std::vector<std::vector<double>> lams;
        for (int bb = b_first; bb < b_end && ok; bb++) {
            const BlockInfo &k = c->blk[bb];
            if (k.kind == 0) {
                const int Tn = (int)(k.t1 - k.t0);
                if (Tn == 0) continue;
                if (k.m != 1 || k.n > 32 || !k.sym || k.URt != Tn || Tn != Pj) { ok = false; break; }
                std::vector<int> pm(Tn, -1), ay(Tn, -1);
                std::vector<double> lam(Tn, 0.0);
                for (i64 q = k.t0; q < k.t1 && ok; q++) {
                    const i64 t = B.perm[q];
                    const int u = B.s_tR[q];
                    if (B.s_tL[q] != u || u < 0 || u >= Tn || pm[u] >= 0) { ok = false; break; }
                    pm[u] = d->term_p[t]; lam[u] = d->term_lambda[t]; ay[u] = (int)t;
                }
                if (!ok) break;
                std::vector<int> seen(pm);
                std::sort(seen.begin(), seen.end());
                for (int i2 = 0; i2 < Tn; i2++) if (seen[i2] != i2) ok = false;      // a permutation of the cluster's constraints
                if (!ok) break;
                if (pm0.empty()) pm0 = pm;
                else if (pm != pm0) { ok = false; break; }
                if (k.n > 16) beyond_w3 = true;
                ays.push_back(ay); lams.push_back(lam);
                nlr++;
            } else if (k.cnt > 0 && k.n != 1) ok = false;
        }
        if (!ok || nlr == 0 || !beyond_w3) continue;
        std::vector<int> inv(Pj, -1);
        for (int u = 0; u < Pj; u++) inv[pm0[u]] = u;
        const int nu = (Pj + 15) / 16 <= 3 ? 3 : 4;
        w.nu = std::max(w.nu, nu);
        w.cl_blk0.push_back((int)w.blk.size());
        const int pm_off = (int)w.pmap.size();
        w.pmap.insert(w.pmap.end(), pm0.begin(), pm0.end());
        const bool ident = std::is_sorted(pm0.begin(), pm0.end());      // (of a permutation: the identity)
        const int dense0 = (int)w.dense.size();
        size_t last_lr = 0;
        int ilr = 0;
        for (int bb = b_first; bb < b_end; bb++) {
            const BlockInfo &k = c->blk[bb];
            if (k.kind != 0) {
                if (k.cnt == 0) continue;
                W3Dense de; de.xyoff = k.xyoff; de.lam_off = (int)w.lam.size(); de.pad = 0;
                std::vector<double> a(Pj, 0.0);
                for (i64 e = k.d0; e < k.d1; e++) a[inv[d->dense_p[e]]] = d->dense_A[d->dense_A_ptr[e]];
                w.lam.insert(w.lam.end(), a.begin(), a.end());
                w.dense.push_back(de);
                continue;
            }
            if (k.t1 == k.t0) continue;
            W3Block k4;
            std::memset(&k4, 0, sizeof(k4));
            k4.xyoff = k.xyoff; k4.n = k.n; k4.U = Pj; k4.pmap_off = pm_off; k4.pmap_identity = ident ? 1 : 0;
            k4.lam_off = (int)w.lam.size();
            w.lam.insert(w.lam.end(), lams[ilr].begin(), lams[ilr].end());
            k4.ay_base = (int)w.ay.size();
            w.ay.insert(w.ay.end(), ays[ilr].begin(), ays[ilr].end());
            ilr++;
            k4.vop_off = (int)(w.vop.size() / 512);
            w.vop.resize(w.vop.size() + (size_t)4 * 512, 0.0);      // (four column tiles for every block: the launch's NU is the largest of its clusters')
            pack_vop(B.h_static.data() + k.zr_off, k.n, k.n, Pj, w.vop.data() + (size_t)k4.vop_off * 512, nu, 8);
            last_lr = w.blk.size();
            w.blk.push_back(k4);
        }
        W3Block &kl = w.blk[last_lr];
        kl.last = 1; kl.S_off = c->Soff[j];
        kl.ndense = (int)w.dense.size() - dense0; kl.dense0 = dense0;
        mark_cluster(c, B, j, 4);
    }
    c->n_wave4_clusters = (int)w.cl_blk0.size();
    return 0;
}

// the cluster-per-wave form of a w1 candidate: every low-rank block uses the same constraint order (U = P) and the dense blocks are 1 x 1
static bool select_w2(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B, int j, const std::vector<WBlock> &mine, const std::vector<size_t> &mine_off, int utr) {
    auto &w2 = B.w2;
    const auto &w = B.w1;
    const int Pj = c->P[j];
    const int *pm0 = nullptr;
    for (size_t i2 = 0; i2 < mine.size(); i2++) {
        const WBlock &wb = mine[i2];
        if (wb.kind == 0) {
            const int *pm = w.pmap.data() + mine_off[i2];
            if (wb.U != Pj) return false;
            else if (!pm0) pm0 = pm;
            else if (std::memcmp(pm, pm0, sizeof(int) * Pj) != 0) return false;
        } else if (wb.n != 1) return false;
    }
    if (!pm0) return false;
    std::vector<int> inv(Pj, -1);
    for (int u = 0; u < Pj; u++) inv[pm0[u]] = u;
    W2Cluster wc2;
    std::memset(&wc2, 0, sizeof(wc2));
    wc2.S = c->d_S + c->Soff[j]; wc2.P = Pj; wc2.nblk = (int)mine.size(); wc2.blk0 = (i64)w2.bl.size();
    w2.cl_pm.push_back(w2.pmap.size());
    w2.pmap.insert(w2.pmap.end(), pm0, pm0 + Pj);
    int bsel = B.cb[j];
    for (size_t i2 = 0; i2 < mine.size(); i2++) {
        const WBlock &wb = mine[i2];
        W2Block q2;
        std::memset(&q2, 0, sizeof(q2));
        q2.kind = wb.kind; q2.n = wb.n; q2.xyoff = wb.xyoff; q2.v_off = wb.v_off;
        w2.boff.push_back(w2.lam.size());
        w2.bl_cl.push_back(w2.cl.size());
        if (wb.kind == 0) {
            w2.lam.insert(w2.lam.end(), w.lam.begin() + mine_off[i2], w.lam.begin() + mine_off[i2] + Pj);
            w2.ay.insert(w2.ay.end(), w.ay.begin() + mine_off[i2], w.ay.begin() + mine_off[i2] + Pj);
        } else {
            // locate the BlockInfo of this dense block to read its 1 x 1 matrices
            while (!(c->blk[bsel].kind != 0 && c->blk[bsel].xyoff == wb.xyoff)) bsel++;
            const BlockInfo &kb = c->blk[bsel];
            std::vector<double> a(Pj, 0.0);
            for (i64 e = kb.d0; e < kb.d1; e++) a[inv[d->dense_p[e]]] = d->dense_A[d->dense_A_ptr[e]];
            w2.lam.insert(w2.lam.end(), a.begin(), a.end());
            w2.ay.insert(w2.ay.end(), Pj, 0);
        }
        w2.bl.push_back(q2);
    }
    w2.cl.push_back(wc2);
    w2.ut = std::max(w2.ut, utr);
    mark_cluster(c, B, j, 3);
    return true;
}

// wave-per-block assembly (k_cluster_assemble_w1): clusters made of "simple" rank-1 blocks with n <= 16 and small dense blocks
static int select_w1_w2(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    auto &w = B.w1;
    const int J = c->J;
    for (int j = 0; j < J && g_cfg_fused_assemble && g_cfg_wave_assemble; j++) {
        bool ok = c->cluster_fused[j] == 0;      // (not taken by k_cluster_assemble_w4)
        int work = 0, ut = 1, nblk = 0;
        std::vector<WBlock> mine;
        std::vector<size_t> mine_off;
        const size_t keep_pm = w.pmap.size(), keep_lam = w.lam.size(), keep_ay = w.ay.size();
        for (int b = B.cb[j]; b < B.cb[j + 1] && ok; b++) {
            BlockInfo &k = c->blk[b];
            WBlock wb;
            std::memset(&wb, 0, sizeof(wb));
            wb.kind = k.kind; wb.n = k.n; wb.xyoff = k.xyoff;
            if (k.kind == 0) {
                const int Tn = (int)(k.t1 - k.t0);
                if (Tn == 0) continue;
                if (k.m != 1 || k.n > 16 || !k.sym || k.URt != Tn || Tn > 128) { ok = false; continue; }
                std::vector<int> pm(Tn, -1), ay(Tn, -1);
                std::vector<double> lam(Tn, 0.0);
                for (i64 q = k.t0; q < k.t1 && ok; q++) {
                    const i64 t = B.perm[q];
                    const int u = B.s_tR[q];
                    if (B.s_tL[q] != u || u < 0 || u >= Tn || pm[u] >= 0) { ok = false; break; }
                    pm[u] = d->term_p[t]; lam[u] = d->term_lambda[t]; ay[u] = (int)t;
                }
                if (ok) {   // one term per constraint
                    std::vector<int> seen(pm);
                    std::sort(seen.begin(), seen.end());
                    for (int i2 = 1; i2 < Tn; i2++) if (seen[i2] == seen[i2 - 1]) ok = false;
                }
                if (!ok) continue;
                wb.U = Tn; wb.v_off = k.zr_off;
                mine_off.push_back(w.pmap.size());
                w.pmap.insert(w.pmap.end(), pm.begin(), pm.end());
                w.ay.insert(w.ay.end(), ay.begin(), ay.end());
                w.lam.resize(w.pmap.size(), 0.0);
                std::copy(lam.begin(), lam.end(), w.lam.end() - Tn);
                ut = std::max(ut, (Tn + 15) / 16);
            } else {
                if (k.cnt == 0) continue;
                const int need = 2 * k.n * k.n + 3 * k.cnt * k.n * k.n;
                if (k.n > 16 || need > 4096) { ok = false; continue; }
                wb.U = k.cnt; wb.v_off = k.w_off;
                mine_off.push_back(w.pmap.size());
                for (i64 e = k.d0; e < k.d1; e++) { w.pmap.push_back(d->dense_p[e]); w.ay.push_back(0); }
                w.lam.resize(w.pmap.size(), 0.0);
                work = std::max(work, need);
            }
            mine.push_back(wb);
            nblk++;
        }
        const int utr = ut <= 2 ? 2 : ut <= 4 ? 4 : 8;
        work = std::max(work, 2 * 17 * 16 * utr);
        const i64 per_wave = (i64)c->P[j] * (c->P[j] | 1) + work;     // slab (odd leading dimension) + work area
        // cluster-per-wave kernel ("wave2_assemble" = 1: automatic, 2: always, 0: never.  Automatic: always when the register-resident kernel
        // k_cluster_assemble_w3 applies (U <= 32) -- it is also the fastest form for a handful of clusters, 8 us against 12.5 us of
        // the wave-per-block kernel on cohnelkies(8,15) -- and from 64 clusters on for the LDS-staged k_cluster_assemble_w2,
        // which walks the blocks of a cluster one after the other and needs enough clusters to fill the chip)
        const bool try_w2 = (g_cfg_wave2_assemble == 2 || (g_cfg_wave2_assemble == 1 && (J >= 64 || (g_cfg_wave3_assemble && utr <= 2)))) && utr <= 4;
        if (!ok || mine.empty() || per_wave > LDS_BUDGET_DOUBLES || (try_w2 && select_w2(c, d, B, j, mine, mine_off, utr))) {
            w.pmap.resize(keep_pm); w.lam.resize(keep_lam); w.ay.resize(keep_ay);
            continue;
        }
        WCluster wc;
        std::memset(&wc, 0, sizeof(wc));
        wc.S = c->d_S + c->Soff[j]; wc.P = c->P[j]; wc.nblk = (int)mine.size(); wc.work_doubles = work;
        w.cl_first.push_back(w.bl.size());
        for (size_t i2 = 0; i2 < mine.size(); i2++) { w.bl.push_back(mine[i2]); w.ioff.push_back(mine_off[i2]); }
        w.cl.push_back(wc);
        mark_cluster(c, B, j, 2);
        w.ut = std::max(w.ut, utr);
        w.nwaves = std::min(w.nwaves, (int)(LDS_BUDGET_DOUBLES / per_wave));
        w.maxblocks = std::max(w.maxblocks, nblk);
        w.cluster_doubles = std::max(w.cluster_doubles, (size_t)per_wave);
    }
    w.nwaves = std::max(1, std::min(w.nwaves, std::max(w.maxblocks, 1)));
    for (WCluster &wc : w.cl) wc.work_doubles = (int)(w.cluster_doubles - (size_t)wc.P * (wc.P | 1));   // one slab + work stride for all clusters
    // a cluster whose own P^2 + work is smaller still gets the common stride; re-check the budget with it
    if ((i64)w.nwaves * (i64)w.cluster_doubles > LDS_BUDGET_DOUBLES) w.nwaves = std::max(1, (int)(LDS_BUDGET_DOUBLES / (i64)w.cluster_doubles));
    c->n_wave_clusters = (int)w.cl.size(); c->n_wave2_clusters = (int)B.w2.cl.size();
    return 0;
}

// ---- which clusters does the fused kernel take?  (everything of the cluster must fit in LDS) ----
static int select_fused(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    auto &f = B.fu;
    for (int j = 0; j < c->J && g_cfg_fused_assemble; j++) {
        int szL = 0, szY = 0, szV = 0, szTY = 0, szZL = 0, szG = 0, szTab = 0, nmax = 0;
        bool ok = c->cluster_fused[j] == 0;      // not already taken by the wave-per-block kernel
        std::vector<FBlock> mine;
        for (int b = B.cb[j]; b < B.cb[j + 1] && ok; b++) {
            BlockInfo &k = c->blk[b];
            FBlock fb;
            std::memset(&fb, 0, sizeof(fb));
            fb.kind = k.kind; fb.n = k.n; fb.xyoff = k.xyoff;
            const int n = k.n, n16 = (n + 15) & ~15;
            if (k.kind == 0) {
                if (k.t1 == k.t0) continue;
                if (n > 64) { ok = false; continue; }
                const int UR16 = (k.URt + 15) & ~15, UL16 = (k.ULt + 15) & ~15, Tn = (int)(k.t1 - k.t0);
                fb.URt = k.URt; fb.ULt = k.ULt; fb.sym = k.sym ? 1 : 0; fb.T = Tn;
                fb.ldn = n16 + 2;                    // >= ceil16(n) rows (zero padded), ldn % 4 == 2: conflict-free ds_read_b64 of the MFMA operands
                fb.ldg = k.ULt | 1;
                fb.v_off = k.zr_off; fb.w_off = k.zl_off; fb.t0 = k.t0; fb.tptr = k.d_tptr;
                szL = std::max(szL, fb.ldn * n16); szY = std::max(szY, fb.ldn * n16);
                szV = std::max(szV, fb.ldn * UR16); szTY = std::max(szTY, fb.ldn * UR16);
                if (!k.sym) szZL = std::max(szZL, fb.ldn * UL16);
                szG = std::max(szG, fb.ldg * k.URt);
                szTab = std::max(szTab, ((c->P[j] + 1 + 2 * Tn + 1) & ~1) / 2 + Tn);
                nmax = std::max(nmax, n);
            } else {
                if (k.cnt == 0) continue;
                if (n > 16) { ok = false; continue; }
                fb.T = k.cnt; fb.ldn = n | 1; fb.v_off = k.w_off; fb.tptr = k.d_tptr;
                const int st = k.cnt * n * n;
                szL = std::max(szL, fb.ldn * n); szY = std::max(szY, fb.ldn * n);
                szV = std::max(szV, st); szTY = std::max(szTY, st); szG = std::max(szG, st);
                szTab = std::max(szTab, (k.cnt + 1) / 2);
            }
            mine.push_back(fb);
        }
        if (!ok || mine.empty()) continue;
        FCluster fc;
        std::memset(&fc, 0, sizeof(fc));
        fc.S = c->d_S + c->Soff[j]; fc.P = c->P[j];
        auto even = [](int v) { return (v + 1) & ~1; };   // keep every region 16-byte aligned
        int o = 0;
        fc.oL = o; o += even(szL); fc.oY = o; o += even(szY); fc.oV = o; o += even(szV); fc.oTY = o; o += even(szTY);
        fc.oZL = o; o += even(szZL); fc.oGX = o; o += even(szG); fc.oGY = o; o += even(szG); fc.oTab = o; o += even(szTab);
        if (o > LDS_BUDGET_DOUBLES) continue;
        const int PP = c->P[j] * c->P[j];
        fc.oS = o;
        if (o + PP <= LDS_BUDGET_DOUBLES) { fc.s_in_lds = 1; o += even(PP); }
        fc.lds_doubles = o;
        fc.b0 = (int)f.bl.size();
        for (const FBlock &fb : mine) f.bl.push_back(fb);
        fc.b1 = (int)f.bl.size();
        f.cl.push_back(fc);
        mark_cluster(c, B, j, 1);
        f.nmax = std::max(f.nmax, nmax);
        f.lds = std::max(f.lds, (size_t)o * sizeof(double));
    }
    c->n_fused_clusters = (int)f.cl.size() + c->n_wave_clusters + c->n_wave2_clusters + c->n_wave4_clusters + c->n_wave5_clusters;
    // Few clusters with several blocks each: the blocks of a cluster are independent until their contributions meet in S_j.  One
    // workgroup per block (groups of blocks beyond 32 per cluster) writes its contribution as a P x P slab, k_sum_S_slabs adds
    // the slabs in block order -- the same additions in the same order as the one-workgroup form, so S_j is bit-identical.
    if (!g_cfg_split_blocks || f.cl.empty() || f.cl.size() > 32) return 0;
    std::vector<FCluster> split;
    std::vector<int> split_sum;                // per entry of `split`: its sum descriptor, or -1
    i64 slab_doubles = 0;
    for (const FCluster &fc : f.cl) {
        const int nb = fc.b1 - fc.b0, groups = std::min(nb, 32);
        if (nb < 2) { split.push_back(fc); split_sum.push_back(-1); continue; }
        SSlabSum ss;
        ss.out = fc.S; ss.slabs = nullptr; ss.len = (i64)fc.P * fc.P; ss.nslabs = groups; ss.pad = (int)slab_doubles;      // offset for now (fits: few small clusters)
        for (int g = 0; g < groups; g++) {
            FCluster part = fc;
            part.b0 = fc.b0 + (int)((i64)g * nb / groups);
            part.b1 = fc.b0 + (int)((i64)(g + 1) * nb / groups);
            part.S = nullptr;                       // patched below: slab g of this cluster
            split.push_back(part);
            split_sum.push_back((int)f.sum.size());
        }
        slab_doubles += ss.len * groups;
        f.sum.push_back(ss);
    }
    if (f.sum.empty()) return 0;
    double *dslabs;
    CLRS_RET(dmalloc(c, &dslabs, slab_doubles));
    std::vector<int> used(f.sum.size(), 0);
    for (size_t i = 0; i < split.size(); i++)
        if (split_sum[i] >= 0) {
            const int si = split_sum[i];
            split[i].S = dslabs + f.sum[si].pad + f.sum[si].len * used[si]++;
        }
    for (SSlabSum &ss : f.sum) { ss.slabs = dslabs + ss.pad; ss.pad = 0; }
    f.cl.swap(split);
    return 0;
}

// ---- A_Y index tables, host copies of the description for the interior-point tables ----
static int ctx_ay_tables(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const i64 T = c->T;
    for (const BlockInfo &k : c->blk)
        if (k.fused && k.kind == 0)
            for (i64 t = k.t0; t < k.t1; t++) B.h_ayidx[t] = -1;   // written by the fused kernel
    CLRS_RET(upload(c, B.h_ayidx, &c->d_ayidx));
    std::vector<int> h_ayL(T), h_ayR(T);
    for (const BlockInfo &k : c->blk) {
        if (k.kind != 0) continue;
        for (i64 t = k.t0; t < k.t1; t++) {
            h_ayL[t] = k.offL[d->term_r[t]] + B.lidx[t];
            h_ayR[t] = k.offR[d->term_s[t]] + B.ridx[B.partner[t]];
        }
    }
    CLRS_RET(upload(c, h_ayL, &c->d_ayL)); CLRS_RET(upload(c, h_ayR, &c->d_ayR));
    c->h_term_p.assign(d->term_p, d->term_p + T); c->h_term_lambda.assign(d->term_lambda, d->term_lambda + T);
    c->h_dense_p.assign(d->dense_p, d->dense_p + c->D);
    return 0;
}

// plan: assemble.  The staged (general) path of the blocks no special kernel took, then one launch per special kernel
static int plan_assemble_general(clrs_ctx *c, const clrs_sdp_desc *d, CtxBuild &B) {
    const int J = c->J, NB = c->NB;
    Plan &pl = c->p_assemble;
    bool need_copy = false;
    for (int b = 0; b < NB; b++) need_copy = need_copy || !c->blk[b].fused;
    c->all_assemble_fused = !need_copy;
    // which of the non-fused blocks still need the work arena (a copy of the static arena that the staged solves overwrite)?
    bool need_work_arena = false;
    std::vector<DBlock> dblocks;
    size_t dense_lds = 0;
    const size_t copy_step_index = pl.steps.size();
    if (need_copy) add_memcpy(pl, c->d_work, c->d_static, sizeof(double) * (size_t)c->solve_arena_len);
    std::vector<TrsmJob> fwd, bwd;
    std::vector<DenseTBlock> dtb;                       // dense blocks taken by k_dense_T32
    std::vector<DenseTPair> dtp;
    std::vector<GemmDesc> g1, g2;
    bool any_general = false;
    for (int b = 0; b < NB; b++) {
        BlockInfo &k = c->blk[b];
        const double *Lx = c->d_Xc + k.xyoff, *Yb = c->d_Y + k.xyoff;
        const int n = k.n, dl = k.delta;
        if (k.fused) continue;
        any_general = true;
        if (k.kind == 0) {
            need_work_arena = true;
            double *ZR = c->d_work + k.zr_off, *ZL = c->d_work + k.zl_off, *TY = c->d_TY + k.ty_off;
            double *GX = c->d_G + k.g_off, *GY = GX + (i64)k.ULt * k.URt;
            const double *VR = c->d_static + k.zr_off, *WL = c->d_static + k.zl_off;
            for (int r = 0; r < k.m; r++) {
                const int r0 = r * dl;
                // columns of sub-block row r are zero above row r0: solve with the trailing triangle only
                if (k.UR[r] > 0) fwd.push_back(TrsmJob{Lx + r0 + (i64)r0 * n, n, n - r0, ZR + r0 + (i64)k.offR[r] * n, n, k.UR[r]});
                if (!k.sym && k.UL[r] > 0) fwd.push_back(TrsmJob{Lx + r0 + (i64)r0 * n, n, n - r0, ZL + r0 + (i64)k.offL[r] * n, n, k.UL[r]});
                // T_Y[:, cols r] = Y[:, r-block] V_r            (src/solver.jl:1125)
                if (k.UR[r] > 0)
                    g1.push_back(mk_gemm(0, 0, n, k.UR[r], dl, 1.0, Yb + (i64)r0 * n, n, VR + r0 + (i64)k.offR[r] * n, n, 0.0, TY + (i64)k.offR[r] * n, n));
            }
            // W = V in one sub-block: GX = V^T X^-1 V and GY = V^T Y V are symmetric -- lower tiles only, the gather mirrors its reads
            const int tri = g_cfg_pairing_tri && k.sym && k.m == 1 && k.ULt == k.URt ? 1 : 0;
            for (int s = 0; s < k.m; s++)  // GY[rows s, :] = W_s^T T_Y[s-block, :]   (src/solver.jl:1131)
                if (k.UL[s] > 0 && k.URt > 0)
                    g2.push_back(mk_gemm(1, 0, k.UL[s], k.URt, dl, 1.0, WL + s * dl + (i64)k.offL[s] * n, n, TY + s * dl, n, 0.0, GY + k.offL[s], k.ULt, 1, 0, 0, 0, tri));
            // GX = ZL^T ZR = W^T X^-1 V       (replaces src/solver.jl:1117,1137-1143)
            if (k.ULt > 0 && k.URt > 0) g2.push_back(mk_gemm(1, 0, k.ULt, k.URt, n, 1.0, ZL, n, ZR, n, 0.0, GX, k.ULt, 1, 0, 0, 0, tri));
        } else if (k.cnt > 0) {
            const size_t n16 = (n + 15) & ~15, msz = (n16 + 2) * n16, need = 2 * msz + n16 + 2 * (size_t)k.cnt * msz + 1024;
            if (g_cfg_dense_block && g_cfg_fused_assemble && n <= 64 && need <= (size_t)LDS_BUDGET_DOUBLES) {   // dense block that fits in LDS: one fused launch for all such blocks
                DBlock db;
                db.n = n; db.cnt = k.cnt; db.xyoff = k.xyoff; db.a_off = k.w_off; db.Sd = c->d_Sd + k.sd_off;
                dblocks.push_back(db);
                dense_lds = std::max(dense_lds, need * sizeof(double));
                continue;
            }
            double *W = c->d_work + k.w_off, *TT = c->d_TT + k.tt_off, *Sd = c->d_Sd + k.sd_off;
            const double *Ast = c->d_static + k.w_off;
            if (g_cfg_dense_wave && n <= 32) {      // T_e = X^-1 A_e Y by one wave per matrix (k_dense_T32), then the same Gram GEMM
                const int bi = (int)dtb.size();
                dtb.push_back(DenseTBlock{Lx, Yb, Ast, nullptr, TT, n, k.cnt});
                for (int e0 = 0; e0 < k.cnt; e0 += DT32_WAVES * DT32_ITER) dtp.push_back(DenseTPair{bi, e0});
            } else {
                need_work_arena = true;
                fwd.push_back(TrsmJob{Lx, n, n, W, n, n * k.cnt});      // X^-1 A_p for all p  (src/solver.jl:1095)
                bwd.push_back(TrsmJob{Lx, n, n, W, n, n * k.cnt});
                g1.push_back(mk_gemm(0, 0, n, n, n, 1.0, W, n, Yb, n, 0.0, TT, n, k.cnt, (i64)n * n, 0, (i64)n * n));  // (X^-1 A_p) Y  (:1097)
            }
            k.sd_tri = g_cfg_pairing_tri != 0;      // <A_i, X^-1 A_k Y> = tr(A_i X^-1 A_k Y) is symmetric in (i, k): lower tiles, mirrored reads
            g2.push_back(mk_gemm(1, 0, k.cnt, k.cnt, n * n, 1.0, Ast, n * n, TT, n * n, 0.0, Sd, k.cnt, 1, 0, 0, 0, k.sd_tri ? 1 : 0));           // <A_i, T_k>   (:1102)
        }
    }
    if (need_copy && !need_work_arena) pl.steps.erase(pl.steps.begin() + copy_step_index);   // nothing left that overwrites it
    CLRS_RET(plan_trsm(c, pl, fwd, 0)); CLRS_RET(plan_trsm(c, pl, bwd, 1)); CLRS_RET(add_gemm_stage(c, pl, g1));
    if (!dtb.empty()) {
        double *linv = nullptr;
        CLRS_RET(dmalloc(c, &linv, (i64)dtb.size() * 1024));
        for (size_t i = 0; i < dtb.size(); i++) dtb[i].Linv = linv + i * 1024;
        DenseTBlock *dblk; DenseTPair *dpr;
        CLRS_RET(upload(c, dtb, &dblk)); CLRS_RET(upload(c, dtp, &dpr));
        Step s1;
        s1.kind = STEP_TRTRI32; s1.grid = (int)dtb.size(); s1.d0 = dblk;
        pl.steps.push_back(s1);
        Step s2;
        s2.kind = STEP_DENSE_T32; s2.grid = (int)dtp.size(); s2.d0 = dblk; s2.d1 = dpr;
        pl.steps.push_back(s2);
        HIPCHECK(hipFuncSetAttribute((const void *)k_dense_T32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dense_T32_lds_bytes()));
    }
    CLRS_RET(add_gemm_stage(c, pl, g2));
    if (!dblocks.empty()) {
        DBlock *ddb;
        CLRS_RET(upload(c, dblocks, &ddb));
        c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y; c->ftables.stat = c->d_static;
        Step s;
        s.kind = STEP_DENSE_BLOCK; s.grid = (int)dblocks.size(); s.d0 = ddb; s.src = &c->ftables; s.bytes = dense_lds;
        pl.steps.push_back(s);
        CLRS_RET(raise_lds_limit((const void *)k_dense_block, dense_lds));
    }
    // gather
    std::vector<SClusterDesc> cl(J);
    std::vector<SBlockDesc> bl;
    std::vector<STile> tiles;
    for (int j = 0; j < J; j++) {
        cl[j].S = c->d_S + c->Soff[j]; cl[j].P = c->P[j]; cl[j].b0 = (int)bl.size(); cl[j].pad = 0;
        for (int b = B.cb[j]; b < B.cb[j + 1]; b++) {
            BlockInfo &k = c->blk[b];
            SBlockDesc sd;
            std::memset(&sd, 0, sizeof(sd));
            sd.kind = k.kind;
            if (k.fused) continue;
            if (k.kind == 0) {
                if (k.t1 == k.t0) continue;
                sd.ldg = k.ULt;
                sd.tri = g_cfg_pairing_tri && k.sym && k.m == 1 && k.ULt == k.URt ? 1 : 0;
                sd.GX = c->d_G + k.g_off; sd.GY = sd.GX + (i64)k.ULt * k.URt;
                sd.tptr = k.d_tptr; sd.tL = B.d_tL; sd.tR = B.d_tR; sd.tlam = B.d_tlam;
            } else {
                if (k.cnt == 0) continue;
                sd.cnt = k.cnt; sd.Sd = c->d_Sd + k.sd_off; sd.tri = k.sd_tri ? 1 : 0;
                std::vector<int> inv(c->P[j], -1);
                for (i64 e = k.d0; e < k.d1; e++) inv[d->dense_p[e]] = (int)(e - k.d0);
                int *dinv;
                CLRS_RET(upload(c, inv, &dinv));
                sd.inv = dinv;
            }
            bl.push_back(sd);
        }
        cl[j].b1 = (int)bl.size();
        if (c->cluster_fused[j]) continue;
        int nt = (c->P[j] + 15) / 16;
        for (int tj = 0; tj < nt; tj++)
            for (int ti = 0; ti <= tj; ti++) tiles.push_back(STile{j, ti, tj, 0});
    }
    if (!tiles.empty()) {
        Step s;
        s.kind = STEP_GATHER_S;
        s.grid = (int)tiles.size();
        for (const SClusterDesc &cd : cl) s.aux0 = std::max(s.aux0, cd.b1 - cd.b0);      // most blocks in one cluster
        SClusterDesc *dcl; SBlockDesc *dbl; STile *dt;
        CLRS_RET(upload(c, cl, &dcl)); CLRS_RET(upload(c, bl, &dbl)); CLRS_RET(upload(c, tiles, &dt));
        s.d0 = dcl; s.d1 = dbl; s.d2 = dt;
        pl.steps.push_back(s);
    }
    if (c->T > 0 && any_general) {
        Step s;
        s.kind = STEP_GATHER_SCALAR;
        s.dst = c->d_AY; s.src = c->d_G; s.d0 = c->d_ayidx; s.n = c->T;
        pl.steps.push_back(s);
    }
    return 0;
}

static int plan_w5(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    const auto &w = B.w5;
    if (w.blk.empty()) return 0;
    int *dcb, *day; W3Block *db5; double *dvop, *dlam;
    CLRS_RET(upload(c, w.cl_blk0, &dcb)); CLRS_RET(upload(c, w.blk, &db5)); CLRS_RET(upload(c, w.vop, &dvop));
    CLRS_RET(upload(c, w.ay, &day)); CLRS_RET(upload(c, w.lam, &dlam));
    c->w5tables.Xc = c->d_Xc; c->w5tables.Y = c->d_Y; c->w5tables.S = c->d_S; c->w5tables.AY = c->d_AY;
    c->w5tables.vop = dvop; c->w5tables.lam = dlam; c->w5tables.ay = day;
    c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y;
    Step s;
    s.kind = STEP_ASSEMBLE_W5;
    s.d0 = dcb; s.d1 = db5; s.src = &c->w5tables; s.n = (i64)w.cl_blk0.size();
    s.aux0 = (int)std::min<i64>(((i64)w.cl_blk0.size() + 3) / 4, (i64)cu_count(c));
    s.aux1 = (int)w.blk.size();
    c->p_assemble.steps.push_back(s);
    return 0;
}

static int plan_w4(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    auto &w = B.w4;
    if (w.blk.empty()) return 0;
    if (w.dense.empty()) { W3Dense de; std::memset(&de, 0, sizeof(de)); w.dense.push_back(de); }
    if (w.ay.empty()) w.ay.push_back(0);
    int *dcb, *dpm, *day; W3Block *db4; W3Dense *dd4; double *dvop, *dlam;
    CLRS_RET(upload(c, w.cl_blk0, &dcb)); CLRS_RET(upload(c, w.blk, &db4)); CLRS_RET(upload(c, w.dense, &dd4)); CLRS_RET(upload(c, w.vop, &dvop));
    CLRS_RET(upload(c, w.pmap, &dpm)); CLRS_RET(upload(c, w.ay, &day)); CLRS_RET(upload(c, w.lam, &dlam));
    c->w4tables.Xc = c->d_Xc; c->w4tables.Y = c->d_Y; c->w4tables.S = c->d_S; c->w4tables.AY = c->d_AY;
    c->w4tables.vop = dvop; c->w4tables.lam = dlam; c->w4tables.pmap = dpm; c->w4tables.ay = day; c->w4tables.dense = dd4;
    c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y;
    const int nu = w.nu <= 3 ? 3 : 4;
    Step s;
    s.kind = STEP_ASSEMBLE_W4;
    s.d0 = dcb; s.d1 = db4; s.src = &c->w4tables; s.n = (i64)w.cl_blk0.size(); s.nmax = w.nu;
    int maxP = 1;
    for (const W3Block &kb : w.blk) maxP = std::max(maxP, kb.U);
    s.grid = maxP;                                                                   // rows of the staged S_j
    s.bytes = W4_LDS_BYTES(nu, maxP);
    s.aux0 = (int)std::min<i64>(((i64)w.cl_blk0.size() + 3) / 4, (i64)cu_count(c) * W4_WGS_PER_CU(nu));      // as many workgroups as are resident at once
    s.aux1 = (int)w.blk.size();
    c->p_assemble.steps.push_back(s);
    HIPCHECK(hipFuncSetAttribute(nu == 3 ? (const void *)k_cluster_assemble_w4<3> : (const void *)k_cluster_assemble_w4<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.bytes));
    return 0;
}

// k_cluster_assemble_w3 instead of _w2: flat sequence of the low-rank blocks, vectors in MFMA-operand order, the 1 x 1 dense
// blocks attached to the last low-rank block of their cluster
static int plan_w3(clrs_ctx *c, const CtxBuild &B, Step &s, bool full, int *dpm, double *dlam) {
    const auto &w = B.w2;
    std::vector<W3Block> b3;
    std::vector<W3Dense> d3;
    std::vector<int> cl_blk0;
    std::vector<double> h_vop;
    for (size_t ci = 0; ci < w.cl.size(); ci++) {
        const W2Cluster &wc = w.cl[ci];
        cl_blk0.push_back((int)b3.size());
        const int dense0 = (int)d3.size();
        size_t last_lr = 0;
        for (int i2 = 0; i2 < wc.nblk; i2++) {
            const size_t bi2 = (size_t)wc.blk0 + i2;
            const W2Block &q2 = w.bl[bi2];
            if (q2.kind != 0) { W3Dense de; de.xyoff = q2.xyoff; de.lam_off = (int)w.boff[bi2]; de.pad = 0; d3.push_back(de); continue; }
            W3Block k3;
            std::memset(&k3, 0, sizeof(k3));
            k3.xyoff = q2.xyoff; k3.n = q2.n; k3.U = wc.P; k3.lam_off = (int)w.boff[bi2]; k3.pmap_off = (int)w.cl_pm[ci];
            k3.ay_base = w.ay[w.boff[bi2]];
            k3.vop_off = (int)(h_vop.size() / 512);
            h_vop.resize(h_vop.size() + 512, 0.0);
            pack_vop(B.h_static.data() + q2.v_off, q2.n, q2.n, wc.P, h_vop.data() + (size_t)k3.vop_off * 512, 2, 4);
            last_lr = b3.size();
            b3.push_back(k3);
        }
        W3Block &kl = b3[last_lr];
        kl.last = 1; kl.S_off = (i64)(wc.S - c->d_S);
        kl.pmap_identity = std::is_sorted(w.pmap.begin() + w.cl_pm[ci], w.pmap.begin() + w.cl_pm[ci] + wc.P) ? 1 : 0;      // (of a permutation: the identity)
        kl.ndense = (int)d3.size() - dense0; kl.dense0 = dense0;
        if (kl.ndense > 0) { kl.dxyoff = d3[dense0].xyoff; kl.dlam_off = d3[dense0].lam_off; }
    }
    if (d3.empty()) { W3Dense de; std::memset(&de, 0, sizeof(de)); d3.push_back(de); }
    int *dcb; W3Block *db3; W3Dense *dd3; double *dvop;
    CLRS_RET(upload(c, cl_blk0, &dcb)); CLRS_RET(upload(c, b3, &db3)); CLRS_RET(upload(c, d3, &dd3)); CLRS_RET(upload(c, h_vop, &dvop));
    c->w3tables.Xc = c->d_Xc; c->w3tables.Y = c->d_Y; c->w3tables.S = c->d_S; c->w3tables.AY = c->d_AY;
    c->w3tables.vop = dvop; c->w3tables.lam = dlam; c->w3tables.pmap = dpm; c->w3tables.dense = dd3;
    // persistent form: as many workgroups as are resident at once, each wave walks a contiguous range of clusters
    int per_cu = 2;
    const int cus = cu_count(c);
    if (full) { if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_cluster_assemble_w3<true>, 256, 0) != hipSuccess) per_cu = 2; }
    else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_cluster_assemble_w3<false>, 256, 0) != hipSuccess) per_cu = 2;
    if (const char *e = std::getenv("CLRS_W3_WGS_PER_CU")) per_cu = std::max(1, std::atoi(e));     // diagnostic: waves per SIMD
    if (std::getenv("CLRS_DEBUG")) std::fprintf(stderr, "[clrs] k_cluster_assemble_w3<%s>: %zu clusters, %zu blocks, %d workgroups per CU x %d CUs\n", full ? "full" : "general", w.cl.size(), b3.size(), per_cu, cus);
    s.kind = STEP_ASSEMBLE_W3;
    s.d0 = dcb; s.d1 = db3; s.src = &c->w3tables; s.bytes = 0;
    s.aux0 = (int)std::min<i64>(((i64)w.cl.size() + 3) / 4, (i64)std::max(per_cu, 1) * cus);
    s.aux1 = (int)b3.size();
    return 0;
}

static int plan_w2(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    auto &w = B.w2;
    if (w.cl.empty()) return 0;
    int *dpm, *day; double *dlam;
    CLRS_RET(upload(c, w.pmap, &dpm)); CLRS_RET(upload(c, w.ay, &day)); CLRS_RET(upload(c, w.lam, &dlam));
    for (size_t i2 = 0; i2 < w.bl.size(); i2++) { w.bl[i2].lam = dlam + w.boff[i2]; w.bl[i2].ay = day + w.boff[i2]; }
    for (size_t i2 = 0; i2 < w.cl.size(); i2++) w.cl[i2].pmap = dpm + w.cl_pm[i2];
    W2Cluster *dwc; W2Block *dwb;
    CLRS_RET(upload(c, w.cl, &dwc)); CLRS_RET(upload(c, w.bl, &dwb));
    c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y; c->ftables.stat = c->d_static; c->ftables.AY = c->d_AY;
    Step s;
    s.kind = STEP_ASSEMBLE_W2;
    bool use_w3 = g_cfg_wave3_assemble && w.ut <= 2;
    // k_cluster_assemble_w3 takes the A_Y position of vector u as ay_base + u (terms of a block consecutive in A_Y, in vector order)
    for (size_t i2 = 0; i2 < w.bl.size() && use_w3; i2++)
        if (w.bl[i2].kind == 0)
            for (int u = 0; u < w.cl[w.bl_cl[i2]].P; u++)
                if (w.ay[w.boff[i2] + u] != w.ay[w.boff[i2]] + u) { use_w3 = false; break; }
    s.d0 = dwc; s.d1 = dwb; s.src = &c->ftables; s.n = (i64)w.cl.size(); s.nmax = w.ut;
    bool full = w.ut <= 2;
    for (size_t i2 = 0; i2 < w.bl.size() && full; i2++) if (w.bl[i2].kind == 0 && w.bl[i2].n != 16) full = false;
    for (size_t i2 = 0; i2 < w.cl.size() && full; i2++) if (w.cl[i2].P != 16 * w.ut) full = false;
    s.grid = full ? 1 : 0;
    s.bytes = (size_t)4 * 2 * 17 * 16 * w.ut * sizeof(double);
    if (use_w3) CLRS_RET(plan_w3(c, B, s, full, dpm, dlam));
    c->p_assemble.steps.push_back(s);
    return raise_lds_limit((const void *)k_cluster_assemble_w2<4, false>, s.bytes);
}

static int plan_w1(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    auto &w = B.w1;
    if (w.cl.empty()) return 0;
    int *dpm, *day; double *dlam;
    CLRS_RET(upload(c, w.pmap, &dpm)); CLRS_RET(upload(c, w.ay, &day)); CLRS_RET(upload(c, w.lam, &dlam));
    for (size_t i2 = 0; i2 < w.bl.size(); i2++) { w.bl[i2].pmap = dpm + w.ioff[i2]; w.bl[i2].ay = day + w.ioff[i2]; w.bl[i2].lam = dlam + w.ioff[i2]; }
    // block table with a fixed number of slots per cluster (the kernel fetches slot `wave` without knowing the cluster yet)
    std::vector<WBlock> table(w.cl.size() * (size_t)w.maxblocks);
    std::memset(table.data(), 0, table.size() * sizeof(WBlock));
    for (size_t ci = 0; ci < w.cl.size(); ci++)
        for (int sl = 0; sl < w.maxblocks; sl++)
            table[ci * w.maxblocks + sl] = w.bl[w.cl_first[ci] + (sl < w.cl[ci].nblk ? sl : 0)];
    WCluster *dwc; WBlock *dwb;
    CLRS_RET(upload(c, w.cl, &dwc)); CLRS_RET(upload(c, table, &dwb));
    c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y; c->ftables.stat = c->d_static; c->ftables.AY = c->d_AY;
    CLRS_RET(ensure_stamps(c));
    Step s;
    s.kind = STEP_ASSEMBLE_W1;
    s.grid = (int)w.cl.size(); s.d0 = dwc; s.d1 = dwb; s.src = &c->ftables; s.n = w.nwaves; s.nmax = w.ut; s.dst = (void *)(intptr_t)w.maxblocks;
    s.bytes = (size_t)w.nwaves * w.cluster_doubles * sizeof(double);
    c->p_assemble.steps.push_back(s);
    return raise_lds_limit(w.ut <= 2 ? (const void *)k_cluster_assemble_w1<2> : w.ut <= 4 ? (const void *)k_cluster_assemble_w1<4> : (const void *)k_cluster_assemble_w1<8>, s.bytes);
}

static int plan_fused(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &B) {
    const auto &f = B.fu;
    if (f.cl.empty()) return 0;
    FCluster *dfc; FBlock *dfb;
    CLRS_RET(upload(c, f.cl, &dfc)); CLRS_RET(upload(c, f.bl, &dfb));
    c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y; c->ftables.stat = c->d_static;
    c->ftables.tL = B.d_tL; c->ftables.tR = B.d_tR; c->ftables.tlam = B.d_tlam;
    c->ftables.ayL = c->d_ayL; c->ftables.ayR = c->d_ayR; c->ftables.AY = c->d_AY;
    CLRS_RET(ensure_stamps(c));
    Step s;
    s.kind = STEP_FUSED_ASSEMBLE;
    s.grid = (int)f.cl.size(); s.d0 = dfc; s.d1 = dfb; s.src = &c->ftables; s.bytes = f.lds; s.nmax = f.nmax;
    c->p_assemble.steps.push_back(s);
    CLRS_RET(raise_lds_limit((const void *)k_cluster_assemble, f.lds));
    if (f.sum.empty()) return 0;
    SSlabSum *dss;
    CLRS_RET(upload(c, f.sum, &dss));
    Step s2;
    s2.kind = STEP_SUM_S_SLABS; s2.grid = (int)f.sum.size(); s2.d0 = dss; s2.n = 0;
    for (const SSlabSum &ss : f.sum) s2.n = std::max<i64>(s2.n, ss.len);
    c->p_assemble.steps.push_back(s2);
    return 0;
}

// plan: factor (src/solver.jl:1244-1279), split like the reference's timings
static int plan_factor(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int J = c->J, N = c->N, NB = c->NB;
    int maxP = 0, maxn = 0;
    for (int j = 0; j < J; j++) maxP = std::max(maxP, c->P[j]);
    for (int b = 0; b < NB; b++) maxn = std::max(maxn, c->blk[b].n);
    c->fused_fs = g_cfg_fused_factor && J > 0 && maxP <= 128;
    c->fused_q = g_cfg_fused_factor && N > 0 && N <= 128;
    c->fused_x = g_cfg_fused_factor && NB > 0 && maxn <= 128;
    CLRS_RET(dmalloc(c, &c->d_dinvS, c->xlen)); CLRS_RET(dmalloc(c, &c->d_dinvQ, N));
    bool q_from_factor = false;
    if (c->fused_fs) {
        std::vector<CFactor> cf(J);
        size_t lds = 0;
        c->q_slabs = c->fused_q && J <= 4096;
        for (int j = 0; j < J; j++) {
            const int P = c->P[j], P16 = (P + 15) & ~15, lda = P16 + 2;
            CFactor &f = cf[j];
            f.S = c->d_S + c->Soff[j]; f.B = c->d_B + c->coff[j]; f.LB = c->d_LB + c->coff[j]; f.dinv = c->d_dinvS + c->coff[j];
            f.P = P; f.N = N; f.ldb = (int)c->xlen; f.code = j + 1;
            const int room = (LDS_BUDGET_DOUBLES - lds_square(P)) / lda;      // columns of B that fit beside L
            f.nc = std::max(1, std::min(std::max(N, 1), room));
            if (f.nc < N || room < ((N + 15) & ~15)) c->q_slabs = false;      // the Gram matrix needs all of LinvB_j (+ tile padding) resident
            lds = std::max(lds, (size_t)(lds_square(P) + lda * (N > 0 ? std::max(f.nc, c->q_slabs ? ((N + 15) & ~15) : 0) : 0)) * sizeof(double));
        }
        if (c->q_slabs) CLRS_RET(dmalloc(c, &c->d_Qslabs, (i64)J * N * N));
        for (int j = 0; j < J; j++) cf[j].Qslab = c->q_slabs ? c->d_Qslabs + (i64)j * N * N : nullptr;
        CFactor *dcf;
        CLRS_RET(upload(c, cf, &dcf));
        Step s;
        s.kind = STEP_CLUSTER_FACTOR; s.grid = J; s.d0 = dcf; s.dst = c->d_info; s.bytes = lds;
        c->p_cholS.steps.push_back(s);      // Cholesky of S_j and L_j^-1 B_j in one launch: the LinvB timing slot stays 0
        CLRS_RET(raise_lds_limit((const void *)k_cluster_factor, lds));
    } else if (g_cfg_factor_aug && g_cfg_potrf_levels && J >= 1 && N > 0 && N <= 512 && *std::min_element(c->P.begin(), c->P.end()) > POTRF_NB) {
        // large clusters, a few free variables: L_j, L_j^-1 B_j and the cluster's share of Q from ONE blocked factorisation of
        // [S_j .; B_j^T 0] each (k_chol_pack), all clusters in the same launches; several clusters: the shares summed in cluster order
        if (J > 1) CLRS_RET(dmalloc(c, &c->d_Qslabs, (i64)J * N * N));
        Step ms; ms.kind = STEP_MEMSET_INFO;
        c->p_cholS.steps.push_back(ms);
        std::vector<PotrfJob> pj;
        std::vector<Step> unpack;
        for (int j = 0; j < J; j++) {
            const int P = c->P[j], P64 = (P + 63) & ~63, na = P64 + N;
            CholAugDesc ad;
            std::memset(&ad, 0, sizeof(ad));
            CLRS_RET(dmalloc(c, &ad.Aug, (i64)na * na));
            ad.S = c->d_S + c->Soff[j]; ad.B = c->d_B + c->coff[j]; ad.LB = c->d_LB + c->coff[j];
            ad.Q = J > 1 ? c->d_Qslabs + (i64)j * N * N : c->d_Q;
            ad.P = P; ad.P64 = P64; ad.N = N; ad.ldb = (int)c->xlen;
            c->chol_aug.push_back(ad);
            Step ps;
            ps.kind = STEP_CHOL_PACK; ps.n = (i64)c->chol_aug.size() - 1; ps.grid = (int)std::min<i64>(((i64)na * na + 255) / 256, 8192);
            c->p_cholS.steps.push_back(ps);
            PotrfJob job{ad.Aug, na, na, j + 1};
            job.stop = P64 / 64;
            pj.push_back(job);
            Step us = ps;
            us.kind = STEP_CHOL_UNPACK; us.grid = (int)std::min<i64>(((i64)P * P + (i64)P * N + (i64)N * N + 255) / 256, 8192);
            unpack.push_back(us);
        }
        CLRS_RET(plan_potrf(c, c->p_cholS, pj));
        for (const Step &us : unpack) c->p_cholS.steps.push_back(us);
        q_from_factor = true;
    } else {
        std::vector<PotrfJob> pj;
        std::vector<TrsmJob> tj;
        Step ms; ms.kind = STEP_MEMSET_INFO;
        c->p_cholS.steps.push_back(ms);
        for (int j = 0; j < J; j++) {
            pj.push_back(PotrfJob{c->d_S + c->Soff[j], c->P[j], c->P[j], j + 1});
            if (N > 0) tj.push_back(TrsmJob{c->d_S + c->Soff[j], c->P[j], c->P[j], c->d_LB + c->coff[j], (int)c->xlen, N});
        }
        CLRS_RET(plan_potrf(c, c->p_cholS, pj));
        if (N > 0) {
            add_memcpy(c->p_linvB, c->d_LB, c->d_B, sizeof(double) * (size_t)(c->xlen * N));
            CLRS_RET(plan_trsm(c, c->p_linvB, tj, 0));
        }
    }
    if (N <= 0) return 0;
    if (q_from_factor || c->q_slabs) {
        // Q came out of the factorisation of S (k_chol_unpack, k_cluster_factor); one share per cluster: they are added up in cluster order
        if (c->q_slabs || J > 1) {
            Step s;
            s.kind = STEP_SUM_SLABS;
            c->p_Q.steps.push_back(s);
        }
    } else if (N <= 16 && c->xlen >= 512) {
        Step s;
        s.kind = STEP_GRAM_SMALL;   // few free variables, many constraints: one reduction per entry of Q
        c->p_Q.steps.push_back(s);
    } else {
        std::vector<GemmDesc> gq;   // Q = LB^T LB  (vcat + matmul, src/solver.jl:1268-1269)
        gq.push_back(mk_gemm(1, 0, N, N, (int)c->xlen, 1.0, c->d_LB, (int)c->xlen, c->d_LB, (int)c->xlen, 0.0, c->d_Q, N));
        CLRS_RET(add_gemm_stage(c, c->p_Q, gq));
    }
    if (!c->fused_q) {
        std::vector<PotrfJob> qj;
        qj.push_back(PotrfJob{c->d_Q, N, N, J + 1});
        return plan_potrf(c, c->p_cholQ, qj);
    }
    std::vector<SmallPotrf> sp(1);
    std::memset(&sp[0], 0, sizeof(SmallPotrf));
    sp[0].in_off = 0; sp[0].out_off = 0; sp[0].dinv = c->d_dinvQ; sp[0].n = N; sp[0].ldin = N; sp[0].ldout = N; sp[0].code = J + 1;
    sp[0].nslabs = 1; sp[0].slab_stride = 0;
    SmallPotrf *dsp;
    CLRS_RET(upload(c, sp, &dsp));
    Step s;
    s.kind = STEP_SMALL_POTRF; s.grid = 1; s.d0 = dsp; s.dst = c->d_info; s.n = 1; s.bytes = (size_t)lds_square(N) * sizeof(double);
    c->p_cholQ.steps.push_back(s);
    if (c->q_slabs) {   // single-GPU path: sum the slabs while loading Q, no separate reduction launch
        sp[0].nslabs = J; sp[0].slab_stride = (i64)N * N;
        CLRS_RET(upload(c, sp, &dsp));
        s.d0 = dsp; s.n = 2;
        c->p_cholQ_slabs.steps.push_back(s);
    }
    return s.bytes > 64 * 1024 ? raise_lds_limit((const void *)k_small_potrf, lds_square(128) * sizeof(double)) : 0;
}

// ONE small cluster: the whole factorisation stage in one launch of one workgroup (measured: 1.6-1.9 us per step saved on
// polyopt 2d = 40 and delsarte(3,10)).  "factor_small" = 2 also takes 2-4 clusters, one wave per cluster -- slower than
// k_cluster_factor + k_small_potrf on cohnelkies(8,15) (23.4 us against 12.4 + 8.0): a single wave per 32 x 32 cluster is
// latency bound on its own dependent chains, the workgroup-per-cluster kernels overlap four waves on them.
static int plan_factor_small(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int J = c->J, N = c->N;
    if (!(g_cfg_factor_small && c->fused_fs && c->fused_q && N > 0 && (J == 1 || (g_cfg_factor_small == 2 && J <= 4)) && !c->p_cholQ_slabs.steps.empty())) return 0;
    bool ok = N <= 64;
    for (int j = 0; j < J; j++) ok = ok && c->P[j] <= 64;
    const size_t need = factor_small_lds_doubles(c->P.data(), J, N) * sizeof(double);
    if (!ok || need > 150 * 1024) return 0;
    std::memset(&c->fsmall, 0, sizeof(c->fsmall));
    const double *Ssrc[4], *Bsrc[4];
    for (int j = 0; j < J; j++) {
        c->fsmall.c[j].S = c->d_S + c->Soff[j]; c->fsmall.c[j].LB = c->d_LB + c->coff[j]; c->fsmall.c[j].dinv = c->d_dinvS + c->coff[j];
        c->fsmall.c[j].P = c->P[j]; c->fsmall.c[j].code = j + 1;
        Ssrc[j] = c->d_S + c->Soff[j]; Bsrc[j] = c->d_B + c->coff[j];
    }
    c->fsmall.Q = c->d_Q; c->fsmall.dinvQ = c->d_dinvQ; c->fsmall.J = J; c->fsmall.N = N; c->fsmall.ldb = (int)c->xlen; c->fsmall.codeQ = J + 1;
    if (!factor_small_jobs(c->fsmall_jobs, c->fsmall, Ssrc, Bsrc)) return 0;
    Step s;
    s.kind = STEP_FACTOR_SMALL; s.bytes = need;
    c->p_factor_small.steps.push_back(s);
    const void *kernels[] = {(const void *)k_factor_small<8>, (const void *)k_factor_small<16>, (const void *)k_factor_small<24>, (const void *)k_factor_small<32>,
                             (const void *)k_factor_small<48>};
    for (const void *k : kernels)
        CLRS_RET(raise_lds_limit(k, need));
    return 0;
}

// plan: solve (src/solver.jl:1527-1582)
static int plan_solve(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int J = c->J, N = c->N;
    std::vector<TrsmJob> tj;
    for (int j = 0; j < J; j++) tj.push_back(TrsmJob{c->d_S + c->Soff[j], c->P[j], c->P[j], c->d_t + c->coff[j], (int)c->xlen, 1});
    CSolve *dcs = nullptr;
    size_t lds_cs = 0;
    if (c->fused_fs) {
        std::vector<CSolve> cs(J);
        for (int j = 0; j < J; j++) {
            cs[j].L = c->d_S + c->Soff[j]; cs[j].dinv = c->d_dinvS + c->coff[j]; cs[j].LB = c->d_LB + c->coff[j];
            cs[j].off = c->coff[j]; cs[j].P = c->P[j]; cs[j].N = N; cs[j].ldb = (int)c->xlen; cs[j].pad = 0;
            lds_cs = std::max(lds_cs, (size_t)(lds_square(c->P[j]) + ((c->P[j] + 15) & ~15) + 2) * sizeof(double));
        }
        CLRS_RET(upload(c, cs, &dcs));
        CLRS_RET(raise_lds_limit((const void *)k_cluster_solve_fwd, lds_cs)); CLRS_RET(raise_lds_limit((const void *)k_cluster_solve_bwd, lds_cs));
        Step s;
        s.kind = STEP_CSOLVE_FWD; s.grid = J; s.d0 = dcs; s.bytes = lds_cs;
        c->p_fwd.steps.push_back(s);                                                        // t_j = L_j^-1 rhs_x[j]   (:1538)
    } else {
        add_memcpy(c->p_fwd, c->d_t, c->d_rhsx, sizeof(double) * (size_t)c->xlen);
        CLRS_RET(plan_trsm(c, c->p_fwd, tj, 0, true));
    }
    if (N > 0) {
        if (c->fused_fs) {
            Step s;
            s.kind = STEP_GEMV_T;                                                           // u = LB^T t             (:1546)
            c->p_fwd.steps.push_back(s);
        } else {
            std::vector<GemmDesc> g;
            g.push_back(mk_gemm(1, 0, N, 1, (int)c->xlen, 1.0, c->d_LB, (int)c->xlen, c->d_t, (int)c->xlen, 0.0, c->d_u, N));
            CLRS_RET(add_gemm_stage(c, c->p_fwd, g));
        }
        if (c->fused_q) {
            Step s;
            s.kind = STEP_Q_SOLVE; s.bytes = (size_t)(lds_square(N) + ((N + 15) & ~15) + 2) * sizeof(double);   // dy = Q^-1 (rhs_y - u)  (:1550-1558)
            c->p_bwd.steps.push_back(s);
            CLRS_RET(raise_lds_limit((const void *)k_q_solve, s.bytes));
        } else {
            Step s;
            s.kind = STEP_SUB; s.dst = c->d_dy; s.src = c->d_rhsy; s.d0 = c->d_u; s.n = N;
            c->p_bwd.steps.push_back(s);
            std::vector<TrsmJob> qj;
            qj.push_back(TrsmJob{c->d_Q, N, N, c->d_dy, N, 1});
            CLRS_RET(plan_trsm(c, c->p_bwd, qj, 0)); CLRS_RET(plan_trsm(c, c->p_bwd, qj, 1));
        }
        if (!c->fused_fs) {
            std::vector<GemmDesc> g2;                                                       // t += LB dy             (:1568-1569)
            g2.push_back(mk_gemm(0, 0, (int)c->xlen, 1, N, 1.0, c->d_LB, (int)c->xlen, c->d_dy, N, 1.0, c->d_t, (int)c->xlen));
            CLRS_RET(add_gemm_stage(c, c->p_bwd, g2));
        }
    }
    if (!c->fused_fs) return plan_trsm(c, c->p_bwd, tj, 1, true);
    Step s;
    s.kind = STEP_CSOLVE_BWD; s.grid = J; s.d0 = dcs; s.bytes = lds_cs;                 // dx_j = L_j^-T (t_j + LB_j dy)  (:1566-1573)
    c->p_bwd.steps.push_back(s);
    return 0;
}

// the one-launch forms of the solve stage: a handful of small clusters in one workgroup, or three launches with u = LinvB^T t inside the Q solve
static int plan_solve_small(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int J = c->J, N = c->N;
    i64 solve_doubles = (i64)N * N + c->xlen * N;                     // operands of one solve: L_j, LinvB, L_Q
    for (int j = 0; j < J; j++) solve_doubles += (i64)c->P[j] * c->P[j];
    if (!(c->fused_fs && (c->fused_q || N == 0) && J <= 8 && c->xlen <= 1024 && solve_doubles <= g_cfg_solve_small_max)) {
        // single-GPU solve in three launches: the u = LinvB^T t product moves into the Q-solve kernel
        if (c->fused_fs && c->fused_q && c->xlen <= 4096) {
            c->p_solve_all.steps.push_back(c->p_fwd.steps[0]);            // k_cluster_solve_fwd
            Step q = c->p_bwd.steps[0];                                   // k_q_solve
            q.n = 1;
            c->p_solve_all.steps.push_back(q);
            c->p_solve_all.steps.push_back(c->p_bwd.steps.back());        // k_cluster_solve_bwd
        }
        return 0;
    }
    int maxP16 = (N + 15) & ~15;
    for (int j = 0; j < J; j++) maxP16 = std::max(maxP16, (c->P[j] + 15) & ~15);
    Step s = c->p_fwd.steps[0];                                   // reuses the CSolve table
    s.kind = STEP_SOLVE_SMALL; s.n = maxP16;
    s.bytes = (size_t)((maxP16 + 2) * maxP16 + 2 * maxP16 + 2 + ((c->xlen + 15) & ~15) + 2 * ((N + 15) & ~15) + 16) * sizeof(double);
    CLRS_RET(raise_lds_limit((const void *)k_solve_small, s.bytes));
    const size_t need2 = solve_small2_lds_doubles(c->P.data(), J, N, c->xlen) * sizeof(double);
    bool fits2 = g_cfg_solve_small2 && need2 <= 150 * 1024;
    if (fits2) {
        HIPCHECK(hipMemcpy(c->solve8.d, s.d0, sizeof(CSolve) * J, hipMemcpyDeviceToHost));
        for (int ph = 0; ph < 3 && fits2; ph++) {
            clrs_ctx::SolveSmall2 &q = c->ss2[ph];
            q.ok = solve_small2_jobs(q.jobs, c->solve8.d, J, c->d_Q, c->d_dinvQ, N, c->xlen, c->d_LB, q.rx_job, q.ry_job, ph, c->d_t, c->d_u);
            fits2 = q.ok;
        }
    }
    if (fits2) {                                                // everything resident at once: the latency-first variant
        Step s1 = s, s2 = s;
        s.aux0 = 2; s.bytes = need2;
        s1.aux0 = 3; s1.bytes = need2; s2.aux0 = 4; s2.bytes = need2;
        c->p_fwd_small.steps.push_back(s1);
        c->p_bwd_small.steps.push_back(s2);
#define CLRS_SS2_KERNELS(NJ) (const void *)k_solve_small2<NJ, 0>, (const void *)k_solve_small2<NJ, 1>, (const void *)k_solve_small2<NJ, 2>
        const void *kernels[] = {CLRS_SS2_KERNELS(8), CLRS_SS2_KERNELS(16), CLRS_SS2_KERNELS(24), CLRS_SS2_KERNELS(32), CLRS_SS2_KERNELS(48)};
#undef CLRS_SS2_KERNELS
        for (const void *k : kernels)
            CLRS_RET(raise_lds_limit(k, s.bytes));
    }
    c->p_solve_all.steps.push_back(s);
    return 0;
}

// plan: Cholesky of X blocks (src/solver.jl:388-399)
static int plan_chol_x(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int NB = c->NB;
    if (c->fused_x) {
        std::vector<SmallPotrf> sp(NB);
        size_t lds = 0;
        for (int b = 0; b < NB; b++) {
            std::memset(&sp[b], 0, sizeof(SmallPotrf));
            sp[b].in_off = c->blk[b].xyoff; sp[b].out_off = c->blk[b].xyoff; sp[b].dinv = nullptr;
            sp[b].n = c->blk[b].n; sp[b].ldin = c->blk[b].n; sp[b].ldout = c->blk[b].n; sp[b].code = b + 1; sp[b].nslabs = 1;
            lds = std::max(lds, (size_t)lds_square(c->blk[b].n) * sizeof(double));
        }
        SmallPotrf *dsp;
        CLRS_RET(upload(c, sp, &dsp));
        Step s;
        s.kind = STEP_SMALL_POTRF; s.grid = NB; s.d0 = dsp; s.dst = c->d_info + 1; s.n = 0; s.bytes = lds;
        c->p_cholX.steps.push_back(s);
        return lds > 64 * 1024 ? raise_lds_limit((const void *)k_small_potrf, lds_square(128) * sizeof(double)) : 0;
    }
    std::vector<PotrfJob> pj;
    Step ms; ms.kind = STEP_MEMSET_INFO; ms.dst = c->d_info + 1;
    c->p_cholX.steps.push_back(ms);
    for (int b = 0; b < NB; b++) pj.push_back(PotrfJob{c->d_X + c->blk[b].xyoff, c->blk[b].n, c->blk[b].n, b + 1});
    CLRS_RET(plan_potrf(c, c->p_cholX, pj, c->d_info + 1));
    if (NB == 0) return 0;
    std::vector<PotrfDesc> zd;      // strict upper triangles -> 0, the output format of approx_cholesky! (src/tools.jl:100-105)
    i64 maxnn = 0;
    for (int b = 0; b < NB; b++) {
        zd.push_back(PotrfDesc{c->d_X + c->blk[b].xyoff, c->blk[b].n, c->blk[b].n, 0, 0});
        maxnn = std::max(maxnn, (i64)c->blk[b].n * c->blk[b].n);
    }
    PotrfDesc *dz;
    CLRS_RET(upload(c, zd, &dz));
    Step zs;
    zs.kind = STEP_ZERO_UPPER; zs.grid = NB; zs.d0 = dz; zs.n = maxnn;
    c->p_cholX.steps.push_back(zs);
    return 0;
}

// ---- algorithmic work counters (SURVEY.md section 8d) ----
static int count_work(clrs_ctx *c, const clrs_sdp_desc *, CtxBuild &) {
    const int N = c->N;
    for (const BlockInfo &k : c->blk) {
        double n = k.n;
        if (k.kind == 0) {
            double U = 0.5 * (k.URt + k.ULt), m = k.m, dl = k.delta, nt = (double)(k.t1 - k.t0);
            c->cnt_bytes += 8.0 * (2 * n * n + dl * U);
            c->cnt_flops += (m == 1) ? 2.0 * (2 * n * n * U + 2 * n * U * U) + U * U : 2.0 * m * (2 * n * dl * U / m + 2 * U * dl * U / m) + nt * nt;
        } else {
            double Pc = k.cnt;
            c->cnt_bytes += 8.0 * (Pc * n * n + 2 * n * n);
            c->cnt_flops += Pc * 6 * n * n * n + Pc * Pc * n * n;
        }
    }
    for (int j = 0; j < c->J; j++) {
        double Pj = c->P[j];
        c->cnt_bytes += 8.0 * Pj * Pj;
        c->cnt_factor_flops += Pj * Pj * Pj / 3 + Pj * Pj * N + 2.0 * N * N * Pj;
        c->cnt_solve_flops += 2 * Pj * Pj + 4 * Pj * N;
    }
    c->cnt_factor_flops += (double)N * N * N / 3;
    c->cnt_solve_flops += 2.0 * N * N;
    return 0;
}

// the stages in the order they run.  It is the order of the device allocations too: a stage that moves changes c->allocs
typedef int (*CtxStage)(clrs_ctx *, const clrs_sdp_desc *, CtxBuild &);
static const CtxStage CTX_STAGES[] = {ctx_device_objects, ctx_sizes, ctx_blocks, ctx_arenas, ctx_buffers, ctx_term_tables, select_w5, select_w4, select_w1_w2,
                                      select_fused, ctx_ay_tables, plan_assemble_general, plan_w5, plan_w4, plan_w2, plan_w1, plan_fused, plan_factor,
                                      plan_factor_small, plan_solve, plan_solve_small, plan_chol_x, count_work};

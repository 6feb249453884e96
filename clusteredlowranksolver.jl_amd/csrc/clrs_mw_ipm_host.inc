// clrs_mw_ipm_host.inc -- host side of the multi-word interior-point iteration (state, launches, C ABI); included by clrs_mw.hip
// after the context type.  The kernels are in clrs_mw_ipm.hip.h.
// =====================================================================================================================
// host
// =====================================================================================================================
struct MwIpm {
    MwIpmDev d = {};
    bool ready = false;
    int iter = 0;
    bool xy_with_tail = false;         // <X,Y> of the new iterate travelled with the previous iteration's objectives (one launch, one record)
    bool upd_recorded = false;         // E_UPD was recorded behind the last update (event mode); else mw_ipm_finish records it
    int sync_seq = 0;                  // enqueued iterations of this context's life (never reset, unlike iter): the value of the side stream's mark (k_mwi_mark)
    bool global_set = false;      // clrs_mw_ipm_set_global has sized the gather buffers for the current world
    int gs_world = 0;
    bool forked = false, tail_pending = false;      // S has been ordered behind M once; an iteration's objectives / record are still to be enqueued
    bool frozen = false;          // flags[6] may be set on the device (a clrs_mw_ipm_solve has ended)
    int held_refine_bits = 0;     // clrs_mw_ipm_iterate: refine_bits of the last record, applied in front of the NEXT BUT ONE enqueue -- as in clrs_mw_ipm_solve, whose host reads
                                  // the record of iteration k after iteration k + 1 is enqueued (both loops then switch at the same iteration: bit-identical iterates)
    bool aff_ok = false;          // the corrector's right-hand side as rhs0 + mu_c tau, with beta_c / mu_c formed on the side stream meanwhile (mw_ipm_enqueue_body)
    double *AX = nullptr;         // [T] K limbs: the pairings w^T X^-1 v of the assembly (MwDev::AX), kept when aff_ok
    int kf_now = 0;               // limbs of the factor stage and of the solve's products in the iterations enqueued from now on (MwDev::kf): the context's reduced count
                                  // (clrs_mw_ctx::kf_low) from clrs_mw_ipm_init / _set until a record reports a first pass too weak for it (mw_ipm_note_record), then K
    double *h_rec = nullptr;      // pinned, two records: iteration k reports into record k & 1
    double *d_rec = nullptr;      // device, two records
    size_t sm_Z = 0, sm_Zi = 0, sm_step = 0;
    int zs = MWI_ZS;              // workgroups per block of k_mwi_Zi
    int zt = MW_PT;               // ... and their threads (clrs_mw_zi_panels.h)
    int zs_step = MWI_ZS;         // column panels per (block, which) of k_mwi_step's congruences
    size_t sm_bmm = 0;            // LDS of k_mwi_bmm: eight rows and eight columns of K limbs over the largest block side
    bool z_tiled = false;         // blocks with sides beyond 24: the products of X^-1 (...) as tiled launches (k_mwi_bmm)
    size_t maxn_inv = 0;          // largest block with an inverse factor
    bool lds_ZL = false, step_w_lds = true, step_inv = false, y_with_x = false, any_xinv = false, any_xsub = false;
    // side stream: what depends on the iterate and the assembly only runs beside the factorisations (mw_ipm_enqueue)
    hipStream_t side = nullptr;
    enum { E_ASM, E_PREP, E_UPD, E_REC0, E_REC1, E_COUNT };
    hipEvent_t ev[E_COUNT] = {};
    ~MwIpm() {
        if (h_rec) (void)hipHostFree(h_rec);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
};

static void mw_ipm_free(clrs_mw_ctx *c) {
    delete c->ipm;
    c->ipm = nullptr;
}

extern "C" int clrs_mw_ipm_create_ex(clrs_mw_ctx *c, const clrs_ipm_data *data, int data_limbs);
extern "C" int clrs_mw_ipm_create(clrs_mw_ctx *c, const clrs_ipm_data *data) { return clrs_mw_ipm_create_ex(c, data, 1); }

// data->C, c, b planar with `data_limbs` planes (at most the data limbs the context was created with)
extern "C" int clrs_mw_ipm_create_ex(clrs_mw_ctx *c, const clrs_ipm_data *data, int data_limbs) {
    if (!c || !data) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (data_limbs < 1 || data_limbs > c->DK) return mw_fail(CLRS_ERR_INVALID, "data limbs of the objective exceed those of the context");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    const int K = c->K, N = q.N, NB = q.NB;
    if (NB == 0) return mw_fail(CLRS_ERR_INVALID, "no PSD blocks");
    if (!c->ipm) c->ipm = new MwIpm();
    MwIpm *st = c->ipm;
    MwIpmDev &p = st->d;
    int rc;
    if (!st->ready) {
        double **xy[] = {&p.X, &p.Y, &p.dX, &p.dY, &p.R, &p.Xc, &p.Pm};
        for (double **b : xy) if ((rc = mw_dmalloc(c, b, q.xylen * K))) return rc;
        double **xs[] = {&p.x, &p.dx, &p.d, &p.rhsx};
        for (double **b : xs) if ((rc = mw_dmalloc(c, b, q.xlen * K))) return rc;
        double **ys[] = {&p.y, &p.dy, &p.pv};
        for (double **b : ys) if ((rc = mw_dmalloc(c, b, (i64)N * K))) return rc;
        if ((rc = mw_dmalloc(c, &p.coef, q.T * K)) || (rc = mw_dmalloc(c, &p.dtr, q.xlen * K))) return rc;
        p.wBn = 0; p.wB = nullptr;
        if (c->maxTb >= 128) {                              // blocks with hundreds of terms: coefficient times right vector once per term (k_mwi_wB)
            int maxn_lr = 1;
            for (auto &k : c->blk) if (k.kind == 0) maxn_lr = std::max(maxn_lr, k.n);
            p.wBn = maxn_lr;
            if ((rc = mw_dmalloc(c, &p.wB, q.T * (i64)maxn_lr * K))) return rc;
        }
        if ((rc = mw_dmalloc(c, &p.Yi, q.xylen * K)) || (rc = mw_dmalloc(c, &p.Zs, q.xylen * K))) return rc;
        if ((rc = mw_dmalloc(c, &p.Zt, q.xylen * K))) return rc;
        { double *t3 = nullptr; if ((rc = mw_dmalloc(c, &t3, (NB + 1) / 2 + 1))) return rc; p.zcnt = (int *)t3; }
        { double *t2 = nullptr; if ((rc = mw_dmalloc(c, &t2, (NB + 1) / 2 + 1))) return rc; p.yfail = (int *)t2; }
        if ((rc = mw_dmalloc(c, &p.sc, (i64)MSC_COUNT * K))) return rc;
        if ((rc = mw_dmalloc(c, &p.part, 5LL * NB * K))) return rc;
        if ((rc = mw_dmalloc(c, &p.eig, 2LL * NB))) return rc;
        if ((rc = mw_dmalloc(c, &p.Wd, 2LL * q.xylen))) return rc;
        { double *t4 = nullptr; if ((rc = mw_dmalloc(c, &t4, NB + 1))) return rc; p.wcnt = (int *)t4; }
        if ((rc = mw_dmalloc(c, &st->d_rec, 2 * MREC_COUNT))) return rc;
        p.rec = st->d_rec;
        double *tmp = nullptr;
        if ((rc = mw_dmalloc(c, &tmp, 4))) return rc;
        p.fmax = (unsigned long long *)tmp;
        if ((rc = mw_dmalloc(c, &tmp, 4))) return rc;
        p.flags = (int *)tmp;
        if ((rc = mw_dmalloc(c, &tmp, 4))) return rc;
        p.sync = (int *)tmp;
        p.tau = p.ttau = p.utau = nullptr;
        p.klow = K;
        p.hop = c->chain_hop;
        std::vector<int> row_clu((size_t)q.xlen);
        for (int j = 0; j < q.J; j++)
            for (int r = 0; r < c->clu[j].P; r++) row_clu[c->clu[j].coff + r] = j;
        if ((rc = mw_upload(c, row_clu, &p.row_clu))) return rc;
        double *dC, *dc, *db;
        if ((rc = mw_dmalloc(c, &dC, q.xylen * c->DK)) || (rc = mw_dmalloc(c, &dc, q.xlen * c->DK)) || (rc = mw_dmalloc(c, &db, (i64)N * c->DK))) return rc;
        p.C = dC; p.c = dc; p.b = db;
        MWCHECK(hipHostMalloc((void **)&st->h_rec, sizeof(double) * 2 * MREC_COUNT, hipHostMallocDefault));
        MWCHECK(hipStreamCreateWithFlags(&st->side, hipStreamNonBlocking));
        // the events between the two streams order work on ONE device: no system-scope fence (write-back and invalidation of the caches for the
        // host's sake) when they complete; the events of the record copies (E_REC*) are what the host waits on and keep it
        for (int e = 0; e < MwIpm::E_COUNT; e++)
            MWCHECK(hipEventCreateWithFlags(&st->ev[e], e < MwIpm::E_REC0 ? (hipEventDisableTiming | hipEventDisableSystemFence) : hipEventDisableTiming));
        p.Ktot = 0;
        size_t maxn = 0;
        for (auto &k : c->blk) { p.Ktot += k.n; maxn = std::max(maxn, (size_t)k.n); }
        const size_t lim = MW_LDS_MAX / sizeof(double), nnK = maxn * maxn * K;
        if (nnK > lim) return mw_fail(CLRS_ERR_INVALID, "device-resident multi-word iteration needs PSD blocks that fit in LDS");
        st->lds_ZL = 3 * nnK <= lim;
        st->sm_Z = (st->lds_ZL ? 3 : 1) * nnK * 8;
        const size_t step_rest = (size_t)K * maxn + maxn * maxn + 3 * maxn + 2 * MW_NT + MW_POTRF_SCR(K, maxn) + 8;
        st->step_w_lds = 2 * nnK + step_rest <= lim;
        const size_t stepd = (st->step_w_lds ? 2 : 1) * nnK + step_rest;
        if (stepd > lim) return mw_fail(CLRS_ERR_INVALID, "device-resident multi-word iteration needs PSD blocks that fit in LDS");
        st->sm_step = stepd * 8;
        // blocks whose inverse factor exists (k_mw_potrf_x): products instead of substitutions in Z and in the step length
        size_t &maxn_inv = st->maxn_inv;
        maxn_inv = 0;
        for (auto &k : c->blk) {
            if (k.inv) { st->any_xinv = true; maxn_inv = std::max(maxn_inv, (size_t)k.n); }
            else st->any_xsub = true;
        }
        {   // column panels per block of k_mwi_Zi (clrs_mw_zi_panels.h: the narrow form of 256 threads where the launch keeps a compute unit per workgroup) and
            // of the congruences of k_mwi_step: narrow enough that a product is ONE pass of the workgroup (64 entries: eight / four lanes each) while the
            // launch stays near one workgroup per compute unit: every workgroup reads the whole matrices its columns are multiplied with, and with 19
            // blocks of sides up to 54 or 64 blocks of 32 x 32 one-column panels were slower
            const MwZiPanels zp = mw_zi_panels((int)maxn_inv, q.NB, K, c->zi_narrow && maxn_inv <= 24);      // (beyond 24 rows: the tiled path, k_mwi_Zi is not launched)
            st->zs = zp.zs; st->zt = zp.threads; st->sm_Zi = zp.sm;
            const int old_rule = std::max<int>(MWI_ZS, (int)((maxn_inv + 7) / 8));     // panels of at most eight columns
            {   // (the step kernel's panels: four lanes per entry, 64 entries per pass, 256 threads: one wave per SIMD already)
                const int pcs = std::max<int>(1, 64 / (int)std::max<size_t>(maxn_inv, 1)), wants = ((int)maxn_inv + pcs - 1) / pcs;
                st->zs_step = std::max<int>(old_rule, std::min<int>(wants, 320 / std::max(q.NB, 1)));
            }
        }
        st->z_tiled = maxn_inv > 24;
        p.Xv = nullptr;                                     // X^-1 = Xi^T Xi for the k_mwi_Zi launches (formed by k_mwi_Xv: mw_ipm_enqueue_body); the tiled path and k_mwi_Z do without
        if (st->any_xinv && !st->z_tiled && c->xinv_product && (rc = mw_dmalloc(c, &p.Xv, q.xylen * K))) return rc;
        st->sm_bmm = (size_t)2 * K * MWI_BT * maxn_inv * 8;
        const size_t step_inv_need = 3 * maxn_inv * maxn_inv * K + step_rest;
        bool all_lds_inv = st->any_xinv;
        for (auto &k : c->blk) all_lds_inv = all_lds_inv && k.inv == 1;
        st->step_inv = all_lds_inv && step_inv_need <= lim;      // the step length factors Y itself, everything in LDS
        const size_t step_need2 = nnK + maxn * maxn + 3 * maxn + 2 * MW_NT + 8;
        st->y_with_x = st->any_xinv && !st->any_xsub && step_need2 <= lim;      // every block has its inverse factor: chol(Y)^-1 rides on the chol(X) launch
        if (!st->y_with_x && !st->step_inv) c->d.no_xfb = 0;      // the step length of X would substitute with Xf
        if (st->step_inv) st->sm_step = std::max(st->sm_step, step_inv_need * 8);
        if (st->y_with_x) st->sm_step = std::max(st->sm_step, step_need2 * 8);
        MW_DISPATCH(c, {
            if ((rc = mw_set_lds(k_mwi_Zi<KK>, st->sm_Zi))) return rc;
            if ((rc = mw_set_lds((k_mwi_rows_fwd<KK, DD>), c->sm_fwd))) return rc;
            if ((rc = mw_set_lds(k_mwi_bmm<KK>, st->sm_bmm))) return rc;
            if ((rc = mw_set_lds(k_mwi_Z<KK>, st->sm_Z))) return rc;
            if ((rc = mw_set_lds((k_mwi_step<KK, DD>), st->sm_step))) return rc;
        });
        {   // The corrector's right-hand side is affine in mu_c: Z = sym(X^-1 (P Y - R' - mu_c I)) = Z0 - mu_c X^-1, so rhs_x = rhs0 + mu_c tau with
            // tau_g = <A_g, X^-1> -- sums of the pairings w^T X^-1 v the assembly has formed anyway.  Z0, its traces and the forward half of the solve then
            // do not wait for the scalar stage that turns the predictor's dot products into beta_c and mu_c (13 us on one thread): that stage runs on the
            // side stream meanwhile, and the solve's backward launch picks mu_c up inside the kernel (MwDev::aff_*).  Where: small unsharded systems with
            // every inverse factor of the X blocks explicit, 1 x 1 dense blocks only, the refined solve in one workgroup per cluster with dy formed by
            // the backward launch itself.
            int mostb = 1;
            for (int j = 0; j < q.J; j++) mostb = std::max(mostb, c->clu[j].b1 - c->clu[j].b0);
            st->aff_ok = N > 0 && !c->wide_solve && (c->lds_q || c->pipe_Q) && mostb < 16 && q.J <= 4 && !q.dn_big && st->any_xinv && !st->any_xsub && !st->z_tiled &&
                         !q.mws_on && !q.mwx_on && c->refine != 0 && g_cfg_mw_affine_corrector != 0;
            if (st->aff_ok) {
                if ((rc = mw_dmalloc(c, &st->AX, q.T * K)) || (rc = mw_dmalloc(c, &p.tau, q.xlen * K)) || (rc = mw_dmalloc(c, &p.ttau, q.xlen * K)) ||
                    (rc = mw_dmalloc(c, &p.utau, (i64)q.J * N * K))) return rc;
            }
        }
        // default parameters (src/solver.jl:103-126)
        p.beta_infeasible = 0.3; p.beta_feasible = 0.1; p.gamma = 0.9; p.dual_thr = 1e-30; p.primal_thr = 1e-30;
        p.max_gap = 1e100; p.step_thr = 1e-7; p.safe_step = 1; p.corrector_only = 0;
        p.gap_thr = 0.0; p.stop_on = 0; p.need_dual = 0; p.need_primal = 0;
        st->ready = true;
    }
    // (re)load the objective data: a context may be reused for another right-hand side / objective
    MWCHECK(hipMemset((void *)p.C, 0, sizeof(double) * q.xylen * c->DK));
    MWCHECK(hipMemset((void *)p.c, 0, sizeof(double) * q.xlen * c->DK));
    if (N) MWCHECK(hipMemset((void *)p.b, 0, sizeof(double) * N * c->DK));
    MWCHECK(hipMemcpy((void *)p.C, data->C, sizeof(double) * q.xylen * data_limbs, hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy((void *)p.c, data->c, sizeof(double) * q.xlen * data_limbs, hipMemcpyHostToDevice));
    if (N) MWCHECK(hipMemcpy((void *)p.b, data->b, sizeof(double) * N * data_limbs, hipMemcpyHostToDevice));
    p.sgn = data->maximize ? 1.0 : -1.0;
    p.constant = data->constant;
    return 0;
}

extern "C" int clrs_mw_ipm_set_params(clrs_mw_ctx *c, const clrs_ipm_params *prm) {
    if (!c || !prm || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MwIpmDev &p = c->ipm->d;
    p.beta_infeasible = prm->beta_infeasible; p.beta_feasible = prm->beta_feasible; p.gamma = prm->gamma;
    p.dual_thr = prm->dual_error_threshold; p.primal_thr = prm->primal_error_threshold; p.max_gap = prm->max_complementary_gap;
    p.step_thr = prm->step_length_threshold; p.safe_step = prm->safe_step; p.corrector_only = prm->corrector_only != 0;
    return 0;
}

// cluster sharding: this rank's record of scalar stage `stage` into its gather slot, all-gather on the channel of the stream (the
// context's stream: stages 2, 3; the side stream: 0, 1, 4).  No-op for an unsharded context.
static int mw_ipm_exchange(clrs_mw_ctx *c, hipStream_t stream, int stage) {
    const MwDev &q = c->d;
    if (q.world <= 1) return 0;
    MwIpm *st = c->ipm;
    const MwIpmDev &p = st->d;
    if (!st->global_set || st->gs_world != q.world) return mw_fail(CLRS_ERR_STATE, "sharded interior-point iteration: clrs_mw_ipm_set_global first");
    const bool onM = stage == 2 || stage == 3;
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_gpack<KK, DD>), dim3(1), dim3(64), 0, stream, q, p, stage));
    MWCHECK(hipGetLastError());
    // during init / set the objectives run on the context's stream: its channel then carries the side buffer
    return mw_allgather(c, stream == c->stream ? 0 : 1, onM ? p.gsM : p.gsS, (size_t)p.GL, stream);
}
// with_xy: the same launch and the same record also carry <X,Y> of the iterate (scalar stage 0 of the NEXT iteration reads it: both look at the iterate
// the last update produced) -- one launch and, sharded, one exchange less per iteration.  Sharded, the record of such a tail (stage 15) carries in addition
// what the NEXT iteration's residuals need of the iterate alone -- this rank's rows of -B^T x and its max|P| (P = sum x_i A_i - X -+ C, formed here) --: the
// side stream then issues ONE exchange per iteration (stages 4 + 0 + 1 of the first version).
static int mw_ipm_wA(clrs_mw_ctx *c, hipStream_t stream, int mode);
static int mw_ipm_objectives(clrs_mw_ctx *c, hipStream_t stream, bool with_xy = false) {
    const MwDev &q = c->d;
    const MwIpmDev &p = c->ipm->d;
    int rc;
    if (with_xy && q.world > 1) {
        if ((rc = mw_ipm_wA(c, stream, 0))) return rc;
        MW_DISPATCH(c, {
            if (q.N) hipLaunchKernelGGL((k_mwi_pv<KK, DD>), dim3((q.N + MW_NT / 8 - 1) / (MW_NT / 8)), dim3(MW_NT), 0, stream, q, p, c->ipm->iter);
        });
    }
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_dots<KK, DD>), dim3(q.NB), dim3(MW_NT), (size_t)KK * 8 * 8, stream, q, p, with_xy ? 5 : 4, 0));
    if ((rc = mw_ipm_exchange(c, stream, with_xy ? 15 : 4))) return rc;
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(64), 0, stream, q, p, 4, c->ipm->iter));
    MWCHECK(hipGetLastError());
    return 0;
}
// Mixed-precision refinement inside the iteration (clrs_mw_kernels.hip.h::mw_kf_of): a solve starts with the context's reduced limb count for the factor
// stage and the products of the solve stage (unsharded contexts), and leaves it for good when the corrector's first pass is no longer good to one limb
// plus MW_KF_MARGIN bits -- below that, one refinement step does not give back the limb the factors lack.  The host reads the record of iteration k
// after iteration k + 1 is enqueued, so the change takes effect two iterations after the measurement; the first-pass accuracy of cohnelkies(8,15)
// falls by ~2 bits per iteration (2^-123 at iteration 1, 2^-99 at 28, 2^-45 at 55: prototype at 209 / 262 bits), hence the margin.
#define MW_KF_MARGIN 14
static void mw_ipm_reset_kf(clrs_mw_ctx *c) {
    c->ipm->kf_now = (c->kf_low < c->K && (!c->d.gathered || g_cfg_mw_sharded_factor_limbs != 0)) ? c->kf_low : c->K;      // (sharded: the accuracy that decides travels with the step lengths)
    c->ipm->held_refine_bits = 0;
    (void)hipMemsetAsync(c->d.refstat, 0, 4 * sizeof(unsigned long long), c->stream);
}
static void mw_ipm_note_bits(clrs_mw_ctx *c, int refine_bits) {
    MwIpm *st = c->ipm;
    if (st->kf_now < c->K && refine_bits > 0 && refine_bits < 53 * (c->K - st->kf_now) + MW_KF_MARGIN) st->kf_now = c->K;
}
// the status words of the decomposition are re-armed by the iteration itself (scalar stage 1); armed here once
static int mw_ipm_arm(clrs_mw_ctx *c) {
    MWCHECK(hipMemsetAsync(c->d.info, 0x7f, 2 * sizeof(int), c->stream));      // MW_INFO_NONE is the byte 0x7f four times
    MWCHECK(hipMemsetAsync(c->ipm->d.flags, 0, 4 * sizeof(double), c->stream));
    return 0;
}

extern "C" int clrs_mw_ipm_init(clrs_mw_ctx *c, double omega_p, double omega_d) {
    if (!c || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    const MwIpmDev &p = st->d;
    const int K = c->K;
    MWCHECK(hipMemsetAsync(p.x, 0, sizeof(double) * q.xlen * K, c->stream));
    if (q.N) MWCHECK(hipMemsetAsync(p.y, 0, sizeof(double) * q.N * K, c->stream));
    int rc;
    if ((rc = mw_ipm_arm(c))) return rc;
    MWCHECK(hipMemsetAsync(p.sc, 0, sizeof(double) * MSC_COUNT * K, c->stream));
    MW_DISPATCH(c, hipLaunchKernelGGL(k_mwi_init<KK>, dim3(q.NB), dim3(MW_NT), 0, c->stream, q, p, omega_p, omega_d));
    MWCHECK(hipGetLastError());
    st->iter = 0;
    st->forked = false; st->tail_pending = false;
    mw_ipm_reset_kf(c);
    if ((rc = mw_ipm_objectives(c, c->stream))) return rc;
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

static int mw_ipm_rows(clrs_mw_ctx *c, hipStream_t stream, int mode);
static int mw_ipm_wA(clrs_mw_ctx *c, hipStream_t stream, int mode);
static int mw_ipm_drain(clrs_mw_ctx *c);
// warm start (dualsol / primalsol keywords, src/solver.jl:202-239): planar limbs; any pointer may be NULL (kept).  The reference computes the residuals
// of the starting iterate before its loop (:322-333) and the first iteration chooses mu_p and beta_c by that feasibility (:373, :429-434): the same
// residuals are formed here (P, d through the pairings of one assembly, p) and leave their verdict in the feasibility flag the first iteration reads.
extern "C" int clrs_mw_ipm_set(clrs_mw_ctx *c, const double *x, const double *y, const double *X, const double *Y) {
    if (!c || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    const MwIpmDev &p = st->d;
    const int K = c->K;
    { int rc_ = mw_ipm_drain(c); if (rc_) return rc_; }
    if (x) MWCHECK(hipMemcpy(p.x, x, sizeof(double) * q.xlen * K, hipMemcpyHostToDevice));
    if (y && q.N) MWCHECK(hipMemcpy(p.y, y, sizeof(double) * q.N * K, hipMemcpyHostToDevice));
    if (X) MWCHECK(hipMemcpy(p.X, X, sizeof(double) * q.xylen * K, hipMemcpyHostToDevice));
    if (Y) MWCHECK(hipMemcpy(p.Y, Y, sizeof(double) * q.xylen * K, hipMemcpyHostToDevice));
    int rc;
    if ((rc = mw_ipm_arm(c))) return rc;
    MWCHECK(hipMemsetAsync(p.fmax, 0, 3 * sizeof(unsigned long long), c->stream));
    hipStream_t M = c->stream;
    if ((rc = mw_cholesky_blocks_dev2(c, p.X, p.Xc, nullptr, nullptr, nullptr))) return rc;      // (a failure here leaves the flag at "infeasible"; the first iteration reports it)
    if ((rc = clrs_mw_schur_assemble_dev(c, p.Xc, p.Y))) return rc;                              // A_Y: the pairings w^T Y v that d = c - <A, Y> - B y is read from
    if ((rc = mw_ipm_wA(c, M, 0))) return rc;                                                    // P = sum x_i A_i - X -+ C, max|P|
    MW_DISPATCH(c, {
        if (q.dn_big) hipLaunchKernelGGL((k_mwi_rows_dn<KK, DD>), dim3((unsigned)((q.xlen + MW_NT / 64 - 1) / (MW_NT / 64))), dim3(MW_NT), 0, M, q, p, 0);
    });
    if ((rc = mw_ipm_rows(c, M, 0))) return rc;                                                  // d, max|d|
    MW_DISPATCH(c, {
        if (q.N) hipLaunchKernelGGL((k_mwi_pv<KK, DD>), dim3((q.N + MW_NT / 8 - 1) / (MW_NT / 8)), dim3(MW_NT), 0, M, q, p, 0);      // p = +-b - B^T x, max|p|
    });
    if ((rc = mw_ipm_exchange(c, M, 1))) return rc;
    MW_DISPATCH(c, {
        if (q.world > 1) hipLaunchKernelGGL((k_mwi_pvfin<KK, DD>), dim3(1), dim3(MW_NT), 0, M, q, p);
        hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(1), 0, M, q, p, 5, 0);
    });
    MWCHECK(hipGetLastError());
    c->assembled = false;
    st->iter = 0;
    st->forked = false; st->tail_pending = false; st->frozen = false;
    mw_ipm_reset_kf(c);
    if ((rc = mw_ipm_objectives(c, c->stream))) return rc;
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- one iteration over two streams ----------------------------------------------------------------------------------------------
// M = the context's stream, S = side.  What stands on one line runs in stream order; arrows are events.
//   M: chol X (+ chol Y^-1), assembly  -E_ASM->  chol S_j, L^-1 B, Q | (E_PREP) chol Q with the solve's first products on its launch, rest of the
//      solve, dX, dY | <X+dX, Y+dY> with R' on its launch, errors, beta_c, mu_c | Z, Z V, rhs_x + first products of the solve, rest of the solve,
//      dX, dY | both step lengths | update  -E_UPD->
//   S: (E_UPD of the previous iteration) its objectives, its record -> host -E_REC-> host | <X,Y>, mu, mu_p | P = sum x_i A_i - X -+ C |
//      R' = -XY | (E_ASM) Z = sym(X^-1(PY - R)), Z V | d, p | rhs_x   -E_PREP-> M
// Everything the predictor's right-hand side needs depends on the iterate and on the assembly's pairings only, so S forms it beside the
// factorisations (two kernels of 94 and 81 us on 8 workgroups each).  Every event recorded or awaited on M costs it a bubble of 6-7 us
// (measured: profiles/r03), which is why M records twice and waits once per iteration and short kernels (R', the step length of X)
// stay in line although they are independent of their neighbours.
static int mw_ipm_rhs(clrs_mw_ctx *c, hipStream_t stream, int which) {      // Z = sym(X^-1(PY - R)) (which 0) or dY (which 1) into the dY buffer
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    st->d.stamps = c->mws.stamps;
    const MwIpmDev &p = st->d;
    MW_DISPATCH(c, {
        if (st->any_xinv && st->z_tiled) {                // large blocks: each product a launch over 8 x 8 tiles
            const int nt = ((int)st->maxn_inv + MWI_BT - 1) / MWI_BT;
            for (int op = 0; op < 4; op++) hipLaunchKernelGGL(k_mwi_bmm<KK>, dim3(nt * nt, q.NB), dim3(MW_NT), st->sm_bmm, stream, q, p, op, which);
        } else if (st->any_xinv) hipLaunchKernelGGL(k_mwi_Zi<KK>, dim3(q.NB, st->zs), dim3(st->zt), st->sm_Zi, stream, q, p, which);
        if (st->any_xsub) hipLaunchKernelGGL(k_mwi_Z<KK>, dim3(q.NB), dim3(MW_NT), st->sm_Z, stream, q, p, which, st->lds_ZL ? 1 : 0);
    });
    MWCHECK(hipGetLastError());
    return 0;
}
static int mw_ipm_trace_rhs(clrs_mw_ctx *c, hipStream_t stream) {             // T = Z V, then rhs_x = -d - <A_*, Z>  (:1518-1523)
    const MwDev &q = c->d;
    const MwIpmDev &p = c->ipm->d;
    MW_DISPATCH(c, {
        if (q.nlr) hipLaunchKernelGGL((k_mwi_MV<KK, DD>), dim3((c->maxn * c->maxU * MWI_EW + MW_NT - 1) / MW_NT, q.nlr), dim3(MW_NT), 0, stream, q, (const double *)p.dY);
        if (q.dn_big) hipLaunchKernelGGL((k_mwi_rows_dn<KK, DD>), dim3((unsigned)((q.xlen + MW_NT / 64 - 1) / (MW_NT / 64))), dim3(MW_NT), 0, stream, q, p, 1);
    });
    MWCHECK(hipGetLastError());
    return 0;
}
static int mw_ipm_rows(clrs_mw_ctx *c, hipStream_t stream, int mode) {
    const MwDev &q = c->d;
    const MwIpmDev &p = c->ipm->d;
    int mostb = 1;
    for (int j = 0; j < q.J; j++) mostb = std::max(mostb, c->clu[j].b1 - c->clu[j].b0);
    const int groups = mostb >= 16 ? 8 : 1;             // lane groups per row, one PSD block of the row's cluster each at a time
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_rows<KK, DD>), dim3((unsigned)((q.xlen * MWI_RW * groups + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, stream, q, p, mode, groups));
    MWCHECK(hipGetLastError());
    return 0;
}
static int mw_ipm_wA(clrs_mw_ctx *c, hipStream_t stream, int mode) {          // sum_i a_i A_i (+ the rest of P or dX), coefficients in LDS when they fit
    const MwDev &q = c->d;
    const MwIpmDev &p = c->ipm->d;
    const int maxnn = c->maxn * c->maxn;
    const size_t sm = (size_t)c->maxTb * c->K * 8;
    const bool in_lds = sm <= 48 * 1024;
    MW_DISPATCH(c, {
        if (q.T && !in_lds) hipLaunchKernelGGL((k_mwi_coef<KK, DD>), dim3((unsigned)((q.T + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, stream, q, p, (const double *)(mode == 0 ? p.x : p.dx));
        const int ew = c->maxTb >= 24 ? 16 : MWI_EW;      // lanes per entry
        if (p.wBn) hipLaunchKernelGGL((k_mwi_wB<KK, DD>), dim3((unsigned)((q.T * (i64)p.wBn + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, stream, q, p, mode);
        hipLaunchKernelGGL((k_mwi_wA<KK, DD>), dim3((maxnn * ew + MW_NT - 1) / MW_NT, q.NB), dim3(MW_NT), in_lds && !p.wBn ? sm : 0, stream, q, p, mode, in_lds && !p.wBn ? 1 : 0, p.wBn ? 17 : ew);
    });
    MWCHECK(hipGetLastError());
    return 0;
}
// predictor: its direction only feeds beta_c (a ratio of two traces, :429-434) and the second-order term dX dY of the corrector's right-hand side -- nothing
// that moves the iterate or enters the residuals -- so its solve stays one pass of products unless clrs_mw_options.refine_predictor asks otherwise; the
// corrector's solve, whose (dx, dy) become the step, always takes the refinement step
static int mw_ipm_solve_dX(clrs_mw_ctx *c, bool predictor = false) {           // on M: (dx, dy) from (rhs_x, p), then dX = P + sum dx_i A_i
    const MwIpmDev &p = c->ipm->d;
    int rc;
    c->refine_skip_next = predictor && !c->refine_predictor;
    if ((rc = clrs_mw_schur_solve_dev(c, p.rhsx, p.pv, p.dx, p.dy))) return rc;
    return mw_ipm_wA(c, c->stream, 1);
}

// enqueue iteration st->iter + 1 (no synchronisation); its record lands in h_rec[(iter & 1) * MREC_COUNT] behind event E_REC0 + (iter & 1)
// of the NEXT enqueue's side-stream head, or of mw_ipm_finish
// word_value > 0: called from the enqueue of the NEXT iteration, whose first launch on M (the Cholesky of the X blocks, submitted just before) stores that
// value to sync[2] as it starts, i.e. when the update is complete: S waits for the word in a kernel of its own.  0 (mw_ipm_finish: nothing follows on M): the event.
static int mw_ipm_tail(clrs_mw_ctx *c, int word_value = 0, bool with_next = false) {      // S: objectives of the iterate the last update produced, record of that iteration (with_next: an iteration follows)
    MwIpm *st = c->ipm;
    if (!st->tail_pending) return 0;
    const int par = st->iter & 1;
    int rc;
    if (word_value > 0) hipLaunchKernelGGL(k_mwi_wait<0>, dim3(1), dim3(64), 0, st->side, (const int *)(st->d.sync + 2), word_value, c->d.info, c->d.J + 1);
    else {
        if (!st->upd_recorded) MWCHECK(hipEventRecord(st->ev[MwIpm::E_UPD], c->stream));      // (word mode, called from mw_ipm_finish: M stands right behind the update)
        MWCHECK(hipStreamWaitEvent(st->side, st->ev[MwIpm::E_UPD], 0));
    }
    if ((rc = mw_ipm_objectives(c, st->side, word_value != 0 || with_next))) return rc;
    st->xy_with_tail = word_value != 0 || with_next;
    MWCHECK(hipMemcpyAsync(st->h_rec + (size_t)par * MREC_COUNT, st->d.rec, sizeof(double) * MREC_COUNT, hipMemcpyDeviceToHost, st->side));
    MWCHECK(hipEventRecord(st->ev[MwIpm::E_REC0 + par], st->side));
    st->tail_pending = false;
    return 0;
}
// both step lengths in one launch (after the Cholesky launch of this iteration: the inverse factors of X, and of Y where they ride along); with every
// inverse factor in memory the congruences are split over column panels (zs workgroups each).  Enqueue only; the caller checks hipGetLastError.
static int mw_ipm_launch_step(clrs_mw_ctx *c, hipStream_t M) {
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    const MwIpmDev &p = st->d;
    const int ip = st->y_with_x ? 2 : st->step_inv ? 1 : 0, wl = st->step_w_lds ? 1 : 0;
    if (ip == 2 && st->z_tiled) {                         // large blocks: the two products of each congruence as tiled launches, then the eigenvalues
        const int nt = ((int)st->maxn_inv + MWI_BT - 1) / MWI_BT;
        MW_DISPATCH(c, {
            hipLaunchKernelGGL(k_mwi_bmm<KK>, dim3(nt * nt, q.NB, 2), dim3(MW_NT), st->sm_bmm, M, q, p, 4, 0);
            hipLaunchKernelGGL(k_mwi_bmm<KK>, dim3(nt * nt, q.NB, 2), dim3(MW_NT), st->sm_bmm, M, q, p, 5, 0);
            hipLaunchKernelGGL((k_mwi_step<KK, DD>), dim3(q.NB, 2, 1), dim3(MW_NT), st->sm_step, M, q, p, wl, 3, st->iter, 0);
        });
    } else
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_step<KK, DD>), dim3(q.NB, 2, ip == 2 ? st->zs_step : 1), dim3(MW_NT), st->sm_step, M, q, p, wl, ip, st->iter, 0));
    return 0;
}
static int mw_ipm_enqueue_body(clrs_mw_ctx *c) {
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    const int maxnn = c->maxn * c->maxn;
    const size_t sm_red = (size_t)c->K * 8 * 8;
    hipStream_t M = c->stream, S = st->side;
    int rc;
    // Between the two streams of one rank: words instead of events where a launch exists that can store or await them (DESIGN.md section 5.5).
    // RULE: a launch that waits for a word inside the kernel is submitted AFTER the launch that stores it.  Streams may share a hardware queue (HIP promises
    // nothing else); a queue runs its packets in submission order, so a producer submitted first has run when its waiter starts on the same queue, and on
    // different queues the waiter spins until the producer runs -- a cycle of waits would need some waiter submitted before its producer.  (Measured the hard
    // way: with the tail's wait submitted BEFORE the Cholesky launch that stores its word, a process with enough streams to make the two share a queue sat in
    // the bounded polls, 4 s each.)
    const bool words = !q.gathered && c->stream_words;      // (off: clrs_config_set("mw_stream_words", 0) or CLRS_MW_STREAM_WORDS=0 -- counter-collection runs serialise kernels)
    c->d.kf = st->kf_now;                                   // limbs of this iteration's factor stage and solve products (mw_ipm_reset_kf)
    const int seq = ++st->sync_seq;
    const MwIpmDev &p = st->d;
    // M: the Cholesky of the X blocks of the NEW iterate first -- its launch stores "the update of the previous iteration is complete" as it starts
    c->ipm_arms_info = true;
    c->d.mark_word = words ? p.sync + 2 : nullptr;
    c->d.mark_value = seq;
    // ... and carries the Y half of the assembly's pairings as riders (T = Y V, GY = V^T T need the iterate only); k_mw_zt / k_mw_gram then skip it
    const bool y_rides = mw_y_riders_ok(c);
    c->ride_y = y_rides ? p.Y : nullptr;
    rc = mw_cholesky_blocks_dev2(c, p.X, p.Xc, st->y_with_x ? p.Y : nullptr, p.Yi, p.yfail);
    c->ride_y = nullptr;
    c->d.mark_word = nullptr;
    if (rc) return rc;
    // S: the previous iteration's objectives and record lead this iteration's side work (they wait for that word, or for the event)
    st->xy_with_tail = false;
    if ((rc = mw_ipm_tail(c, words ? seq : 0, true))) return rc;
    if (!st->forked) {                                   // first iteration after init / set: S starts behind whatever M has been doing
        MWCHECK(hipEventRecord(st->ev[MwIpm::E_UPD], M));
        MWCHECK(hipStreamWaitEvent(S, st->ev[MwIpm::E_UPD], 0));
        st->forked = true;
    }
    st->iter++;
    st->d.rec = st->d_rec + (size_t)(st->iter & 1) * MREC_COUNT;
    // M: the rest of the decomposition -- the longest chain of the iteration
    const bool aff = st->aff_ok && !q.gathered;            // (the corrector's right-hand side affine in mu_c: clrs_mw_ipm_create_ex)
    c->d.AX = aff ? st->AX : nullptr;
    c->d.skip_y = y_rides ? 1 : 0;
    rc = clrs_mw_schur_assemble_dev(c, p.Xc, p.Y);
    c->d.skip_y = 0;
    if (rc) return rc;
    if (!words) MWCHECK(hipEventRecord(st->ev[MwIpm::E_ASM], M));
    c->d.mark_word = words ? p.sync + 1 : nullptr;        // "the assembly is complete" (stored by the first launch of the factorisation): S waits for it below
    // the factorisation in its two halves, so that the Cholesky of Q is enqueued behind the side stream's work (below) and can carry
    // the first products of the predictor's solve, whose right-hand side the side stream forms
    const bool split_factor = q.N > 0;
    rc = split_factor ? clrs_mw_schur_factor_local_dev(c) : clrs_mw_schur_factor_dev(c);
    c->d.mark_word = nullptr;
    if (rc) return rc;
    if (split_factor && q.gathered && (rc = mw_allgather(c, 0, q.Qg, (size_t)q.N * q.N * c->K, M))) return rc;      // sharded: the partial Q of every rank (as clrs_mw_schur_factor_dev)
    c->ipm_arms_info = false;
    // S: everything that needs the iterate only
    if (!st->xy_with_tail) {                             // (<X,Y> came with the tail's launch and record otherwise)
        MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_dots<KK, DD>), dim3(q.NB), dim3(MW_NT), sm_red, S, q, p, 1, 0));
        if ((rc = mw_ipm_exchange(c, S, 0))) return rc;
    }
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(1), 0, S, q, p, st->xy_with_tail ? 10 : 0, st->iter));
    MWCHECK(hipGetLastError());
    // sharded, behind a tail: P, this rank's -B^T x and max|P| came with the tail's record (stage 15); p and the maxima are completed here, the exchange of
    // stage 1 does not take place
    const bool res_with_tail = st->xy_with_tail && q.world > 1;
    if (res_with_tail) {
        MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_pvfin<KK, DD>), dim3(1), dim3(MW_NT), 0, S, q, p));
        MWCHECK(hipGetLastError());
    } else if ((rc = mw_ipm_wA(c, S, 0))) return rc;
    MW_DISPATCH(c, hipLaunchKernelGGL(k_mwi_R<KK>, dim3((maxnn * MWI_EW + MW_NT - 1) / MW_NT, q.NB), dim3(MW_NT), 0, S, q, p, 0));
    MWCHECK(hipGetLastError());
    if (words) hipLaunchKernelGGL(k_mwi_wait<0>, dim3(1), dim3(64), 0, S, (const int *)(p.sync + 1), seq, q.info, q.J + 1);      // the inverse factors of chol(X), and A_Y: the pairings w^T Y v of the assembly
    else MWCHECK(hipStreamWaitEvent(S, st->ev[MwIpm::E_ASM], 0));
    if (p.Xv) {
        // Xv = Xi^T Xi, once for the four k_mwi_Zi launches of this iteration.  Written here only: behind the Cholesky of X of THIS iteration (the wait above) and so
        // behind the previous iteration's update, i.e. behind every launch of M that read the previous Xv; M reads it first behind the Cholesky of Q, whose
        // riders have waited for this stream's mark (E_PREP in event mode), which is submitted behind this launch.
        const int xv_tiles = ((int)(st->maxn_inv * st->maxn_inv) * MWI_ZL + MW_NT - 1) / MW_NT;
        MW_DISPATCH(c, hipLaunchKernelGGL(k_mwi_Xv<KK>, dim3(xv_tiles, q.NB), dim3(MW_NT), 0, S, q, p));
        MWCHECK(hipGetLastError());
    }
    if ((rc = mw_ipm_rhs(c, S, 0))) return rc;
    if ((rc = mw_ipm_trace_rhs(c, S))) return rc;
    MW_DISPATCH(c, {
        if (q.dn_big) hipLaunchKernelGGL((k_mwi_rows_dn<KK, DD>), dim3((unsigned)((q.xlen + MW_NT / 64 - 1) / (MW_NT / 64))), dim3(MW_NT), 0, S, q, p, 0);
    });
    {   // d (and, with an affine corrector, tau beside it)
        double *const keep_tau = st->d.tau;
        if (!aff) st->d.tau = nullptr;
        rc = mw_ipm_rows(c, S, 0);
        st->d.tau = keep_tau;
        if (rc) return rc;
    }
    if (!res_with_tail) {
        MW_DISPATCH(c, {
            if (q.N) hipLaunchKernelGGL((k_mwi_pv<KK, DD>), dim3((q.N + MW_NT / 8 - 1) / (MW_NT / 8)), dim3(MW_NT), 0, S, q, p, st->iter);
        });
        if ((rc = mw_ipm_exchange(c, S, 1))) return rc;              // -B^T x, max|P|, max|d| of every rank (first iteration of a solve: no tail in front of it)
    }
    MW_DISPATCH(c, {
        if (q.world > 1 && !res_with_tail) hipLaunchKernelGGL((k_mwi_pvfin<KK, DD>), dim3(1), dim3(MW_NT), 0, S, q, p);
        if (q.dn_big) hipLaunchKernelGGL((k_mwi_rows_dn<KK, DD>), dim3((unsigned)((q.xlen + MW_NT / 64 - 1) / (MW_NT / 64))), dim3(MW_NT), 0, S, q, p, 1);
    });
    MWCHECK(hipGetLastError());
    if ((rc = mw_ipm_rows(c, S, 1))) return rc;
    // M: predictor.  What it reads from S (rhs_x first, by the workgroups that ride on the Cholesky of Q) is ready when S has passed this point: when those
    // workgroups exist (small unsharded systems whose Q is factored in one launch) they wait for a word S writes, inside their launch -- the launch itself,
    // and so the 31 pivots of Q, start without the main stream having waited for an event (a bubble of 6-15 us, measured); every later kernel of M is
    // behind that launch.  Otherwise: the event.
    const bool word_sync = words && split_factor && !c->wide_solve && (c->lds_q || c->pipe_Q);
    if (word_sync) hipLaunchKernelGGL(k_mwi_mark<0>, dim3(1), dim3(1), 0, S, p.sync, seq);
    else {
        MWCHECK(hipEventRecord(st->ev[MwIpm::E_PREP], S));
        MWCHECK(hipStreamWaitEvent(M, st->ev[MwIpm::E_PREP], 0));
    }
    if (split_factor) {
        c->ride_wait = word_sync ? p.sync : nullptr;
        c->ride_wait_value = seq;
        c->ride_fwd = p.rhsx;
        c->ipm_arms_info = true;
        if (aff) { c->d.ride2_rhs = p.tau; c->d.ride2_t = p.ttau; c->d.ride2_u = p.utau; }      // t_tau, u_tau: the forward half on tau, beside the predictor's
        rc = clrs_mw_schur_factor_finish_dev(c);
        c->d.ride2_rhs = nullptr;
        c->ipm_arms_info = false;
        c->ride_fwd = nullptr;
        c->ride_wait = nullptr;
        if (rc) return rc;
    }
    // the predictor's dX, dY and the dot products that lead to beta_c in the limbs of the factors its (dx, dy) came from (MwIpmDev::klow): nothing of them moves
    // the iterate or enters a residual -- only beta_c and the second-order term dX dY of the corrector's right-hand side
    st->d.klow = c->refine_predictor ? c->K : c->d.kf;
    rc = mw_ipm_solve_dX(c, true);
    if (!rc) rc = mw_ipm_rhs(c, M, 1);
    if (rc) { st->d.klow = c->K; return rc; }
    // the corrector's R' rides on the launch of the dot products; sixteen lanes per entry while the launch stays small (it is the longer half)
    const bool r16 = (i64)maxnn * 16 * q.NB <= 65536;
    const int r_tiles = (maxnn * (r16 ? 16 : MWI_EW) + MW_NT - 1) / MW_NT;
    MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_dots<KK, DD>), dim3(q.NB + r_tiles * q.NB), dim3(MW_NT), sm_red, M, q, p, 2, r16 ? -r_tiles : r_tiles));
    st->d.klow = c->K;
    if ((rc = mw_ipm_exchange(c, M, 2))) return rc;
    const bool aff_async = aff && word_sync;      // ... with the scalar stage on the side stream (words); without words the same algebra in stream order (bit-identical)
    if (aff_async) {
        // M goes on with Z0 = sym(X^-1 (P Y - R')) at once; its first launch stores "the dot products are complete" as it starts.  S: errors (stage 1),
        // beta_c, mu_c, then "mu_c is there".  (Submission order: the waiting launches behind the storing ones -- the RULE above.)
        c->d.mark_word = p.sync + 3; c->d.mark_value = seq;
        rc = mw_ipm_rhs(c, M, 2);
        c->d.mark_word = nullptr;
        if (rc) return rc;
        hipLaunchKernelGGL(k_mwi_wait<0>, dim3(1), dim3(64), 0, S, (const int *)(p.sync + 3), seq, q.info, q.J + 1);
        MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(1), 0, S, q, p, 2, st->iter));
        hipLaunchKernelGGL(k_mwi_mark<0>, dim3(1), dim3(1), 0, S, p.sync + 4, seq);
        MWCHECK(hipGetLastError());
    } else {
        MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(1), 0, M, q, p, 2, st->iter));       // errors (stage 1), then beta_c, mu_c
        MWCHECK(hipGetLastError());
        // M: corrector
        if ((rc = mw_ipm_rhs(c, M, aff ? 2 : 0))) return rc;
    }
    if ((rc = mw_ipm_trace_rhs(c, M))) return rc;
    {   // small unsharded systems whose clusters have a few blocks: rhs_x and the first products of the solve in one launch
        int mostb = 1;
        for (int j = 0; j < q.J; j++) mostb = std::max(mostb, c->clu[j].b1 - c->clu[j].b0);
        if (!c->wide_solve && mostb < 16 && q.J <= 64) {
            MW_DISPATCH(c, hipLaunchKernelGGL((k_mwi_rows_fwd<KK, DD>), dim3(q.J), dim3(MW_NT), c->sm_fwd, M, q, p));
            MWCHECK(hipGetLastError());
            c->fwd_rode = true;
        } else if ((rc = mw_ipm_rows(c, M, 1))) return rc;
    }
    if (aff) {
        if (!c->fwd_rode) return mw_fail(CLRS_ERR_STATE, "affine corrector without the fused forward half");
        c->d.aff_mu = p.sc + MSC_MUS; c->d.aff_mu_plane = MSC_COUNT; c->d.aff_rhs = p.tau; c->d.aff_t = p.ttau; c->d.aff_u = p.utau;
        c->d.aff_wait = aff_async ? p.sync + 4 : nullptr; c->d.aff_wait_value = seq;
    }
    rc = mw_ipm_solve_dX(c);
    c->d.aff_mu = nullptr;
    if (rc) return rc;
    if ((rc = mw_ipm_rhs(c, M, 1))) return rc;
    if ((rc = mw_ipm_launch_step(c, M))) return rc;
    if ((rc = mw_ipm_exchange(c, M, 3))) return rc;
    MW_DISPATCH(c, {
        if (q.world > 1) hipLaunchKernelGGL((k_mwi_scalar<KK, DD>), dim3(1), dim3(1), 0, M, q, p, 3, st->iter);
        hipLaunchKernelGGL(k_mwi_update<KK>, dim3((unsigned)std::min<i64>(1024, (q.xylen + q.xlen + q.N + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, M, q, p);
    });
    MWCHECK(hipGetLastError());
    if (!words) MWCHECK(hipEventRecord(st->ev[MwIpm::E_UPD], M));
    st->upd_recorded = !words;
    st->tail_pending = true;
    return 0;
}
// (the body toggles context-wide switches -- who re-arms the status words, whose right-hand side rides on the Cholesky of Q -- and returns early on
// errors: whatever the exit, they are back in their resting state, so that later calls outside the iteration do not read stale state)
static int mw_ipm_enqueue(clrs_mw_ctx *c) {
    const int rc = mw_ipm_enqueue_body(c);
    c->d.kf = c->kf_entry;
    c->ipm->d.klow = c->K;
    c->d.AX = nullptr; c->d.aff_mu = nullptr; c->d.ride2_rhs = nullptr;
    c->ipm_arms_info = false;
    c->ride_fwd = nullptr;
    c->ride_wait = nullptr;
    c->ride_y = nullptr;
    c->d.skip_y = 0;
    c->d.mark_word = nullptr;
    if (rc) { c->fwd_rode = false; c->ipm->tail_pending = false; }
    return rc;
}
// the record of the last enqueued iteration without enqueuing another one
static int mw_ipm_finish(clrs_mw_ctx *c) { return mw_ipm_tail(c); }
static void mw_ipm_read_record(const double *r, clrs_ipm_record *out) {
    out->iter = (int)r[MREC_ITER]; out->pd_feas = (int)r[MREC_PDFEAS]; out->error_code = (int)r[MREC_ERR];
    out->factor_status = (int)r[MREC_FSTAT]; out->cholesky_status = (int)r[MREC_XSTAT]; out->refine_bits = (int)r[MREC_REFB];
    out->mu = r[MREC_MU]; out->d_obj = r[MREC_DOBJ]; out->p_obj = r[MREC_POBJ]; out->gap = r[MREC_GAP];
    out->dual_error = r[MREC_DERR]; out->primal_error = r[MREC_PERR]; out->alpha_d = r[MREC_AD]; out->alpha_p = r[MREC_AP];
    out->beta_c = r[MREC_BETA]; out->max_P = r[MREC_MAXP]; out->max_p = r[MREC_MAXp]; out->max_d = r[MREC_MAXd];
}
static int mw_ipm_drain(clrs_mw_ctx *c) {
    MWCHECK(hipStreamSynchronize(c->stream));
    MWCHECK(hipStreamSynchronize(c->ipm->side));
    return 0;
}

extern "C" int clrs_mw_ipm_iterate(clrs_mw_ctx *c, clrs_ipm_record *out) {
    if (!c || !out || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    MwIpm *st = c->ipm;
    st->d.stop_on = 0;                      // the caller decides about termination
    int rc;
    if (st->frozen) { MWCHECK(hipMemsetAsync(st->d.flags + 6, 0, sizeof(int), c->stream)); st->frozen = false; }
    const int held = st->held_refine_bits;          // (of the record before the last: see MwIpm::held_refine_bits)
    if ((rc = mw_ipm_enqueue(c))) return rc;
    mw_ipm_note_bits(c, held);
    if ((rc = mw_ipm_finish(c))) return rc;
    MWCHECK(hipEventSynchronize(st->ev[MwIpm::E_REC0 + (st->iter & 1)]));
    mw_ipm_read_record(st->h_rec + (size_t)(st->iter & 1) * MREC_COUNT, out);
    st->held_refine_bits = out->refine_bits;
    return 0;
}

// The whole loop of solvesdp (src/solver.jl:348-589) with its termination test (:921-950): iterations are enqueued ONE AHEAD of the
// record the host waits for, so that the device never idles between two iterations; the device evaluates the same test on the same
// numbers at the end of every iteration and, once it holds, freezes the iterate (k_mwi_update becomes a no-op), which makes the
// iteration the host has already enqueued behind the last one harmless.  records[i] = the table row of iteration i + 1.
// Returns 0; *n_iter = iterations run; *error_code = 0, or 1 / 3 / 4 from the device, or 2 (max_iterations reached).
static int mw_ipm_solve_body(clrs_mw_ctx *c, const clrs_ipm_stop *stop, clrs_ipm_record_fn on_record, void *user, clrs_ipm_record *records, int max_records, int *n_iter, int *error_code);
// on_record (may be NULL): called on the calling thread with the record of every iteration as the host reads it -- the table row of src/solver.jl:566-582 while
// the device is already one iteration further; it must not call into this context
extern "C" int clrs_mw_ipm_solve_cb(clrs_mw_ctx *c, const clrs_ipm_stop *stop, clrs_ipm_record_fn on_record, void *user, clrs_ipm_record *records, int max_records,
                                    int *n_iter, int *error_code) {
    if (!c || !stop || !n_iter || !error_code || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    const int rc = mw_ipm_solve_body(c, stop, on_record, user, records, max_records, n_iter, error_code);
    c->ipm->d.stop_on = 0;                       // on every exit: a later step-by-step iteration must not find the device-side test armed
    if (rc) c->ipm->frozen = true;               // ... and clears the freeze word before it runs (clrs_mw_ipm_iterate)
    return rc;
}
extern "C" int clrs_mw_ipm_solve(clrs_mw_ctx *c, const clrs_ipm_stop *stop, clrs_ipm_record *records, int max_records, int *n_iter, int *error_code) {
    return clrs_mw_ipm_solve_cb(c, stop, nullptr, nullptr, records, max_records, n_iter, error_code);
}
static int mw_ipm_solve_body(clrs_mw_ctx *c, const clrs_ipm_stop *stop, clrs_ipm_record_fn on_record, void *user, clrs_ipm_record *records, int max_records, int *n_iter,
                             int *error_code) {
    MwIpm *st = c->ipm;
    MwIpmDev &p = st->d;
    p.stop_on = 1; p.gap_thr = stop->duality_gap_threshold; p.need_dual = stop->need_dual_feasible; p.need_primal = stop->need_primal_feasible;
    MWCHECK(hipMemsetAsync(p.flags + 6, 0, sizeof(int), c->stream));
    st->frozen = false;
    *n_iter = 0; *error_code = 0;
    const int first = st->iter + 1, last = st->iter + stop->max_iterations;      // iteration numbers this call may run
    int rc, enq = st->iter;
    if (stop->max_iterations <= 0) { *error_code = 2; return 0; }
    mw_ipm_note_bits(c, st->held_refine_bits);      // (a record clrs_mw_ipm_iterate left behind)
    st->held_refine_bits = 0;
    if ((rc = mw_ipm_enqueue(c))) return rc;
    enq = st->iter;
    for (int k = first;; k++) {
        if (k < last) { if ((rc = mw_ipm_enqueue(c))) return rc; enq = st->iter; }      // one ahead (its side-stream head carries the record of k)
        else if ((rc = mw_ipm_finish(c))) return rc;
        MWCHECK(hipEventSynchronize(st->ev[MwIpm::E_REC0 + (k & 1)]));
        clrs_ipm_record r;
        mw_ipm_read_record(st->h_rec + (size_t)(k & 1) * MREC_COUNT, &r);
        mw_ipm_note_bits(c, r.refine_bits);
        if (records && *n_iter < max_records) records[*n_iter] = r;
        (*n_iter)++;
        if (on_record) on_record(&r, user);
        const bool df = r.dual_error < p.dual_thr, pf = r.primal_error < p.primal_thr;
        bool done = r.error_code != 0 || (p.need_dual && df) || (p.need_primal && pf) || (!p.corrector_only && df && pf && r.gap < p.gap_thr);
        if (r.error_code != 0) *error_code = r.error_code;
        if (!done && k == last) { *error_code = 2; done = true; }                  // src/solver.jl:362-366
        if (done) break;
    }
    st->frozen = true;
    st->tail_pending = false;                    // (the iteration enqueued ahead has no reader)
    if ((rc = mw_ipm_drain(c))) return rc;      // the iteration enqueued ahead of the last record found the iterate frozen
    st->iter = *n_iter + first - 1;
    (void)enq;
    p.stop_on = 0;
    return 0;
}

// Cluster-sharded iteration: what a rank cannot know from its own clusters.  rows_of_X_global = the K of mu = <X,Y> / K (src/solver.jl:369)
// over ALL clusters; clusters_global = J of the whole problem; cluster_ids / block_ids = the global number (0-based) of every local
// cluster / PSD block, so that failure codes name the same block on every rank (NULL: local numbers).  After clrs_mw_ipm_create and
// after the context has its rank (clrs_mw_comm_init / clrs_mw_comm_init_local / clrs_mw_set_shard), before clrs_mw_ipm_init.
extern "C" int clrs_mw_ipm_set_global(clrs_mw_ctx *c, int rows_of_X_global, int clusters_global, const int32_t *cluster_ids, const int32_t *block_ids) {
    if (!c || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    if (rows_of_X_global <= 0 || clusters_global < c->d.J) return mw_fail(CLRS_ERR_INVALID, "bad global sizes");
    MWCHECK(hipSetDevice(c->device));
    MwIpm *st = c->ipm;
    MwIpmDev &p = st->d;
    const MwDev &q = c->d;
    int rc;
    p.Ktot = rows_of_X_global;
    p.Jglob = clusters_global;
    p.GL = MWG_LEN(c->K, q.N);
    if (st->gs_world != q.world) {
        if ((rc = mw_dmalloc(c, &p.gsM, (i64)q.world * p.GL)) || (rc = mw_dmalloc(c, &p.gsS, (i64)q.world * p.GL))) return rc;
        st->gs_world = q.world;
    }
    p.clu_gid = p.blk_gid = nullptr;
    if (cluster_ids) { std::vector<int> v(cluster_ids, cluster_ids + q.J); if ((rc = mw_upload(c, v, &p.clu_gid))) return rc; }
    if (block_ids) { std::vector<int> v(block_ids, block_ids + q.NB); if ((rc = mw_upload(c, v, &p.blk_gid))) return rc; }
    st->global_set = true;
    return 0;
}

extern "C" int clrs_mw_ipm_get(clrs_mw_ctx *c, double *x, double *y, double *X, double *Y) {
    if (!c || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    { int rc_ = mw_ipm_drain(c); if (rc_) return rc_; }
    const MwDev &q = c->d;
    const MwIpmDev &p = c->ipm->d;
    const int K = c->K;
    if (x) MWCHECK(hipMemcpy(x, p.x, sizeof(double) * q.xlen * K, hipMemcpyDeviceToHost));
    if (y && q.N) MWCHECK(hipMemcpy(y, p.y, sizeof(double) * q.N * K, hipMemcpyDeviceToHost));
    if (X) MWCHECK(hipMemcpy(X, p.X, sizeof(double) * q.xylen * K, hipMemcpyDeviceToHost));
    if (Y) MWCHECK(hipMemcpy(Y, p.Y, sizeof(double) * q.xylen * K, hipMemcpyDeviceToHost));
    return 0;
}
// objectives and gap of the current iterate, K limbs each: out[0..K-1] d_obj, [K..2K-1] p_obj, [2K..3K-1] gap
extern "C" int clrs_mw_ipm_objectives(clrs_mw_ctx *c, double *out) {
    if (!c || !out || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    MWCHECK(hipSetDevice(c->device));
    { int rc_ = mw_ipm_drain(c); if (rc_) return rc_; }
    const int K = c->K;
    std::vector<double> h((size_t)MSC_COUNT * K);
    MWCHECK(hipMemcpy(h.data(), c->ipm->d.sc, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int l = 0; l < K; l++) {
        out[l] = h[(size_t)l * MSC_COUNT + MSC_DOBJ];
        out[K + l] = h[(size_t)l * MSC_COUNT + MSC_POBJ];
        out[2 * K + l] = h[(size_t)l * MSC_COUNT + MSC_GAP];
    }
    return 0;
}

// ---- test hooks of the step length -------------------------------------------------------------------------------------------------------
// clrs_test_min_eig, forms 0 and 1 (the C entry point and its argument checks: clrs_hip.hip): workgroup b copies the b-th matrix into LDS as k_mwi_step holds
// its W (full storage, leading dimension n) and calls the routine; work space of 3 n + 2 MW_NT doubles behind it, as in k_mwi_step.
__global__ __launch_bounds__(MW_NT) void k_mw_test_min_eig(const double *A, double *out, int n, int form) {
    using namespace mwk;
    lds_d *W = MW_LDS, *work = W + n * n;
    const int tid = threadIdx.x;
    const double *Ag = A + (long)blockIdx.x * n * n;
    for (int e = tid; e < n * n; e += MW_NT) W[e] = Ag[e];
    __syncthreads();
    const double ev = form == 0 ? wg_min_eig32(W, n, work, tid) : wg_min_eig(W, n, work, tid);
    if (tid == 0) out[blockIdx.x] = ev;
}
int mw_test_min_eig_launch(int form, int n, int count, const double *dA, double *dOut) {
    const size_t sm = sizeof(double) * ((size_t)n * n + 3 * (size_t)n + 2 * MW_NT);
    int rc;
    if ((rc = mw_set_lds(k_mw_test_min_eig, sm))) return rc;
    hipLaunchKernelGGL(k_mw_test_min_eig, dim3(count), dim3(MW_NT), sm, nullptr, dA, dOut, n, form);
    MWCHECK(hipGetLastError());
    return 0;
}

// The step-length stage of one iteration on matrices given to it: X, Y, dX, dY (planar limbs, K x xy_len each) go into the iteration's buffers, then the
// Cholesky launch of an iteration (chol X, and chol(Y)^-1 where it rides along) and mw_ipm_launch_step run with the plan the context chose, as the first
// iteration of a solve would run them (limbs of the factor stage: mw_ipm_reset_kf).  eig[2 NB]: what the step kernel left in its eigenvalue buffer
// ((X, dX) of every block, then (Y, dY)); info[8] = {inv_path, W in LDS, tiled products, column panels, limbs of the factors, failure flag, 0, 0}.
// The iterate is overwritten: clrs_mw_ipm_init or clrs_mw_ipm_set before the next solve.  Unsharded contexts.
extern "C" int clrs_mw_test_step_eig(clrs_mw_ctx *c, const double *X, const double *Y, const double *dX, const double *dY, double *eig, int32_t *info) {
    if (!c || !c->ipm || !c->ipm->ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_ipm_create first");
    if (!X || !Y || !dX || !dY || !eig || !info) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (c->d.world > 1 || c->d.gathered) return mw_fail(CLRS_ERR_STATE, "clrs_mw_test_step_eig on a sharded context");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    MwIpm *st = c->ipm;
    const MwIpmDev &p = st->d;
    const size_t bytes = sizeof(double) * (size_t)q.xylen * c->K;
    int rc;
    if ((rc = mw_ipm_drain(c))) return rc;
    MWCHECK(hipMemcpy(p.X, X, bytes, hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(p.Y, Y, bytes, hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(p.dX, dX, bytes, hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(p.dY, dY, bytes, hipMemcpyHostToDevice));
    if ((rc = mw_ipm_arm(c))) return rc;                                       // status words, flags (the failure flag, the counter of finished workgroups)
    MWCHECK(hipMemsetAsync(p.wcnt, 0, sizeof(int) * 2 * q.NB, c->stream));     // the panel counters
    MWCHECK(hipMemsetAsync(p.eig, 0, sizeof(double) * 2 * q.NB, c->stream));
    mw_ipm_reset_kf(c);
    c->d.kf = st->kf_now;
    rc = mw_cholesky_blocks_dev2(c, p.X, p.Xc, st->y_with_x ? p.Y : nullptr, p.Yi, p.yfail);
    if (!rc) rc = mw_ipm_launch_step(c, c->stream);
    const int kf_used = c->d.kf;
    c->d.kf = c->kf_entry;
    if (rc) return rc;
    MWCHECK(hipGetLastError());
    MWCHECK(hipStreamSynchronize(c->stream));
    int flags[8];
    MWCHECK(hipMemcpy(eig, p.eig, sizeof(double) * 2 * q.NB, hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(flags, p.flags, sizeof(flags), hipMemcpyDeviceToHost));
    info[0] = st->y_with_x ? 2 : st->step_inv ? 1 : 0;
    if (info[0] == 2 && st->z_tiled) info[0] = 3;
    info[1] = st->step_w_lds ? 1 : 0; info[2] = st->z_tiled ? 1 : 0; info[3] = st->zs_step; info[4] = kf_used; info[5] = flags[2]; info[6] = info[7] = 0;
    // the launch ended with the step lengths of these matrices in the scalar slots and possibly an error code in the flags: re-armed for what follows
    if ((rc = mw_ipm_arm(c))) return rc;
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

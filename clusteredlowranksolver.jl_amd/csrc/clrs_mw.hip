// clrs_mw.hip -- the hot path at the reference's working precision: multi-word fp64 (K limbs), host side + C ABI
// (include/clrs_hip.h, clrs_mw_*).  Compiled with -ffp-contract=off (clrs_mw_arith.h) and linked into libclrs_hip.so.
//
// A context of its own (clrs_mw_ctx), created from the same clrs_sdp_desc as the fp64 context: the de-duplication of
// the sampled vectors (precompute_matrices_bilinear_pairings, src/solver.jl:985-1059) is redone into ONE table of
// expanded unique vectors per PSD block by the host-only table builder (clrs_mw_tables.h, which says what the tables
// hold); creation here is the sequence of stages around it (clrs_mw_create_opts).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_mw_kernels.hip.h"
#include "clrs_mw_pipe.hip.h"
#include "clrs_mw_exact.hip.h"
#include "clrs_mw_ipm.hip.h"
#include "clrs_mw_rank.hip.h"
#include "clrs_mw_gemm.hip.h"
#include "clrs_mw_posv.hip.h"
#include "clrs_mw_kernel_vectors.hip.h"
#include "clrs_mw_rational.hip.h"
#include "clrs_mw_inst.h"
#include "clrs_mw_tables.h"      // host only: mw_build_tables, mw_cut_digits
#ifdef MW_SPLIT_UNITS        // the kernels of these limb counts are compiled in units of their own (clrs_mw_inst.hip)
MW_KERNELS_ALL(extern template, 4)
MW_KERNELS_ALL(extern template, 5)
MW_KERNELS_ALL(extern template, 6)
MW_KERNELS_ALL(extern template, 8)
MW_KERNELS_ALL(extern template, 10)
#endif

typedef long long i64;

extern int g_cfg_mw_zi_narrow;        // clrs_hip.hip, clrs_config_set("mw_zi_narrow", 0 / 1)
extern int g_cfg_mw_xinv_product;     // clrs_hip.hip, clrs_config_set("mw_xinv_product", 0 / 1)
extern int g_cfg_mw_chain_hop, g_cfg_mw_skip_xfb, g_cfg_mw_y_riders;   // clrs_hip.hip, clrs_config_set("mw_chain_hop", 0 / 1 / 2), ("mw_skip_xfb", 0 / 1), ("mw_y_riders", 0 / 1)
extern int g_cfg_mw_stream_words;                        // clrs_hip.hip, clrs_config_set("mw_stream_words", 0 / 1); env CLRS_MW_STREAM_WORDS
extern int g_cfg_mw_pipeline64;                          // clrs_hip.hip, clrs_config_set("mw_pipeline64", 0 / 1): the 64-row form for clusters of 33 .. 64 rows
extern int g_cfg_mw_zt_small_maxn;                       // clrs_hip.hip, clrs_config_set("mw_zt_small_maxn", rows): k_mw_zt with two columns per workgroup and eight lanes per entry up to this block side
extern int g_cfg_mw_pipeline_x, g_cfg_mw_pipeline_x_min; // clrs_hip.hip, clrs_config_set("mw_pipeline_x", 0 / 1), ("mw_pipeline_x_min", rows): the Cholesky of the X blocks through the pipelines
extern int g_cfg_mw_sharded_factor_limbs;                // clrs_hip.hip, clrs_config_set("mw_sharded_factor_limbs", 0 / 1)
extern int g_cfg_mw_pipeline;                            // clrs_hip.hip, clrs_config_set("mw_pipeline", 0 / 1): read at context creation
extern int g_cfg_mw_refine_predictor;                    // clrs_hip.hip, clrs_config_set("mw_refine_predictor", 0 / 1)
extern int g_cfg_mw_refine;                              // clrs_hip.hip, clrs_config_set("mw_refine", 0 / 1): read at context creation
extern int g_cfg_mw_exact_products;                      // clrs_hip.hip, clrs_config_set("mw_exact_products", 0 / 1 / 2): read at context creation
extern int g_cfg_mw_affine_corrector;                    // clrs_hip.hip, clrs_config_set("mw_affine_corrector", 0 / 1): read by clrs_mw_ipm_create
extern int g_cfg_mw_factor_limbs;                        // clrs_hip.hip, clrs_config_set("mw_factor_limbs", 0 / limbs): read at context creation
extern "C" void clrs_set_last_error(const char *msg);   // clrs_hip.hip: the library keeps one thread-local message

static int mw_fail(int code, const std::string &msg) {
    clrs_set_last_error(msg.c_str());
    return code;
}
#define MWCHECK(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return mw_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// RCCL is bound at run time (dlopen): a process that already holds a copy (PyTorch ships one) keeps using that copy, and the
// library loads on machines without RCCL.
typedef struct { char internal[128]; } mw_nccl_id;
struct MwNccl {
    void *lib = nullptr;
    int (*GetUniqueId)(mw_nccl_id *) = nullptr;
    int (*CommInitRank)(void **, int, mw_nccl_id, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
static MwNccl g_nccl;
static int mw_nccl_load() {
    if (g_nccl.lib) return 0;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;      // a copy the process already has
    for (const char *n : names) { if (h) break; h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); }
    if (!h) return mw_fail(CLRS_ERR_INVALID, std::string("RCCL is not available: ") + dlerror());
    g_nccl.GetUniqueId = (int (*)(mw_nccl_id *))dlsym(h, "ncclGetUniqueId");
    g_nccl.CommInitRank = (int (*)(void **, int, mw_nccl_id, int))dlsym(h, "ncclCommInitRank");
    g_nccl.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    g_nccl.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(h, "ncclAllGather");
    g_nccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_nccl.GetUniqueId || !g_nccl.CommInitRank || !g_nccl.CommDestroy || !g_nccl.AllGather) return mw_fail(CLRS_ERR_INVALID, "RCCL symbols missing");
    g_nccl.lib = h;
    return 0;
}
#define NCCLCHECK(expr)                                                                                                          \
    do {                                                                                                                         \
        int r_ = (expr);                                                                                                         \
        if (r_ != 0) return mw_fail(CLRS_ERR_HIP, std::string(#expr) + ": " + (g_nccl.GetErrorString ? g_nccl.GetErrorString(r_) : "RCCL error")); \
    } while (0)
static const int MW_NCCL_FLOAT64 = 8;      // ncclFloat64 / ncclDouble

// In-process stand-in for a communicator: `world` contexts of ONE process that share one device, driven by one host thread each
// (the two-shards-on-one-GPU tests; a box has one GPU, and RCCL refuses two ranks on one device).  An all-gather is: every rank
// records "my slot is written" on its stream, the host threads meet, every rank copies the peers' slots device to device behind the
// peers' events, records "I have read", the host threads meet again and every rank orders its stream behind the peers' reads (a
// slot is rewritten every iteration).  Two channels, like the two RCCL communicators of a context: one per stream that exchanges.
struct clrs_mw_local_group {
    int world = 0;
    int attached = 0;                   // contexts that point to this group (clrs_mw_comm_init_local / clrs_mw_comm_destroy, clrs_mw_destroy)
    std::mutex m;
    std::condition_variable cv;
    struct Chan {
        int arrived = 0;
        long gen = 0;
        std::vector<double *> base;
        std::vector<hipEvent_t> ready, copied;
    } ch[2];
    void barrier(int k) {
        std::unique_lock<std::mutex> lk(m);
        Chan &c = ch[k];
        const long g = c.gen;
        if (++c.arrived == world) { c.arrived = 0; c.gen++; cv.notify_all(); }
        else cv.wait(lk, [&] { return c.gen != g; });
    }
};

static const size_t MW_LDS_MAX = 160 * 1024 - 2048;     // bytes of LDS one workgroup may claim on gfx950 (margin for the runtime)

struct clrs_mw_ctx {
    int device = 0, K = 4, DK = 1;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    MwDev d = {};
    std::vector<MwBlk> blk;
    std::vector<MwClu> clu;
    std::vector<void *> allocs;
    int maxU = 0, maxP = 0, maxn = 0, maxn_dense = 0;
    bool all_inv = false;               // every low-rank block has its inverse factor (k.inv != 0)
    bool xinv_valid = false;            // Xi holds the inverses of the current Cholesky factors (they come from k_mw_potrf_x, not from the caller)
    bool lds_x = false, lds_q = false, lds_zt_L = false, dense_two = false;
    int nw_factor = 1;                  // workgroups per cluster in k_mw_factor (they share out the columns of the inverse factor)
    int maxcnt = 0;
    double *vz = nullptr;               // 2 N numbers of scratch of the solve stage over many workgroups (k_mw_solve_wide)
    bool wide_solve = false;            // some cluster or Q has more than 64 rows: the products of the solve stage are launches of their own
    const double *ride_fwd = nullptr;   // set by the iteration around clrs_mw_schur_factor_finish_dev: rhs_x of the solve that follows
    const int *ride_wait = nullptr;     // ... and, with it, the word its workgroups wait for inside the launch (>= ride_wait_value) instead of an event in front of it
    int ride_wait_value = 0;
    bool fwd_rode = false;              // ... and its first product pair (k_mw_solve_fwd's work) was done on the launch of k_mw_potrf_q
    int n_one_term = 0, n_many_term = 0;   // clusters whose S_j goes through k_mw_saccum_one / through the general k_mw_saccum
    int sa_lanes = MW_SA_W;             // lanes per entry of k_mw_saccum: 1, 2 or 4 by the largest block count of a cluster
    int maxTb = 0;                      // most low-rank terms in one PSD block
    size_t sm_x = 0, sm_zt = 0, sm_dense = 0, sm_factor = 0, sm_q = 0, sm_fwd = 0, sm_mid = 0, sm_bwd = 0;
    int *h_info = nullptr;               // pinned
    double *d_Xin = nullptr, *d_Xc = nullptr, *d_Y = nullptr, *d_rx = nullptr, *d_ry = nullptr, *d_dx = nullptr, *d_dy = nullptr;   // staging of the host-pointer entry points
    bool assembled = false, factored = false;
    bool timing = false;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double times[6] = {0, 0, 0, 0, 0, 0};
    double cnt_mul = 0;                  // multi-word multiply-adds of one assembly (algorithmic)
    double cnt_factor = 0, cnt_solve = 0;
    struct MwIpm *ipm = nullptr;
    size_t sm_bp_diag = 0, sm_bp_panel = 0, sm_bp_inv = 0;   // LDS of the blocked factorisation (k_mw_bp_*)
    std::vector<MwBp> bp_S, bp_Q;       // the matrices of the blocked path: the clusters beyond LDS, and Q (when it is)
    const MwBp *d_bp = nullptr;         // both lists on the device, bp_S first
    bool any_lds_cluster = false;
    void *comm = nullptr;                // ncclComm_t when the library does the exchanges itself (clrs_mw_comm_init): the context's stream
    void *comm_side = nullptr;           // a second communicator for the exchanges of the iteration's side stream (clrs_mw_comm_init_side)
    clrs_mw_local_group *lgroup = nullptr;   // or: the in-process group (clrs_mw_comm_init_local)
    bool local_factored = false, fwd_done = false;
    const double *split_rhs_x = nullptr;   // right-hand side of the last clrs_mw_schur_solve_fwd_dev (the refinement's residual needs it)
    bool refine_ready = false;             // clrs_mw_schur_solve_bwd_dev left the first half of a refinement step behind
    MwdDev mwd = {};                     // static digits of the dense matrices of the blocks k_mwx_dense takes
    int mwd_blocks = 0, mwd_tasks = 0;
    size_t sm_mwd = 0;
    MwxDev mwx = {};                     // digits of V (static), Z, T of the blocks whose pairing matrices go through k_mwx_slice / k_mwx_gram
    int mwx_blocks = 0, mwx_maxU16 = 0;
    MwsDev mws = {};                     // static V slices of the blocks the exact-product kernel takes
    int mws_blocks = 0;                  // how many
    int mws_turns = 1;                   // 2: some eligible block has more than four T / Z tiles
    size_t sm_mws = 0;
    bool pipe_bp = false;                // the diagonal blocks of the blocked factorisation as pipelines (k_mw_bp_diag_pipe)
    bool pipe_S64 = false;               // ... the clusters' S_j of 33 .. 64 rows through the 64-row form of the pipeline (k_mw_factor_pipe64; limbs <= 6)
    bool pipe_X = false;                 // ... the Cholesky of the X blocks (and of the Y blocks beside it) through the pipelines (k_mw_potrf_x_pipe): every block with its explicit inverse factor, <= 64 rows
    unsigned long long *pipe_pcx = nullptr;    // its hand-off granules: [2 NB][MWP_PC_WORDS_N(K, 64)]
    double *xpipe_L = nullptr, *xpipe_rd = nullptr;   // where the factors / reciprocal diagonals of the Y blocks go (only their inverses are kept)
    int *xpipe_info = nullptr;
    bool pipe_S = false, pipe_Q = false;  // the factorisations of the clusters / of Q as pipelines of workgroups (clrs_mw_pipe.hip.h): every matrix <= 32 rows, few clusters
    unsigned long long *pipe_pc64 = nullptr;   // hand-off granules of k_mw_factor_pipe64: [J][MWP_PC_WORDS_N(K, 64)]
    int pipe_pcQ = 0;                    // index of Q's hand-off region in pipe_pc
    unsigned pipe_epoch = 0;             // launch counter: the tag of the hand-off granules
    bool stream_words = true;            // the interior-point iteration synchronises its two streams through words (clrs_mw_ipm_host.inc) where it can; false: events only
    bool y_riders = true;                // the iteration may form the Y pairings on the Cholesky launch (clrs_config_set("mw_y_riders", ..) when the context was created)
    const double *ride_y = nullptr;      // set by the iteration around its Cholesky of the X blocks: the Y of the assembly that follows, whose pairings ride on that launch
    bool zi_narrow = true;               // k_mwi_Zi with 256 threads and panels of half the width where clrs_mw_zi_panels.h allows it (clrs_config_set("mw_zi_narrow", ..) when the context was created)
    bool xinv_product = true;            // k_mwi_Zi applies X^-1 as one product with Xv = Xi^T Xi, formed once per iteration (MwIpmDev::Xv; clrs_config_set("mw_xinv_product", ..) when the context was created)
    int chain_hop = 1;                   // form of the in-launch hand-offs of k_mwi_Zi / k_mwi_step (MwIpmDev::hop; clrs_config_set("mw_chain_hop", ..) when the context was created)
    bool refine_skip_next = false;       // the interior-point iteration's PREDICTOR solve: one pass (set by clrs_mw_ipm_host.inc for the next clrs_mw_schur_solve_dev only)
    int refine_predictor = 0;            // clrs_mw_options.refine_predictor: 1 = the predictor's solve is refined like every other
    int refine = 1;                      // iterative refinement of the solve stage (clrs_mw_options / clrs_config_set("mw_refine")): 0 off, 1 one step with the correction in all K limbs, 2 ... in mw_kc(K) limbs
    bool ipm_arms_info = false;          // inside the device-resident iteration the status words are re-armed by a kernel, not by a memset per call
    // Mixed-precision refinement (MwDev::kf, mw_kf_of): kf_low = the reduced limb count this context may run its factor stage and the products of its solve
    // stage in (K: it may not -- limb counts without a reduced form, refinement off or in fewer limbs, blocked / row-parallel paths); kf_entry = what the
    // stand-alone entry points use (clrs_mw_options.factor_limbs: 0 = K there and kf_low, adaptively, inside clrs_mw_ipm_*; explicit: that count everywhere)
    int kf_low = 0, kf_entry = 0;
};

template <class T>
static int mw_upload(clrs_mw_ctx *c, const std::vector<T> &h, const T **d) {
    T *p = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    MWCHECK(hipMalloc((void **)&p, bytes));
    c->allocs.push_back(p);
    if (!h.empty()) MWCHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *d = p;
    return 0;
}
static int mw_dmalloc(clrs_mw_ctx *c, double **d, i64 n) {
    size_t bytes = (size_t)std::max<i64>(n, 1) * sizeof(double);
    MWCHECK(hipMalloc((void **)d, bytes));
    c->allocs.push_back(*d);
    MWCHECK(hipMemset(*d, 0, bytes));
    return 0;
}

// dispatch over the limb count K of the computed numbers and DK of the problem data (1: fp64, 2: double-double)
#define MW_CASE(Kc, Dc, ...) if (c_K_ == Kc && c_D_ == Dc) { constexpr int KK = Kc; constexpr int DD = Dc; __VA_ARGS__; } else
#define MW_DISPATCH(ctx, ...)                                                                                       \
    do {                                                                                                            \
        const int c_K_ = (ctx)->K, c_D_ = (ctx)->DK;                                                                \
        MW_CASE(2, 1, __VA_ARGS__) MW_CASE(2, 2, __VA_ARGS__) MW_CASE(3, 1, __VA_ARGS__) MW_CASE(3, 2, __VA_ARGS__)  \
        MW_CASE(4, 1, __VA_ARGS__) MW_CASE(4, 2, __VA_ARGS__) MW_CASE(5, 1, __VA_ARGS__) MW_CASE(5, 2, __VA_ARGS__)  \
        MW_CASE(6, 1, __VA_ARGS__) MW_CASE(6, 2, __VA_ARGS__) MW_CASE(8, 1, __VA_ARGS__) MW_CASE(8, 2, __VA_ARGS__)  \
        MW_CASE(10, 1, __VA_ARGS__) MW_CASE(10, 2, __VA_ARGS__)                                                      \
        MW_CASE(3, 3, __VA_ARGS__) MW_CASE(4, 4, __VA_ARGS__) MW_CASE(5, 5, __VA_ARGS__) MW_CASE(6, 6, __VA_ARGS__)  \
        MW_CASE(8, 8, __VA_ARGS__) MW_CASE(10, 10, __VA_ARGS__)                                                      \
        return mw_fail(CLRS_ERR_INVALID, "limbs must be 2..6, 8 or 10 and data limbs 1, 2 or the limbs");           \
    } while (0)

template <class F>
static int mw_set_lds(F kernel, size_t bytes) {
    if (bytes > 48 * 1024) MWCHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

extern "C" void clrs_mw_destroy(clrs_mw_ctx *c);
static void mw_ipm_free(clrs_mw_ctx *c);
static int mw_launch_xrd(clrs_mw_ctx *c, const double *d_Xc);

extern "C" int clrs_mw_create_opts(const clrs_sdp_desc *d, int data_limbs, int device, int limbs, const clrs_mw_options *opts, clrs_mw_ctx **out);
extern "C" int clrs_mw_create(const clrs_sdp_desc *d, int device, int limbs, clrs_mw_ctx **out) {
    return clrs_mw_create_opts(d, 1, device, limbs, nullptr, out);
}
extern "C" int clrs_mw_create_ex(const clrs_sdp_desc *d, int data_limbs, int device, int limbs, clrs_mw_ctx **out) {
    return clrs_mw_create_opts(d, data_limbs, device, limbs, nullptr, out);
}

// ---- context creation: clrs_mw_create_opts is the sequence of the stages below; a stage returns 0 or the error code (its message is set), and the
// caller's guard destroys the half-built context on every failure ----
#define MW_RET(call) do { if (int rc_ = (call)) return rc_; } while (0)
static int mw_hip(hipError_t e, const char *what) {
    return e == hipSuccess ? 0 : mw_fail(CLRS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// `count` elements with every byte set to `byte`, owned by the context
template <class T>
static int mw_alloc_fill(clrs_mw_ctx *c, T **p, size_t count, int byte) {
    if (hipMalloc((void **)p, count * sizeof(T)) != hipSuccess) return mw_fail(CLRS_ERR_HIP, "hipMalloc failed");
    c->allocs.push_back(*p);
    if (hipMemset(*p, byte, count * sizeof(T)) != hipSuccess) return mw_fail(CLRS_ERR_HIP, "hipMemset failed");
    return 0;
}

// opts: per-context choices (a field < 0, or opts == NULL: the process-wide default of clrs_config_set) -- contexts created side by side from
// several threads do not share a knob this way
struct MwOpts { int exact, refine, pipe, refine_pred, factor_limbs, km; };
static int mw_resolve_opts(const clrs_mw_options *opts, int limbs, int data_limbs, MwOpts &o) {
    o.exact = opts && opts->exact_products >= 0 ? opts->exact_products : g_cfg_mw_exact_products;
    o.refine = opts && opts->refine >= 0 ? opts->refine : g_cfg_mw_refine;
    o.pipe = opts && opts->pipeline >= 0 ? opts->pipeline : g_cfg_mw_pipeline;
    o.refine_pred = opts && opts->refine_predictor >= 0 ? opts->refine_predictor : g_cfg_mw_refine_predictor;
    o.factor_limbs = opts && opts->factor_limbs >= 0 ? opts->factor_limbs : g_cfg_mw_factor_limbs;
    // matmul_prec of the reference (src/solver.jl:125): limbs of the pairing products, rounded UP to the next count on offer (mw_km_ok); 0 = the context's limbs
    o.km = opts && opts->matmul_limbs > 0 ? opts->matmul_limbs : limbs;
    if (o.km > limbs) o.km = limbs;
    while (o.km < limbs && !mw_km_ok(limbs, o.km)) o.km++;
    if (data_limbs > 2) o.exact = 0;                     // (the static digits of the exact slice products are cut from two data limbs)
    if (o.km < limbs) o.exact = 0;                       // (the exact slice products have one slice count per limb count: the expansion kernels take the reduced products)
    if (o.exact > 2 || o.refine > 2) return mw_fail(CLRS_ERR_INVALID, "clrs_mw_options: exact_products and refine are 0, 1 or 2 (or < 0 for the default)");
    if (limbs < 2 || limbs > 10 || limbs == 7 || limbs == 9) return mw_fail(CLRS_ERR_INVALID, "limbs must be 2..6, 8 or 10");
    if (data_limbs < 1 || data_limbs > limbs || (data_limbs > 2 && data_limbs != limbs))
        return mw_fail(CLRS_ERR_INVALID, "data limbs must be 1, 2 or the context's limbs (the problem data at the working precision: src/interface.jl:1078-1112)");
    return 0;
}

static int mw_stage_stream(clrs_mw_ctx *c) {
    {   // The context's stream at the HIGHEST priority, the side stream of the interior-point iteration (clrs_mw_ipm_host.inc) at the default one: the runtime
        // maps streams onto a few hardware queues PER PRIORITY (GPU_MAX_HW_QUEUES, 4 by default), and two streams of one iteration that land on one queue run
        // its packets in submission order -- measured: the second context of a process, whose side stream shared a queue, 0.58 ms per iteration against
        // 0.45 (profiles/r05).  Different priorities never share; and the main stream carries the longest chain of the iteration.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; (void)hipGetLastError(); }
        if (hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest) != hipSuccess) return mw_fail(CLRS_ERR_HIP, "hipStreamCreateWithPriority failed");
    }
    if (hipHostMalloc((void **)&c->h_info, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) return mw_fail(CLRS_ERR_HIP, "hipHostMalloc failed");
    return 0;
}

// the block and cluster records move into the context (the LDS plans below fill MwBlk::inv and MwClu::lds), the sizes and counters are copied
static void mw_adopt_tables(clrs_mw_ctx *c, MwTables &t) {
    c->blk.swap(t.blk); c->clu.swap(t.clu);
    c->maxU = t.maxU; c->maxP = t.maxP; c->maxn = t.maxn; c->maxn_dense = t.maxn_dense; c->maxTb = t.maxTb; c->maxcnt = t.maxcnt;
    c->sa_lanes = t.sa_lanes; c->n_one_term = t.n_one_term; c->n_many_term = t.n_many_term;
    c->cnt_mul = t.cnt_mul; c->cnt_factor = t.cnt_factor; c->cnt_solve = t.cnt_solve;
    c->wide_solve = c->maxP > 64 || t.N > 64;
}

static int mw_stage_lds(clrs_mw_ctx *c, const MwTables &t) {
    const int K = c->K, J = t.J, N = t.N;
    const size_t lim = MW_LDS_MAX / sizeof(double);
    {
        size_t nn = (size_t)c->maxn * c->maxn * K;
        size_t bcw = MW_POTRF_SCR(K, (size_t)c->maxn);       // scratch of wg_potrf
        c->lds_x = nn + bcw <= lim;
        size_t xneed = (c->lds_x ? nn : 0) + bcw;
        for (auto &k : c->blk) {                            // X blocks whose factor and its inverse fit side by side: Xi is formed
            const size_t one = (size_t)k.n * k.n * K + MW_POTRF_SCR(K, (size_t)k.n) + (size_t)K * k.n;   // + a reciprocal diagonal (the Y workgroups of the iteration)
            const size_t two = one + (size_t)MW_TRI(k.n) * K;                // + the packed inverse factor
            k.inv = !c->lds_x ? 0 : two <= lim ? 1 : one <= lim ? 2 : 0;       // the inverse in LDS beside the factor, or in place in memory
            if (k.inv) xneed = std::max(xneed, k.inv == 1 ? two : one);
        }
        c->all_inv = !c->blk.empty();
        for (auto &k : c->blk) c->all_inv = c->all_inv && (k.kind != 0 || k.inv != 0);
        c->sm_x = xneed * 8;
        size_t zt = (size_t)c->maxn * MW_CT * K;
        c->lds_zt_L = zt + nn <= lim;
        c->sm_zt = (zt + (c->lds_zt_L ? nn : 0)) * 8;
        if (zt > lim) return mw_fail(CLRS_ERR_INVALID, "PSD block too large for the multi-word kernels");
        size_t maxnd = 0;
        for (auto &k : c->blk) if (k.kind != 0 && k.n > 1) maxnd = std::max(maxnd, (size_t)k.n);
        if (maxnd * maxnd * K > lim) return mw_fail(CLRS_ERR_INVALID, "dense block too large for the multi-word kernels");
        c->dense_two = 2 * maxnd * maxnd * K <= lim;        // room for the two buffers of the product form of X^-1 A
        c->sm_dense = (c->dense_two ? 2 : 1) * maxnd * maxnd * K * 8;
        size_t fmax = 0;
        for (auto &q : c->clu) {                        // S_j and the inverse of its factor side by side in LDS, or the blocked path
            const size_t need = ((size_t)q.P * q.P + (size_t)MW_TRI(q.P)) * K + MW_POTRF_SCR(K, (size_t)q.P);
            q.lds = need <= lim ? 1 : 0;
            if (q.lds) fmax = std::max(fmax, need);
        }
        c->sm_factor = std::max<size_t>(fmax, 1) * 8;
        c->nw_factor = std::max(1, std::min(MW_INV_WG, 256 / std::max(J, 1)));     // only while the clusters leave compute units idle
        c->sm_fwd = 2 * (size_t)c->maxP * K * 8;
        c->sm_bwd = 3 * (size_t)c->maxP * K * 8;              // (three vectors: the refinement's first half rides on the backward launch)
        const size_t qn = (size_t)N * N * K;
        const size_t qneed = qn + (size_t)MW_TRI(N) * K + MW_POTRF_SCR(K, (size_t)N);
        c->lds_q = qneed <= lim;
        c->sm_q = (c->lds_q ? qneed : 1) * 8;
        c->sm_mid = 2 * (size_t)std::max(N, 1) * K * 8;
        if (c->sm_fwd > MW_LDS_MAX || c->sm_mid > MW_LDS_MAX) return mw_fail(CLRS_ERR_INVALID, "cluster too large for the multi-word solve kernels");
    }
    MW_DISPATCH(c, {
        MW_RET(mw_set_lds(k_mw_potrf_x<KK>, c->sm_x)); MW_RET(mw_set_lds((k_mw_potrf_x_ride<KK, DD>), c->sm_x)); MW_RET(mw_set_lds(k_mw_zt<KK, DD>, c->sm_zt)); MW_RET(mw_set_lds((k_mw_dense_t<KK, DD>), c->sm_dense));
        // (only what can be launched: Q beyond LDS never rides k_mw_potrf_q, and systems whose dy and three cluster vectors exceed LDS take the
        // row-parallel solve (k_mw_solve_wide) -- sharded, they are refused at the launch, not here)
        constexpr int KC = mw_kc(KK);
        const size_t bw = std::min(c->sm_mid + c->sm_bwd, MW_LDS_MAX);
        MW_RET(mw_set_lds(k_mw_factor<KK>, c->sm_factor)); MW_RET(mw_set_lds(k_mw_potrf_q<KK>, c->lds_q ? std::max(c->sm_q, c->sm_fwd) : c->sm_fwd));
        MW_RET(mw_set_lds(k_mw_solve_fwd<KK>, c->sm_fwd)); MW_RET(mw_set_lds((k_mw_solve_mid<KK, KK>), c->sm_mid)); MW_RET(mw_set_lds((k_mw_solve_mid<KK, KC>), c->sm_mid));
        MW_RET(mw_set_lds((k_mw_solve_bwd<KK, KK, DD, 0>), bw)); MW_RET(mw_set_lds((k_mw_solve_bwd<KK, KK, DD, 1>), bw)); MW_RET(mw_set_lds((k_mw_solve_bwd<KK, KK, DD, 2>), bw));
        MW_RET(mw_set_lds((k_mw_solve_bwd<KK, KC, DD, 1>), bw)); MW_RET(mw_set_lds((k_mw_solve_bwd<KK, KC, DD, 2>), bw));
    });
    return 0;
}

// the static digits of a column of n numbers of V or of a dense matrix: data(l, i) = plane l of entry i; the column's window exponent goes to *e_out,
// every digit to put(i, s, digit)
template <class DATA, class PUT>
static void mw_cut_column(int n, int DK, int S, DATA &&data, int *e_out, PUT &&put) {
    double mx = 0;
    for (int i = 0; i < n; i++) mx = std::max(mx, std::fabs(data(0, i)));
    const int e = *e_out = mwk::mws_exponent(mx);
    for (int i = 0; i < n; i++)
        mw_cut_digits(data(0, i), DK > 1 ? data(1, i) : 0.0, e, S, [&](int s, float dgt) { put(i, s, dgt); });
}

// ---- exact-product path (clrs_mw_exact.hip.h): static slices of V of the eligible blocks; mws_off[b] >= 0: block b goes through k_mws_pair ----
static int mw_stage_mws(clrs_mw_ctx *c, const MwTables &t, const MwOpts &o, std::vector<long long> &mws_off) {
    const int K = c->K, DK = c->DK, NB = t.NB;
    mws_off.assign((size_t)std::max(NB, 1), -1);
    const int S = mws_slices(K);
    std::vector<float> hVs;
    std::vector<int> hVe, hve_off((size_t)std::max(NB, 1), 0), hsv((size_t)std::max(NB, 1), 0);
    for (int b = 0; b < NB; b++) {
        const MwBlk &k = c->blk[b];
        if (k.kind != 0 || !k.inv || k.n > 32) continue;
        const int n = k.n, U = k.U, np = (n + 3) & ~3, n16 = (n + 15) & ~15, U16 = (U + 15) & ~15, rV = mws_rowstride(U16);
        if ((n16 / 16) * (U16 / 16) > 4 || mws_lds_bytes(S, mws_sv_class(S, 1), n, U) > MW_LDS_MAX) continue;
        if (2 * (n16 / 16) * (U16 / 16) > 4) c->mws_turns = 2;
        mws_off[b] = (long long)hVs.size();
        hve_off[b] = (int)hVe.size();
        hVs.resize(hVs.size() + (size_t)S * np * rV, 0.0f);
        hVe.resize(hVe.size() + U16, 0);
        float *dst = hVs.data() + mws_off[b];
        int sv = 0;
        for (int u = 0; u < U; u++)
            mw_cut_column(n, DK, S, [&](int l, int i) { return t.V[(size_t)l * t.Vp + k.v_off + (i64)u * n + i]; }, &hVe[hve_off[b] + u], [&](int i, int s, float dgt) {
                dst[(size_t)s * np * rV + (size_t)i * rV + mws_col(i, u, U16)] = dgt;      // [s][k = row i of V][col = u]
                if (dgt != 0.0f) sv = std::max(sv, s + 1);
            });
        if (mws_lds_bytes(S, mws_sv_class(S, sv), n, U) > MW_LDS_MAX) {      // (the test above assumed the fewest slices of V)
            hVs.resize((size_t)mws_off[b]); hVe.resize((size_t)hve_off[b]);
            mws_off[b] = -1;
            continue;
        }
        hsv[b] = sv;
        c->mws_blocks++;
        c->sm_mws = std::max(c->sm_mws, mws_lds_bytes(S, mws_sv_class(S, sv), n, U));
    }
    const bool on = o.exact == 2 ? c->mws_blocks > 0 : (o.exact == 1 && c->mws_blocks >= 256);
    if (!on) { c->mws_blocks = 0; std::fill(mws_off.begin(), mws_off.end(), -1); }
    else {
        MW_RET(mw_upload(c, hVs, &c->mws.Vs)); MW_RET(mw_upload(c, hVe, &c->mws.Vexp));
        MW_RET(mw_upload(c, hve_off, &c->mws.ve_off)); MW_RET(mw_upload(c, hsv, &c->mws.sv));
        MW_DISPATCH(c, { if constexpr (DD <= 2) { MW_RET(mw_set_lds((k_mws_pair<KK, DD, 1>), c->sm_mws)); MW_RET(mw_set_lds((k_mws_pair<KK, DD, 2>), c->sm_mws)); } });
    }
    return mw_upload(c, mws_off, &c->mws.vs_off);
}

// ---- pairing matrices of blocks of any size through digits in global memory (k_mwx_slice, k_mwx_gram): blocks without sub-blocks that
// k_mws_pair does not take and that have enough unique vectors for their U x U Gram products to matter ----
static int mw_stage_mwx(clrs_mw_ctx *c, const MwTables &t, const MwOpts &o, const std::vector<long long> &mws_off) {
    const int K = c->K, DK = c->DK, NB = t.NB;
    std::vector<long long> mwx_off((size_t)std::max(NB, 1), -1);
    if (o.exact == 0) return mw_upload(c, mwx_off, &c->mwx.d_off);
    const int S = mws_slices(K);
    std::vector<float> hVd;
    std::vector<int> heV, he_off((size_t)std::max(NB, 1), 0), hsv((size_t)std::max(NB, 1), 0);
    for (int b = 0; b < NB; b++) {
        const MwBlk &k = c->blk[b];
        if (k.kind != 0 || k.m != 1 || mws_off[b] >= 0) continue;
        if (k.U < (o.exact == 2 ? 16 : 64) || k.n < 8) continue;
        const int n = k.n, U = k.U, np = (n + 3) & ~3, U16 = (U + 15) & ~15;
        mwx_off[b] = (long long)hVd.size();
        he_off[b] = (int)heV.size();
        hVd.resize(hVd.size() + (size_t)S * np * U16, 0.0f);
        heV.resize(heV.size() + U16, 0);
        float *dst = hVd.data() + mwx_off[b];
        int sv = 0;
        for (int u = 0; u < U; u++)
            mw_cut_column(n, DK, S, [&](int l, int i) { return t.V[(size_t)l * t.Vp + k.v_off + (i64)u * n + i]; }, &heV[he_off[b] + u], [&](int i, int s, float dgt) {
                dst[(size_t)s * np * U16 + (size_t)i * U16 + u] = dgt;
                if (dgt != 0.0f) sv = std::max(sv, s + 1);
            });
        hsv[b] = sv;
        c->mwx_blocks++;
        c->mwx_maxU16 = std::max(c->mwx_maxU16, U16);
    }
    if (c->mwx_blocks > 0) {
        MW_RET(mw_upload(c, hVd, &c->mwx.Vd)); MW_RET(mw_upload(c, heV, &c->mwx.eV));
        MW_RET(mw_upload(c, he_off, &c->mwx.e_off)); MW_RET(mw_upload(c, hsv, &c->mwx.sv));
        double *zd = nullptr, *td = nullptr, *ez = nullptr, *et = nullptr;      // (the allocator counts doubles)
        MW_RET(mw_dmalloc(c, &zd, (i64)(hVd.size() + 1) / 2)); MW_RET(mw_dmalloc(c, &td, (i64)(hVd.size() + 1) / 2));
        MW_RET(mw_dmalloc(c, &ez, (i64)(heV.size() + 1) / 2)); MW_RET(mw_dmalloc(c, &et, (i64)(heV.size() + 1) / 2));
        c->mwx.Zd = (float *)zd; c->mwx.Td = (float *)td; c->mwx.eZ = (int *)ez; c->mwx.eT = (int *)et;
        MW_RET(mw_hip(hipMemset(zd, 0, hVd.size() * sizeof(float)), "hipMemset")); MW_RET(mw_hip(hipMemset(td, 0, hVd.size() * sizeof(float)), "hipMemset"));      // the padding rows and columns stay zero
        MW_RET(mw_hip(hipMemset(ez, 0, heV.size() * sizeof(int)), "hipMemset")); MW_RET(mw_hip(hipMemset(et, 0, heV.size() * sizeof(int)), "hipMemset"));
    }
    return mw_upload(c, mwx_off, &c->mwx.d_off);
}

// ---- dense blocks with 16 < n <= 32 and inverse factors: X^-1 (A_e Y) through exact slice products (k_mwx_dense), static digits of the A_e ----
static int mw_stage_mwd(clrs_mw_ctx *c, const MwTables &t, const MwOpts &o) {
    const int K = c->K, DK = c->DK, NB = t.NB;
    std::vector<long long> mwd_off((size_t)std::max(NB, 1), -1);
    if (o.exact == 0 || K > 6) return mw_upload(c, mwd_off, &c->mwd.a_off);
    const int S = mws_slices(K), S1 = (S + 1) / 2, sN = 32 * 32;
    std::vector<float> hAd;
    std::vector<int> heA, he_off((size_t)std::max(NB, 1), 0);
    for (int b = 0; b < NB; b++) {
        const MwBlk &k = c->blk[b];
        if (k.kind == 0 || !k.inv || k.n <= 16 || k.n > 32 || k.cnt <= 0) continue;
        const int n = k.n;
        const size_t base = hAd.size(), ebase = heA.size();
        hAd.resize(base + (size_t)k.cnt * S1 * sN, 0.0f);
        heA.resize(ebase + (size_t)k.cnt * 32, 0);
        bool fits = true;
        for (int e = 0; e < k.cnt && fits; e++) {
            float *dst = hAd.data() + base + (size_t)e * S1 * sN;
            const i64 a0 = k.a_off + (i64)e * n * n;
            for (int col = 0; col < n; col++)
                mw_cut_column(n, DK, S, [&](int l, int kk) { return t.dA[(size_t)l * t.dAp + a0 + kk + (i64)col * n]; }, &heA[ebase + (size_t)e * 32 + col], [&](int kk, int s, float dgt) {
                    if (s < S1) dst[(size_t)s * sN + (size_t)kk * 32 + mws_col(kk, col, 32)] = dgt;
                    else if (dgt != 0.0f) fits = false;      // data beyond the slices kept: leave the block to the expansion kernels
                });
        }
        if (!fits) { hAd.resize(base); heA.resize(ebase); continue; }
        mwd_off[b] = (long long)base;
        he_off[b] = (int)ebase;
        c->mwd_blocks++;
    }
    if (c->mwd_blocks > 0) {
        std::vector<int> tasks;
        for (size_t di = 0; di < t.dn_list.size(); di++) {
            const int b = t.dn_list[di];
            if (mwd_off[b] < 0) continue;
            for (int e = 0; e < c->blk[b].cnt; e++) { tasks.push_back((int)di); tasks.push_back(e); }
        }
        c->mwd_tasks = (int)tasks.size() / 2;
        MW_RET(mw_upload(c, tasks, &c->mwd.tasks));
        MW_RET(mw_upload(c, hAd, &c->mwd.Ad)); MW_RET(mw_upload(c, heA, &c->mwd.eA)); MW_RET(mw_upload(c, he_off, &c->mwd.e_off));
        c->sm_mwd = (size_t)2 * S * sN * sizeof(float) + 128 * sizeof(int);
        MW_DISPATCH(c, { if constexpr (DD <= 2) { MW_RET(mw_set_lds((k_mwx_dense<KK, DD>), c->sm_mwd)); } });
    }
    return mw_upload(c, mwd_off, &c->mwd.a_off);
}

// ---- upload: the tables of mw_build_tables behind the pointers of MwDev ----
static int mw_stage_upload(clrs_mw_ctx *c, const MwTables &t) {
    MwDev &q = c->d;
    q.mws_off = c->mws.vs_off; q.mws_on = c->mws_blocks > 0 ? 1 : 0;
    q.mwx_off = c->mwx.d_off; q.mwx_on = c->mwx_blocks > 0 ? 1 : 0;
    q.mwd_off = c->mwd.a_off; q.mwd_on = 0;            // (switched on per assembly: the kernel needs the inverse factors of this context's chol X)
    q.J = t.J; q.N = t.N; q.NB = t.NB; q.nlr = (int)t.lr_list.size(); q.ndn = (int)t.dn_list.size();
    q.xylen = t.xylen; q.xlen = t.xlen; q.Slen = t.Slen; q.T = t.T; q.xrdlen = t.xrdlen;
    q.zlen = std::max<i64>(t.zlen, 1); q.glen = std::max<i64>(t.glen, 1); q.wlen = std::max<i64>(t.wlen, 1); q.sdlen = std::max<i64>(t.sdlen, 1);
    q.Vp = t.Vp; q.dAp = t.dAp; q.lamp = t.lamp; q.Bp = t.Bp;
    MW_RET(mw_upload(c, c->blk, &q.blk)); MW_RET(mw_upload(c, c->clu, &q.clu));
    MW_RET(mw_upload(c, t.lr_list, &q.lr_list)); MW_RET(mw_upload(c, t.dn_list, &q.dn_list));
    MW_RET(mw_upload(c, t.V, &q.V)); MW_RET(mw_upload(c, t.vrow, &q.vrow));
    MW_RET(mw_upload(c, t.st_a, &q.st_a)); MW_RET(mw_upload(c, t.st_b, &q.st_b)); MW_RET(mw_upload(c, t.st_lam, &q.st_lam));
    MW_RET(mw_upload(c, t.tptr, &q.tptr));
    MW_RET(mw_upload(c, t.st_orig, &q.st_orig)); MW_RET(mw_upload(c, t.st_p, &q.st_p)); MW_RET(mw_upload(c, t.st_war, &q.st_war)); MW_RET(mw_upload(c, t.st_wac, &q.st_wac));
    MW_RET(mw_upload(c, t.st_trl, &q.st_trl)); MW_RET(mw_upload(c, t.st_trd, &q.st_trd)); MW_RET(mw_upload(c, t.st_flag, &q.st_flag));
    MW_RET(mw_upload(c, t.ay_a, &q.ay_a)); MW_RET(mw_upload(c, t.ay_b, &q.ay_b)); MW_RET(mw_upload(c, t.ay_blk, &q.ay_blk));
    MW_RET(mw_upload(c, t.dA, &q.dA)); MW_RET(mw_upload(c, t.dmap, &q.dmap)); MW_RET(mw_upload(c, t.dense_p, &q.dense_p));
    MW_RET(mw_upload(c, t.drow_ptr, &q.drow_ptr)); MW_RET(mw_upload(c, t.drow_blk, &q.drow_blk)); MW_RET(mw_upload(c, t.drow_en, &q.drow_en));
    q.dn_big = t.dn_big;
    q.maxcnt = c->maxcnt;
    return mw_upload(c, t.B, &q.B);
}

static int mw_stage_buffers(clrs_mw_ctx *c) {
    MwDev &q = c->d;
    const int K = c->K, J = q.J, N = q.N;
    const i64 xlen = q.xlen, Slen = q.Slen, xyoff = q.xylen, rdoff = q.xrdlen, T = q.T;
    MW_RET(mw_dmalloc(c, &q.Z, q.zlen * K)); MW_RET(mw_dmalloc(c, &q.Tm, q.zlen * K));
    MW_RET(mw_dmalloc(c, &q.GX, q.glen * K)); MW_RET(mw_dmalloc(c, &q.GY, q.glen * K));
    MW_RET(mw_dmalloc(c, &q.W, q.wlen * K)); MW_RET(mw_dmalloc(c, &q.Sd, q.sdlen * K));
    MW_RET(mw_dmalloc(c, &q.S, Slen * K)); MW_RET(mw_dmalloc(c, &q.LB, xlen * (i64)N * K)); MW_RET(mw_dmalloc(c, &q.Q, (i64)N * N * K));
    MW_RET(mw_dmalloc(c, &q.Si, Slen * K)); MW_RET(mw_dmalloc(c, &q.Qi, (i64)N * N * K));

    MW_RET(mw_dmalloc(c, &q.Xf, xyoff * K)); MW_RET(mw_dmalloc(c, &q.Xb, xyoff * K)); MW_RET(mw_dmalloc(c, &q.Xi, xyoff * K));
    MW_RET(mw_dmalloc(c, &q.xrd, rdoff * K)); MW_RET(mw_dmalloc(c, &q.srd, xlen * K)); MW_RET(mw_dmalloc(c, &q.qrd, (i64)N * K));
    MW_RET(mw_dmalloc(c, &q.t, xlen * K)); MW_RET(mw_dmalloc(c, &q.u, (i64)J * N * K)); MW_RET(mw_dmalloc(c, &q.AY, T * K));
    q.AX = nullptr;                      // (the interior-point iteration asks for it: clrs_mw_ipm_create)
    q.aff_mu = q.aff_rhs = q.aff_t = q.aff_u = nullptr; q.aff_wait = nullptr; q.ride2_rhs = nullptr; q.ride2_t = q.ride2_u = nullptr;
    MW_RET(mw_dmalloc(c, &c->vz, 2 * (i64)N * K));
    MW_RET(mw_dmalloc(c, &q.S0, Slen * K)); MW_RET(mw_dmalloc(c, &q.ub, (i64)J * N * K));
    MW_RET(mw_dmalloc(c, &q.rx2, xlen * K)); MW_RET(mw_dmalloc(c, &q.dx2, xlen * K));
    MW_RET(mw_dmalloc(c, &q.u2, (i64)N * K)); MW_RET(mw_dmalloc(c, &q.dy2, (i64)N * K));
    q.uadd = nullptr;
    MW_RET(mw_dmalloc(c, &c->d_Xin, xyoff * K)); MW_RET(mw_dmalloc(c, &c->d_Xc, xyoff * K)); MW_RET(mw_dmalloc(c, &c->d_Y, xyoff * K));
    MW_RET(mw_dmalloc(c, &c->d_rx, xlen * K)); MW_RET(mw_dmalloc(c, &c->d_dx, xlen * K));
    MW_RET(mw_dmalloc(c, &c->d_ry, (i64)N * K)); MW_RET(mw_dmalloc(c, &c->d_dy, (i64)N * K));
    int *info = nullptr;
    MW_RET(mw_hip(hipMalloc((void **)&info, 2 * sizeof(int)), "hipMalloc"));
    c->allocs.push_back(info);
    q.info = info;
    int init[2] = {MW_INFO_NONE, MW_INFO_NONE};
    MW_RET(mw_hip(hipMemcpy(info, init, sizeof(init), hipMemcpyHostToDevice), "hipMemcpy"));
    return mw_alloc_fill(c, &q.pcnt, (size_t)(2 * J + 3), 0);
}

// matrices of the blocked path (k_mw_bp_*): the clusters beyond LDS, and Q
static int mw_stage_blocked(clrs_mw_ctx *c) {
    MwDev &q = c->d;
    const int K = c->K, J = q.J, N = q.N;
    for (int j = 0; j < J; j++) {
        const MwClu &cl = c->clu[j];
        if (cl.lds) { c->any_lds_cluster = true; continue; }
        c->bp_S.push_back(MwBp{q.S + cl.Soff, q.Si + cl.Soff, q.srd + cl.coff, q.Slen, q.xlen, cl.P, cl.P, j + 1, 0, (int)c->bp_S.size(), 0});
    }
    if (N > 0) c->bp_Q.push_back(MwBp{q.Q, q.Qi, q.qrd, (i64)N * N, (i64)N, N, N, J + 1, 0, (int)c->bp_S.size(), 0});
    std::vector<MwBp> all = c->bp_S;
    all.insert(all.end(), c->bp_Q.begin(), c->bp_Q.end());
    MW_RET(mw_upload(c, all, &c->d_bp));
    const int MW_PB = MW_PB_OF(K);
    c->sm_bp_diag = ((size_t)MW_POTRF_SCR(K, MW_PB) + (size_t)K * MW_PB * MW_PB + (size_t)K * MW_TRI(MW_PB) + (size_t)K * MW_PB) * 8;
    c->sm_bp_panel = (size_t)K * MW_BP_PR * MW_PB * 8;
    c->sm_bp_inv = (size_t)K * MW_PB * MW_BP_IC * 8;
    MW_DISPATCH(c, { MW_RET(mw_set_lds(k_mw_bp_diag<KK>, std::max(c->sm_bp_diag, c->sm_factor))); MW_RET(mw_set_lds(k_mw_bp_panel<KK>, c->sm_bp_panel)); MW_RET(mw_set_lds(k_mw_bp_inv<KK>, c->sm_bp_inv)); MW_RET(mw_set_lds(k_mw_bp_inv_row<KK>, c->sm_bp_inv)); });
    return 0;
}

// pipelined factorisations (clrs_mw_pipe.hip.h): matrices of at most 32 rows, while stages + W workgroups of every matrix can be resident side by side
static int mw_stage_pipelines(clrs_mw_ctx *c, const MwOpts &o) {
    MwDev &q = c->d;
    const int K = c->K, J = q.J, N = q.N, cfg_pipe = o.pipe;
    bool small = c->maxP <= MWP_N;
    for (auto &cl : c->clu) small = small && cl.lds;
    c->pipe_S = cfg_pipe != 0 && (K <= 6 || cfg_pipe >= 2) && small && (i64)J * ((MWP_N / MWP_W) + MWP_WW) <= 256;      // (8, 10 limbs: measured slower than one workgroup, 2.42 against 2.34 ms per iteration: opt-in)
    // (Q: with the columns asked for four steps ahead the pipeline was slower than the one-workgroup kernel on the named problem, 83 against 80 us; with
    // MWP_AHEAD = 0 it is faster -- whole iterations 0.4197 -> 0.4165 ms on cohnelkies(8,15), 0.4113 -> 0.4057 on delsarte(3,10,1/2): on from two stages,
    // and with pipeline = 2 for every Q of at most MWP_N rows)
    c->pipe_Q = (cfg_pipe >= 2 || (cfg_pipe == 1 && K <= 6 && N > MWP_W)) && N > 0 && N <= MWP_N;
    bool lds_all = !c->clu.empty();
    for (auto &cl : c->clu) lds_all = lds_all && cl.lds;
    // (measured at 5 limbs, factor stage in 4: PolyOpt 2d = 40, P = 41 -- six stages, five hops -- 0.478 -> 0.487 ms per iteration; the tested three-point instance,
    // P = 50, 0.648 -> 0.638: by default from 48 rows on, with pipeline = 2 for every cluster of 33 .. 64 rows)
    c->pipe_S64 = cfg_pipe != 0 && K <= 6 && lds_all && c->maxP > MWP_N && c->maxP <= MWP_N64 && (i64)J * 16 <= 256 && g_cfg_mw_pipeline64 != 0 &&
                  (cfg_pipe >= 2 || c->maxP >= 48);
    // the diagonal blocks of the blocked factorisation (k_mw_bp_diag_pipe): the same pipeline per 32-column block of every matrix beyond LDS
    const size_t nbp = c->bp_S.size() + c->bp_Q.size();
    const bool any_bp = !c->bp_S.empty() || (N > 0 && !c->lds_q);
    // (at every limb count: 8 and 10 limbs gain 2-4 % per iteration as well -- scripts/blocked_pipe_limbs.py -- unlike the clusters that fit in LDS)
    c->pipe_bp = cfg_pipe != 0 && any_bp && (i64)std::max<size_t>(c->bp_S.size(), 1) * ((MWP_N / MWP_W) + MWP_WW) <= 256;
    q.pipe_pc = nullptr;
    q.pipe_stamps = nullptr;
    q.pipe_bp = 0;
    {   // the Cholesky of the X blocks through the pipelines: every block carries its inverse factor in LDS form (inv == 1) and has at most 64 rows
        // (measured at 5 limbs, whole iterations: blocks of 32 and 48 rows -- Nsphere_packing N = 2 1.146 -> 1.122 ms, N = 3 2.059 -> 2.027; blocks of at most 21 rows:
        // nothing either way; 64 blocks of 32 rows -- 2 x 64 x 8 working workgroups for 256 compute units -- 1.69 -> 1.87: by default from 24 rows of the largest
        // block on and while every working workgroup of the launch has a compute unit of its own)
        bool all_inv = c->d.NB > 0 && c->lds_x;
        int maxn_x = 0;
        i64 working = 0;
        for (auto &kb : c->blk) {
            all_inv = all_inv && kb.inv == 1;
            maxn_x = std::max(maxn_x, kb.n);
            working += 2 * ((kb.n + MWP_W - 1) / MWP_W + (kb.n > MWP_N ? MWP_N64 / MWP_W : MWP_WW));
        }
        // no reader of the scaled triangles Xf / Xb in such a context (k_mw_zt and k_mw_dense_t take the products with Xi, k_mwi_Z is not launched, k_mwi_step
        // takes an inverse-factor path: clrs_mw_ipm_create_ex clears this where it would not) unless a dense block of more than one row substitutes for want of
        // LDS; callers' own factors (k_mw_xrd) come with triangles of their own
        q.no_xfb = (all_inv && (!q.dn_big || c->dense_two) && g_cfg_mw_skip_xfb != 0) ? 1 : 0;
        c->pipe_X = cfg_pipe != 0 && K <= 6 && all_inv && maxn_x <= MWP_N64 && g_cfg_mw_pipeline_x != 0 &&
                    (cfg_pipe >= 2 || (maxn_x >= g_cfg_mw_pipeline_x_min && working <= 256));
        if (c->pipe_X) {
            double *pcx = nullptr, *ti = nullptr;
            MW_RET(mw_dmalloc(c, &pcx, (i64)2 * c->d.NB * MWP_PC_WORDS_N(K, MWP_N64)));
            c->pipe_pcx = (unsigned long long *)pcx;
            MW_RET(mw_dmalloc(c, &c->xpipe_L, c->d.xylen * K));
            MW_RET(mw_dmalloc(c, &c->xpipe_rd, c->d.xrdlen * K));
            MW_RET(mw_dmalloc(c, &ti, c->d.NB + 1));
            c->xpipe_info = (int *)ti;
            MW_DISPATCH(c, { if constexpr (KK <= 6) { MW_RET(mw_set_lds(k_mw_potrf_x_pipe<KK>, MWP_LDS_ALONE64)); } });
        }
    }
    if (c->pipe_S64) {                                    // (its own hand-off region: 64-row columns; no other pipeline runs in such a context's factor stage but Q's / the blocked path's below)
        MW_RET(mw_alloc_fill(c, &c->pipe_pc64, (size_t)J * MWP_PC_WORDS_N(K, MWP_N64), 0xff));
        MW_DISPATCH(c, { if constexpr (KK <= 6) { MW_RET(mw_set_lds(k_mw_factor_pipe64<KK>, MWP_LDS_ALONE64)); } });
    }
    if (c->pipe_S || c->pipe_Q || c->pipe_bp) {
        const size_t own = (size_t)(c->pipe_S ? J : 0) + 1;
        MW_RET(mw_alloc_fill(c, &q.pipe_pc, (own + (c->pipe_bp ? nbp : 0)) * MWP_PC_WORDS(K), 0xff));      // no launch epoch has this tag
        c->pipe_pcQ = c->pipe_S ? J : 0;
        q.pipe_q = c->pipe_pcQ;
        q.pipe_bp = (int)own;
        MW_DISPATCH(c, {
            MW_RET(mw_set_lds(k_mw_factor_pipe<KK>, MWP_LDS_ALONE));
            MW_RET(mw_set_lds(k_mw_potrf_q_pipe<KK>, std::max<size_t>(MWP_LDS_ALONE, c->sm_fwd)));
            MW_RET(mw_set_lds(k_mw_bp_diag_pipe<KK>, std::max<size_t>(MWP_LDS_ALONE, c->sm_factor)));
        });
    }
    return 0;
}

// factor stage and solve products in fewer limbs, residuals and iterate in K (mw_kf_of): the LDS-resident paths with the full-limb refinement step
static int mw_stage_reduced_limbs(clrs_mw_ctx *c, const MwOpts &o) {
    MwDev &q = c->d;
    const int K = c->K, N = q.N;
    q.rank = 0; q.world = 1; q.gathered = 0;      // (the gather slots of a sharded context, allocated at this point of the sequence)
    MW_RET(mw_dmalloc(c, &q.Qg, (i64)N * N * K)); MW_RET(mw_dmalloc(c, &q.ug, (i64)N * K));
    const bool may = mw_kf_of(K) < K && c->refine == 1;      // (every factorisation and solve path carries the reduced form: LDS-resident, pipelined, blocked, row-parallel)
    c->kf_low = may ? mw_kf_of(K) : K;
    if (o.factor_limbs != 0 && o.factor_limbs != K && o.factor_limbs != c->kf_low) return mw_fail(CLRS_ERR_INVALID, "factor_limbs: 0 (automatic), the context's limbs, or the reduced count of this limb count where the LDS-resident refined solve runs");
    if (o.factor_limbs == K) c->kf_low = K;
    c->kf_entry = o.factor_limbs == 0 ? K : o.factor_limbs;
    q.kf = c->kf_entry;
    q.km = o.km;
    return mw_alloc_fill(c, &q.refstat, 4, 0);
}

extern "C" int clrs_mw_create_opts(const clrs_sdp_desc *d, int data_limbs, int device, int limbs, const clrs_mw_options *opts, clrs_mw_ctx **out) {
    if (!d || !out) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MwOpts o;
    MW_RET(mw_resolve_opts(opts, limbs, data_limbs, o));
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) return mw_fail(CLRS_ERR_NO_DEVICE, "no usable HIP device");
    MW_RET(mw_hip(hipSetDevice(device), "hipSetDevice(device)"));
    if (d->n_clusters <= 0 || d->n_free < 0 || d->n_blocks < 0) return mw_fail(CLRS_ERR_INVALID, "bad sizes");      // (before the stream, as ever; mw_build_tables says the same)
    std::unique_ptr<clrs_mw_ctx, void (*)(clrs_mw_ctx *)> guard(new clrs_mw_ctx(), clrs_mw_destroy);      // the one cleanup path of every failure below
    clrs_mw_ctx *c = guard.get();
    c->device = device;
    c->K = limbs;
    c->DK = data_limbs;
    c->refine = o.refine;
    c->refine_predictor = o.refine_pred;
    {
        const char *e = std::getenv("CLRS_MW_STREAM_WORDS");
        c->stream_words = e && *e ? std::atoi(e) != 0 : g_cfg_mw_stream_words != 0;
        c->chain_hop = std::min(std::max(g_cfg_mw_chain_hop, 0), 2);
        c->y_riders = g_cfg_mw_y_riders != 0;
        c->zi_narrow = g_cfg_mw_zi_narrow != 0;
        c->xinv_product = g_cfg_mw_xinv_product != 0;
    }
    MW_RET(mw_stage_stream(c));
    MwTables t;
    std::string err;
    if (mw_build_tables(d, data_limbs, t, err)) return mw_fail(CLRS_ERR_INVALID, err);
    mw_adopt_tables(c, t);
    MW_RET(mw_stage_lds(c, t));
    std::vector<long long> mws_off;
    MW_RET(mw_stage_mws(c, t, o, mws_off));
    MW_RET(mw_stage_mwx(c, t, o, mws_off));
    MW_RET(mw_stage_mwd(c, t, o));
    MW_RET(mw_stage_upload(c, t));
    MW_RET(mw_stage_buffers(c));
    MW_RET(mw_stage_blocked(c));
    MW_RET(mw_stage_pipelines(c, o));
    MW_RET(mw_stage_reduced_limbs(c, o));
    for (auto &e : c->ev) MW_RET(mw_hip(hipEventCreate(&e), "hipEventCreate(&e)"));
    *out = guard.release();
    return 0;
}
#undef MW_RET

extern "C" void clrs_mw_destroy(clrs_mw_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    mw_ipm_free(c);
    if (c->comm && g_nccl.CommDestroy) { (void)g_nccl.CommDestroy(c->comm); c->comm = nullptr; }
    if (c->comm_side && g_nccl.CommDestroy) { (void)g_nccl.CommDestroy(c->comm_side); c->comm_side = nullptr; }
    if (c->lgroup) { std::lock_guard<std::mutex> lk(c->lgroup->m); c->lgroup->attached--; c->lgroup = nullptr; }
    for (void *p : c->allocs) (void)hipFree(p);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->h_info) (void)hipHostFree(c->h_info);
    if (c->stream && c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int clrs_mw_limbs(const clrs_mw_ctx *c) { return c ? c->K : 0; }
extern "C" void *clrs_mw_stream(clrs_mw_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int clrs_mw_set_stream(clrs_mw_ctx *c, void *stream) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
    return 0;
}
extern "C" int clrs_mw_get_dims(const clrs_mw_ctx *c, clrs_dims *o) {
    if (!c || !o) return mw_fail(CLRS_ERR_INVALID, "null argument");
    o->xy_len = c->d.xylen; o->x_len = c->d.xlen; o->S_len = c->d.Slen; o->n_terms = c->d.T;
    o->n_free = c->d.N; o->n_clusters = c->d.J; o->n_blocks = c->d.NB; o->reserved = c->K;
    return 0;
}
extern "C" int clrs_mw_get_unique_count(const clrs_mw_ctx *c, int32_t block, int32_t *n_unique) {
    if (!c || !n_unique || block < 0 || block >= c->d.NB) return mw_fail(CLRS_ERR_INVALID, "bad argument");
    *n_unique = c->blk[block].U;
    return 0;
}
extern "C" int clrs_mw_set_timing(clrs_mw_ctx *c, int on) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    c->timing = on != 0;
    return 0;
}
extern "C" int clrs_mw_get_counters(const clrs_mw_ctx *c, double *assemble_muladds, double *factor_muladds, double *solve_muladds) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (assemble_muladds) *assemble_muladds = c->cnt_mul;
    if (factor_muladds) *factor_muladds = c->cnt_factor;
    if (solve_muladds) *solve_muladds = c->cnt_solve;
    return 0;
}

// the assembly's small form of k_mw_zt (two columns per workgroup, eight lanes per entry), once the inverse factors of this context's Cholesky exist
static bool mw_zt_small(const clrs_mw_ctx *c) { return c->all_inv && (i64)c->d.nlr * c->maxU <= 2048 && c->maxn <= g_cfg_mw_zt_small_maxn; }
// ... and, in such a context, whether the Y half of the pairings can ride on the Cholesky launch of the X blocks: no block goes through the exact-product
// kernels (they read T as a whole), one context holds the whole problem, the Cholesky is the one-workgroup kernel
static bool mw_y_riders_ok(const clrs_mw_ctx *c) {
    return c->y_riders && mw_zt_small(c) && c->d.nlr > 0 && c->mws_blocks == 0 && c->mwx_blocks == 0 && !c->pipe_X && !c->d.gathered && c->d.world <= 1;
}
static int mw_reset_info(clrs_mw_ctx *c, int which) {
    if (c->ipm_arms_info) return 0;
    MWCHECK(hipMemsetAsync(c->d.info + which, 0x7f, sizeof(int), c->stream));      // MW_INFO_NONE is the byte 0x7f four times
    return 0;
}
static int mw_read_info(clrs_mw_ctx *c, int which, int *status) {
    MWCHECK(hipMemcpyAsync(c->h_info + which, c->d.info + which, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MWCHECK(hipStreamSynchronize(c->stream));
    *status = c->h_info[which] == MW_INFO_NONE ? 0 : c->h_info[which];
    return 0;
}

// ---- the path, device pointers (planar K x len arrays), enqueue only ------------------------------------------------
// d_Y2 (optional): a second block-diagonal matrix whose inverse Cholesky factors go to d_Yi, failures per block to d_yfail
static int mw_cholesky_blocks_dev2(clrs_mw_ctx *c, const double *d_X, double *d_Xchol, const double *d_Y2, double *d_Yi, int *d_yfail) {
    if (!c || !d_X || !d_Xchol) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    int rc;
    if ((rc = mw_reset_info(c, 1))) return rc;
    if (c->d.NB == 0) return 0;
    const int grid = d_Y2 ? 2 * c->d.NB : c->d.NB;
    bool in_mem = false;                                  // some block forms its inverse factor in memory, or in LDS beside a large block: four workgroups share its columns
    for (auto &k : c->blk) in_mem = in_mem || k.inv == 2 || mw_x_shares(k);
    if (c->pipe_X) {
        c->pipe_epoch = (c->pipe_epoch + 1) & 0x3ffffff;
        MW_DISPATCH(c, { if constexpr (KK <= 6) { hipLaunchKernelGGL(k_mw_potrf_x_pipe<KK>, dim3(mwp_blocks64(grid)), dim3(MWP_NT64), MWP_LDS_ALONE64, c->stream, c->d, d_X, d_Xchol, d_Y2, d_Yi, d_yfail,
                                                                     c->xpipe_L, c->xpipe_rd, c->xpipe_info, c->pipe_pcx, c->pipe_epoch); } });
    } else if (c->ride_y && mw_y_riders_ok(c)) {           // (low-rank block, two unique vectors) tasks behind the factorisations: T = Y V and GY = V^T T of the assembly that follows
        const int ntile = (c->maxU + 1) / 2;
        MW_DISPATCH(c, hipLaunchKernelGGL((k_mw_potrf_x_ride<KK, DD>), dim3(grid + c->d.nlr * ntile, in_mem && c->lds_x ? MW_INV_WG : 1), dim3(MW_PT), c->sm_x, c->stream, c->d, d_X, d_Xchol,
                                          c->lds_x ? 1 : 0, d_Y2, d_Yi, d_yfail, c->ride_y, grid, ntile));
    } else
    MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_potrf_x<KK>, dim3(grid, in_mem && c->lds_x ? MW_INV_WG : 1), dim3(MW_PT), c->sm_x, c->stream, c->d, d_X, d_Xchol, c->lds_x ? 1 : 0, d_Y2, d_Yi, d_yfail));
    MWCHECK(hipGetLastError());
    c->xinv_valid = true;
    return 0;
}
extern "C" int clrs_mw_cholesky_blocks_dev(clrs_mw_ctx *c, const double *d_X, double *d_Xchol) { return mw_cholesky_blocks_dev2(c, d_X, d_Xchol, nullptr, nullptr, nullptr); }
extern "C" int clrs_mw_sync_status_cholesky(clrs_mw_ctx *c) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    int st = 0, rc;
    if ((rc = mw_read_info(c, 1, &st))) return rc;
    return st;
}

extern "C" int clrs_mw_schur_assemble_dev(clrs_mw_ctx *c, const double *d_Xchol, const double *d_Y) {
    if (!c || !d_Xchol || !d_Y) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    if (c->timing) MWCHECK(hipEventRecord(c->ev[0], c->stream));
    MW_DISPATCH(c, {
        const bool exact = c->mws_blocks > 0 && c->xinv_valid;      // the exact-product kernel needs chol(X)^-1 (k_mw_potrf_x of this context)
        bool dense_done = exact && q.ndn && !q.dn_big;          // 1 x 1 dense blocks ride on the launch of the exact pairing matrices ...
        const int pair_grid = q.nlr + (dense_done ? q.ndn : 0);
        if constexpr (DD <= 2) {                             // (data at the working precision: the exact slice products are off, clrs_mw_create_opts)
            if (exact && c->mws_turns == 1) hipLaunchKernelGGL((k_mws_pair<KK, DD, 1>), dim3(pair_grid), dim3(MWS_NT), c->sm_mws, c->stream, q, c->mws, d_Y);
            else if (exact) hipLaunchKernelGGL((k_mws_pair<KK, DD, 2>), dim3(pair_grid), dim3(MWS_NT), c->sm_mws, c->stream, q, c->mws, d_Y);
        }
        if (q.nlr && !(exact && c->mws_blocks == q.nlr)) {
            MwDev q2 = q;
            q2.mws_on = exact ? 1 : 0;
            const int gper = MW_NT / MW_GRAM_W;
            // few blocks, every one with its inverse factor: two columns per workgroup and eight lanes per entry
            const int zt_ct = (c->xinv_valid && mw_zt_small(c)) ? 2 : MW_CT;
            hipLaunchKernelGGL((k_mw_zt<KK, DD>), dim3((c->maxU + zt_ct - 1) / zt_ct, q.nlr), dim3(MW_NT), c->sm_zt, c->stream, q2, d_Y, c->lds_zt_L ? 1 : 0, c->xinv_valid ? 1 : 0, zt_ct);
            const bool ride_gram = !dense_done && q.ndn && !q.dn_big;      // ... or on that of the expansion kernel
            dense_done = dense_done || ride_gram;
            q2.mwx_on = c->mwx_blocks > 0 ? 1 : 0;
            hipLaunchKernelGGL((k_mw_gram<KK, DD>), dim3((c->maxU * (c->maxU + 1) / 2 + gper - 1) / gper, q.nlr + (ride_gram ? q.ndn : 0)), dim3(MW_NT), 0, c->stream, q2, d_Y);
            if (q2.mwx_on) {                                 // the large pairing matrices: digits of Z and T, then 16 x 16 tiles on the matrix cores
                const int nt = c->mwx_maxU16 / 16;
                hipLaunchKernelGGL(k_mwx_slice<KK>, dim3(nt, 2, q.nlr), dim3(MWS_NT), 0, c->stream, q2, c->mwx);
                hipLaunchKernelGGL(k_mwx_gram<KK>, dim3((nt * (nt + 1) / 2 + MWS_NT / 64 - 1) / (MWS_NT / 64), 2, q.nlr), dim3(MWS_NT), 0, c->stream, q2, c->mwx);
            }
        }
        if (q.ndn && !dense_done) {
            const bool panels = c->xinv_valid && c->maxn_dense > 16 && c->maxn_dense <= MW_NT;      // dense blocks of side > 16 with inverse factors: column panels (k_mw_dense_tp)
            MwDev q3 = q;
            q3.mwd_on = (panels && c->mwd_blocks > 0) ? 1 : 0;     // ... or exact slice products for sides up to 32 (k_mwx_dense)
            hipLaunchKernelGGL((k_mw_dense_t<KK, DD>), dim3(q.ndn, q.dn_big ? c->maxcnt : 1), dim3(MW_NT), c->sm_dense, c->stream, q3, d_Y, c->xinv_valid ? 1 : 0, c->dense_two ? 1 : 0, panels ? 1 : 0);
            if (panels) {
                const int pcmin = std::max(1, MW_NT / c->maxn_dense);
                if (c->mwd_blocks < q.ndn)
                    hipLaunchKernelGGL((k_mw_dense_tp<KK, DD>), dim3(q.ndn, c->maxcnt, (c->maxn_dense + pcmin - 1) / pcmin), dim3(MW_NT), (size_t)2 * KK * MW_NT * 8, c->stream, q3, d_Y);
                c->mwd.stamps = c->mws.stamps;
                if constexpr (DD <= 2) { if (q3.mwd_on) hipLaunchKernelGGL((k_mwx_dense<KK, DD>), dim3(c->mwd_tasks), dim3(MWS_NT), c->sm_mwd, c->stream, q3, c->mwd, d_Y); }
            }
            const int pairs = c->maxcnt * (c->maxcnt + 1) / 2;
            const int ds_lanes = c->maxn_dense * c->maxn_dense <= 128 ? 8 : c->maxn_dense * c->maxn_dense <= 512 ? 16 : 64;      // per pair of the table
            if (q.dn_big) hipLaunchKernelGGL((k_mw_dense_s<KK, DD>), dim3(q.ndn, (pairs + MW_NT / ds_lanes - 1) / (MW_NT / ds_lanes)), dim3(MW_NT), 0, c->stream, q, ds_lanes);
        }
        // (the per-term pairings A_Y are written by k_mw_saccum, or by k_mw_saccum_one cluster by cluster when no cluster is left to k_mw_saccum)
        if (c->n_many_term) hipLaunchKernelGGL((k_mw_saccum<KK, DD>), dim3((c->maxP * (c->maxP + 1) / 2 * c->sa_lanes + MW_NT - 1) / MW_NT, q.J), dim3(MW_NT), 0, c->stream, q, c->sa_lanes);
        if (c->n_one_term) hipLaunchKernelGGL((k_mw_saccum_one<KK, DD>), dim3((c->maxP * (c->maxP + 1) / 2 + MW_NT - 1) / MW_NT, q.J), dim3(MW_NT), 0, c->stream, q, c->n_many_term ? 0 : 1);
    });
    MWCHECK(hipGetLastError());
    if (c->timing) MWCHECK(hipEventRecord(c->ev[1], c->stream));
    c->assembled = true;
    c->factored = false;
    c->local_factored = false;
    return 0;
}

// ---- cluster sharding: split-phase entry points and the RCCL exchange ---------------------------------------------------

extern "C" int clrs_comm_unique_id(void *id128) {
    if (!id128) return mw_fail(CLRS_ERR_INVALID, "null argument");
    int rc = mw_nccl_load();
    if (rc) return rc;
    NCCLCHECK(g_nccl.GetUniqueId((mw_nccl_id *)id128));
    return 0;
}

// This context holds the clusters of rank `rank` of `world` (the description it was created from lists only those clusters, with
// all N free variables).  world = 1 restores the unsharded behaviour.
extern "C" int clrs_mw_set_shard(clrs_mw_ctx *c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return mw_fail(CLRS_ERR_INVALID, "bad rank / world");
    MWCHECK(hipSetDevice(c->device));
    MWCHECK(hipStreamSynchronize(c->stream));
    MwDev &q = c->d;
    if (world != q.world) {
        int rc;
        if ((rc = mw_dmalloc(c, &q.Qg, (i64)world * q.N * q.N * c->K))) return rc;       // (the previous buffers stay in `allocs` until destroy)
        if ((rc = mw_dmalloc(c, &q.ug, (i64)world * q.N * c->K))) return rc;
    }
    q.rank = rank; q.world = world;
    q.gathered = (world > 1 || c->comm || c->lgroup) ? 1 : 0;
    return 0;
}
// The library performs the two exchanges itself with RCCL all-gathers on the context stream (one of limbs*N*N doubles per
// factorisation, one of limbs*N per solve): clrs_mw_schur_factor_dev / _solve_dev then are collective calls.
extern "C" int clrs_mw_comm_init(clrs_mw_ctx *c, const void *id128, int rank, int world) {
    if (!c || !id128) return mw_fail(CLRS_ERR_INVALID, "null argument");
    int rc = mw_nccl_load();
    if (rc) return rc;
    if ((rc = clrs_mw_set_shard(c, rank, world))) return rc;
    mw_nccl_id id;
    std::memcpy(&id, id128, sizeof(id));
    NCCLCHECK(g_nccl.CommInitRank(&c->comm, world, id, rank));
    c->d.gathered = 1;
    return 0;
}
extern "C" int clrs_mw_comm_destroy(clrs_mw_ctx *c) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (c->comm) {
        (void)hipStreamSynchronize(c->stream);
        NCCLCHECK(g_nccl.CommDestroy(c->comm));
        c->comm = nullptr;
        if (c->comm_side) { NCCLCHECK(g_nccl.CommDestroy(c->comm_side)); c->comm_side = nullptr; }
    }
    if (c->lgroup) {                                     // detach from the in-process group (which counts its attached ranks)
        (void)hipStreamSynchronize(c->stream);
        std::lock_guard<std::mutex> lk(c->lgroup->m);
        c->lgroup->attached--;
        c->lgroup = nullptr;
    }
    c->d.gathered = c->d.world > 1 ? 1 : 0;
    return 0;
}
extern "C" double *clrs_mw_q_gather_dev(clrs_mw_ctx *c) { return c ? c->d.Qg : nullptr; }
extern "C" double *clrs_mw_u_gather_dev(clrs_mw_ctx *c) { return c ? c->d.ug : nullptr; }

// all-gather of `cnt` doubles per rank inside `base` ([world][cnt], this rank's slot written by earlier work on `stream`); channel 0 =
// the context's stream, 1 = the side stream of the interior-point iteration
static bool mw_has_comm(const clrs_mw_ctx *c, int chan) { return c->lgroup || (chan == 0 ? c->comm : c->comm_side); }
static int mw_allgather(clrs_mw_ctx *c, int chan, double *base, size_t cnt, hipStream_t stream) {
    const MwDev &q = c->d;
    if (c->lgroup) {
        clrs_mw_local_group *g = c->lgroup;
        auto &ch = g->ch[chan];
        const int r = q.rank;
        MWCHECK(hipEventRecord(ch.ready[r], stream));
        ch.base[r] = base;
        g->barrier(chan);
        for (int p = 0; p < g->world; p++) {
            if (p == r) continue;
            MWCHECK(hipStreamWaitEvent(stream, ch.ready[p], 0));
            MWCHECK(hipMemcpyAsync(base + (size_t)p * cnt, ch.base[p] + (size_t)p * cnt, cnt * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
        MWCHECK(hipEventRecord(ch.copied[r], stream));
        g->barrier(chan);
        for (int p = 0; p < g->world; p++)
            if (p != r) MWCHECK(hipStreamWaitEvent(stream, ch.copied[p], 0));
        return 0;
    }
    void *comm = chan == 0 ? c->comm : c->comm_side;
    if (!comm) return mw_fail(CLRS_ERR_STATE, chan == 0 ? "sharded context without a communicator: use the split-phase entry points or clrs_mw_comm_init"
                                                        : "the sharded interior-point iteration needs the side communicator: clrs_mw_comm_init_side");
    NCCLCHECK(g_nccl.AllGather(base + (size_t)q.rank * cnt, base, cnt, MW_NCCL_FLOAT64, comm, stream));
    return 0;
}
// Diagnostic for the multi-GPU bench: the cost of the exchanges of one sharded interior-point iteration on this context's communicator, measured with
// HIP events on the context's stream around `reps` all-gathers of each size, back to back: us[0] the partial Q (limbs N^2 doubles per rank), us[1] the
// partial u (limbs N), us[2] a scalar record (MWG_LEN).  Collective: every rank of the communicator must call it.  info[0..2] = rank, world, backend
// (0 none, 1 RCCL, 2 in-process group).
extern "C" int clrs_mw_comm_probe(clrs_mw_ctx *c, int reps, double us[3], int info[3]) {
    if (!c || !us || !info || reps < 1) return mw_fail(CLRS_ERR_INVALID, "bad argument");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    info[0] = q.rank; info[1] = q.world; info[2] = c->comm ? 1 : c->lgroup ? 2 : 0;
    us[0] = us[1] = us[2] = 0.0;
    if (!mw_has_comm(c, 0) || q.N <= 0) return 0;
    const size_t cnt[3] = {(size_t)q.N * q.N * c->K, (size_t)q.N * c->K, (size_t)MWG_LEN(c->K, q.N)};      // (the record as the iteration exchanges it: clrs_mw_ipm.hip.h)
    double *scratch = nullptr;                                       // (a buffer of its own: the exchanges must not disturb Qg / ug)
    MWCHECK(hipMalloc((void **)&scratch, cnt[0] * q.world * sizeof(double)));
    MWCHECK(hipMemsetAsync(scratch, 0, cnt[0] * q.world * sizeof(double), c->stream));
    hipEvent_t e0, e1;
    MWCHECK(hipEventCreate(&e0)); MWCHECK(hipEventCreate(&e1));
    int rc = 0;
    for (int k = 0; k < 3 && !rc; k++) {
        for (int w = 0; w < 3 && !rc; w++) rc = mw_allgather(c, 0, scratch, cnt[k], c->stream);          // warm-up
        if (rc) break;
        (void)hipEventRecord(e0, c->stream);
        for (int i = 0; i < reps && !rc; i++) rc = mw_allgather(c, 0, scratch, cnt[k], c->stream);
        (void)hipEventRecord(e1, c->stream);
        if (hipEventSynchronize(e1) != hipSuccess) rc = mw_fail(CLRS_ERR_HIP, "hipEventSynchronize failed");
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        us[k] = 1e3 * ms / reps;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(scratch);
    return rc;
}
// second RCCL communicator (its own unique id), for the exchanges the interior-point iteration issues on its side stream
extern "C" int clrs_mw_comm_init_side(clrs_mw_ctx *c, const void *id128) {
    if (!c || !id128) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (!c->comm) return mw_fail(CLRS_ERR_STATE, "clrs_mw_comm_init first");
    mw_nccl_id id;
    std::memcpy(&id, id128, sizeof(id));
    NCCLCHECK(g_nccl.CommInitRank(&c->comm_side, c->d.world, id, c->d.rank));
    return 0;
}
extern "C" int clrs_mw_local_group_create(int world, int device, clrs_mw_local_group **out) {
    if (!out || world < 1) return mw_fail(CLRS_ERR_INVALID, "bad argument");
    MWCHECK(hipSetDevice(device));
    clrs_mw_local_group *g = new clrs_mw_local_group();
    g->world = world;
    for (auto &ch : g->ch) {
        ch.base.assign(world, nullptr);
        ch.ready.assign(world, nullptr);
        ch.copied.assign(world, nullptr);
        for (int r = 0; r < world; r++) {
            MWCHECK(hipEventCreateWithFlags(&ch.ready[r], hipEventDisableTiming));
            MWCHECK(hipEventCreateWithFlags(&ch.copied[r], hipEventDisableTiming));
            // recorded once on the null stream, so that a wait issued before the first real record of a peer is well defined
            MWCHECK(hipEventRecord(ch.ready[r], nullptr));
            MWCHECK(hipEventRecord(ch.copied[r], nullptr));
        }
    }
    MWCHECK(hipDeviceSynchronize());
    *out = g;
    return 0;
}
// (refused -- the group is leaked and the last error set -- while contexts are attached: they would dereference freed events in their next exchange;
// clrs_mw_comm_destroy or clrs_mw_destroy on each rank first)
extern "C" void clrs_mw_local_group_destroy(clrs_mw_local_group *g) {
    if (!g) return;
    {
        std::lock_guard<std::mutex> lk(g->m);
        if (g->attached > 0) { (void)mw_fail(CLRS_ERR_STATE, "clrs_mw_local_group_destroy: contexts are still attached (clrs_mw_comm_destroy them first)"); return; }
    }
    for (auto &ch : g->ch) {
        for (auto e : ch.ready) if (e) (void)hipEventDestroy(e);
        for (auto e : ch.copied) if (e) (void)hipEventDestroy(e);
    }
    delete g;
}
// this context is rank `rank` of the in-process group: the library's exchanges then go through it (one host thread per rank)
extern "C" int clrs_mw_comm_init_local(clrs_mw_ctx *c, clrs_mw_local_group *g, int rank) {
    if (!c || !g) return mw_fail(CLRS_ERR_INVALID, "null argument");
    int rc = clrs_mw_set_shard(c, rank, g->world);
    if (rc) return rc;
    if (c->lgroup != g) {
        if (c->lgroup) { std::lock_guard<std::mutex> lk(c->lgroup->m); c->lgroup->attached--; }
        std::lock_guard<std::mutex> lk(g->m);
        g->attached++;
    }
    c->lgroup = g;
    c->d.gathered = 1;
    return 0;
}

// blocked Cholesky and inverse factor of matrices in global memory over many workgroups (clrs_mw_kernels.hip.h, k_mw_bp_*): all matrices of the
// list side by side in every launch (their block columns are chains of five launches each: the clusters of Nsphere_packing with N = 3 wait
// for nothing but their own).  ride_factor: the first launch also carries the clusters that fit in LDS (k_mw_factor's work).
static int mw_potrf_blocked(clrs_mw_ctx *c, const std::vector<MwBp> &hm, const MwBp *d_ms, bool ride_factor) {
    const MwDev &q = c->d;
    const int MW_PB = MW_PB_OF(c->K), nm = (int)hm.size();
    int nmax = 0;
    for (auto &m : hm) nmax = std::max(nmax, m.n);
    const int nbk = (nmax + MW_PB - 1) / MW_PB;
    MW_DISPATCH(c, {
        for (int j0 = 0; j0 < nmax; j0 += MW_PB) {
            const int nb = std::min(MW_PB, nmax - j0), mm = nmax - j0 - nb;
            const bool ride = ride_factor && j0 == 0;
            if (c->pipe_bp) {
                // block row j0 / MW_PB - 1 of the inverse factors rides on this launch (its diagonal block was the previous launch's)
                const int inv_row = j0 / MW_PB - 1 >= 1 ? j0 / MW_PB - 1 : 0;
                c->pipe_epoch = (c->pipe_epoch + 1) & 0x3ffffff;
                hipLaunchKernelGGL(k_mw_bp_diag_pipe<KK>, dim3(mwp_blocks(nm) + (ride ? q.J * MW_INV_WG : 0) + inv_row * (MW_PB / MW_BP_IC) * nm), dim3(MWP_NT),
                                   ride ? std::max<size_t>(MWP_LDS_ALONE, c->sm_factor) : std::max<size_t>(MWP_LDS_ALONE, c->sm_bp_inv),
                                   c->stream, q, d_ms, nm, j0, c->pipe_epoch, ride ? q.J : 0, inv_row);
            } else
            hipLaunchKernelGGL(k_mw_bp_diag<KK>, dim3(MW_INV_WG, nm + (ride ? q.J : 0)), dim3(MW_PT), ride ? std::max(c->sm_bp_diag, c->sm_factor) : c->sm_bp_diag, c->stream, q, d_ms, nm, j0);
            if (mm > 0) {
                hipLaunchKernelGGL(k_mw_bp_panel<KK>, dim3((mm + MW_BP_PR - 1) / MW_BP_PR, nm), dim3(MW_PT), c->sm_bp_panel, c->stream, q, d_ms, j0);
                hipLaunchKernelGGL(k_mw_bp_syrk<KK>, dim3((unsigned)(((i64)mm * (mm + 1) / 2 * MW_BP_SW + MW_NT - 1) / MW_NT), nm), dim3(MW_NT), 0, c->stream, q, d_ms, j0);
            }
        }
        if (c->pipe_bp) {                // the rows 1 .. nbk - 2 rode on the launches of the diagonal blocks; the last row has none to ride on
            if (nbk >= 2) hipLaunchKernelGGL(k_mw_bp_inv_row<KK>, dim3(nbk - 1, MW_PB / MW_BP_IC, nm), dim3(MW_PT), c->sm_bp_inv, c->stream, q, d_ms, nbk - 1);
        } else
        for (int d = 1; d < nbk; d++)
            hipLaunchKernelGGL(k_mw_bp_inv<KK>, dim3(nbk - d, MW_PB / MW_BP_IC, nm), dim3(MW_PT), c->sm_bp_inv, c->stream, q, d_ms, d);
        hipLaunchKernelGGL(k_mw_bp_finish<KK>, dim3((unsigned)std::min<i64>(1024, ((i64)nmax * nmax + MW_NT - 1) / MW_NT), nm), dim3(MW_NT), 0, c->stream, q, d_ms);
    });
    MWCHECK(hipGetLastError());
    return 0;
}

// L_j, LinvB_j of this rank's clusters and its partial Q into slot `rank` of the gather buffer
extern "C" int clrs_mw_schur_factor_local_dev(clrs_mw_ctx *c) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (!c->assembled) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_factor before clrs_mw_schur_assemble");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    int rc;
    if ((rc = mw_reset_info(c, 0))) return rc;
    if (c->timing) MWCHECK(hipEventRecord(c->ev[2], c->stream));
    // clusters that do not fit in LDS: blocked over many workgroups, all of them side by side; the others ride on the first of those launches
    // when they take the same number of workgroups per matrix, else they have their launch (k_mw_factor)
    const bool ride = !c->bp_S.empty() && c->nw_factor == MW_INV_WG && c->any_lds_cluster;
    if (c->pipe_S64) {
        c->pipe_epoch = (c->pipe_epoch + 1) & 0x3ffffff;
        MwDev q64 = q;
        q64.pipe_pc = c->pipe_pc64;
        MW_DISPATCH(c, { if constexpr (KK <= 6) { hipLaunchKernelGGL(k_mw_factor_pipe64<KK>, dim3(mwp_blocks64(q.J)), dim3(MWP_NT64), MWP_LDS_ALONE64, c->stream, q64, c->pipe_epoch); } });
    } else if (c->pipe_S) {
        c->pipe_epoch = (c->pipe_epoch + 1) & 0x3ffffff;
        MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_factor_pipe<KK>, dim3(mwp_blocks(q.J)), dim3(MWP_NT), MWP_LDS_ALONE, c->stream, q, c->pipe_epoch); });
    } else if (!ride && c->any_lds_cluster) MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_factor<KK>, dim3(q.J, c->nw_factor), dim3(MW_PT), c->sm_factor, c->stream, q); });
    if (!c->bp_S.empty()) MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_keep_S<KK>, dim3((unsigned)std::min<i64>(64, ((i64)c->maxP * c->maxP + MW_NT - 1) / MW_NT), q.J), dim3(MW_NT), 0, c->stream, q));
    if (!c->bp_S.empty() && (rc = mw_potrf_blocked(c, c->bp_S, c->d_bp, ride))) return rc;
    MW_DISPATCH(c, {
        if (q.N > 0)
            hipLaunchKernelGGL((k_mw_linvb<KK, DD>), dim3((c->maxP * q.N + MW_NT / MW_LBI_W - 1) / (MW_NT / MW_LBI_W), q.J), dim3(MW_NT), 0, c->stream, q);
        if (c->timing) (void)hipEventRecord(c->ev[3], c->stream);
        const int qw = (i64)q.N * (q.N + 1) / 2 * 32 <= 32768 && q.xlen >= 32 ? 32 : MW_Q_W;      // lanes per entry of Q
        if (q.N > 0) hipLaunchKernelGGL(k_mw_qgram<KK>, dim3((q.N * (q.N + 1) / 2 + MW_NT / qw - 1) / (MW_NT / qw)), dim3(MW_NT), 0, c->stream, q, qw);
        if (c->timing) (void)hipEventRecord(c->ev[4], c->stream);
    });
    MWCHECK(hipGetLastError());
    c->local_factored = true;
    c->factored = false;
    c->assembled = false;                       // S now holds L_j: a second factorisation needs a new assembly (as the fp64 entry point)
    return 0;
}
// after the gather buffer holds every rank's partial Q: Q = their sum, Cholesky of Q (redundantly on every rank)
extern "C" int clrs_mw_schur_factor_finish_dev(clrs_mw_ctx *c) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (!c->local_factored) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_factor_finish before clrs_mw_schur_factor_local");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    if (q.N > 0 && c->pipe_Q) {
        const bool ride = c->ride_fwd != nullptr && !c->wide_solve;
        c->pipe_epoch = (c->pipe_epoch + 1) & 0x3ffffff;
        MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_potrf_q_pipe<KK>, dim3(64 + (ride ? q.J * (q.ride2_rhs ? 2 : 1) : 0)), dim3(MWP_NT), std::max<size_t>(MWP_LDS_ALONE, ride ? c->sm_fwd : 0),
                                            c->stream, q, c->pipe_epoch, c->ride_fwd, ride ? c->ride_wait : (const int *)nullptr, c->ride_wait_value); });
        c->fwd_rode = ride;
    } else if (q.N > 0 && c->lds_q) {
        // the interior-point iteration hands over the right-hand side of its next solve: the solve's first product pair rides on this launch
        const bool ride = c->ride_fwd != nullptr && !c->wide_solve;
        MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_potrf_q<KK>, dim3(MW_INV_WG + (ride ? q.J * (q.ride2_rhs ? 2 : 1) : 0)), dim3(MW_PT), ride ? std::max(c->sm_q, c->sm_fwd) : c->sm_q, c->stream, q, MW_INV_WG, c->ride_fwd, ride ? c->ride_wait : (const int *)nullptr, c->ride_wait_value); });
        c->fwd_rode = ride;
    } else if (q.N > 0) {
        MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_qsum<KK>, dim3((unsigned)std::min<i64>(256, ((i64)q.N * q.N + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, c->stream, q); });
        int rc = mw_potrf_blocked(c, c->bp_Q, c->d_bp + c->bp_S.size(), false);
        if (rc) return rc;
    }
    MWCHECK(hipGetLastError());
    if (c->timing) MWCHECK(hipEventRecord(c->ev[5], c->stream));
    c->factored = true;
    return 0;
}
extern "C" int clrs_mw_schur_factor_dev(clrs_mw_ctx *c) {
    int rc = clrs_mw_schur_factor_local_dev(c);
    if (rc) return rc;
    const MwDev &q = c->d;
    if (q.gathered && q.N > 0) {
        int rc2 = mw_allgather(c, 0, q.Qg, (size_t)q.N * q.N * c->K, c->stream);
        if (rc2) return rc2;
    }
    return clrs_mw_schur_factor_finish_dev(c);
}
extern "C" int clrs_mw_sync_status(clrs_mw_ctx *c) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    int st = 0, rc;
    if ((rc = mw_read_info(c, 0, &st))) return rc;
    return st;
}

// t_j = L_j^-1 rhs_x[j] and this rank's partial u (slot `rank` of the u gather buffer when sharded)
extern "C" int clrs_mw_schur_solve_fwd_dev(clrs_mw_ctx *c, const double *d_rhs_x) {
    if (!c || !d_rhs_x) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (!c->local_factored) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_solve before clrs_mw_schur_factor");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    if (c->timing) MWCHECK(hipEventRecord(c->ev[6], c->stream));
    MW_DISPATCH(c, {
        hipLaunchKernelGGL(k_mw_solve_fwd<KK>, dim3(q.J), dim3(MW_NT), c->sm_fwd, c->stream, q, d_rhs_x);
        if (q.gathered && q.N > 0) hipLaunchKernelGGL(k_mw_usum<KK>, dim3(1), dim3(MW_NT), 0, c->stream, q);
    });
    MWCHECK(hipGetLastError());
    c->fwd_done = true;
    c->split_rhs_x = d_rhs_x;
    return 0;
}
// the backward half: dy = Q^-1 (rhs_y - sum u), dx_j = L_j^-T (t_j + LinvB_j dy).  mode 0: plain; 1: followed by the first half of the refinement step
// (residuals, t', u' into q.t, q.ub); 2: the correction's backward half, added to dx, dy (k_mw_solve_bwd).  full_kc: the correction in all K limbs.
#define MW_BWD(KCC, MODE) hipLaunchKernelGGL((k_mw_solve_bwd<KK, KCC, DD, MODE>), dim3(q.J), dim3(MW_NT), lds, c->stream, q, (const double *)dy_mid, d_dx, mid, d_dy, d_rhs_x)
static int mw_solve_bwd(clrs_mw_ctx *c, const MwDev &q, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy, int mode, bool full_kc) {
    if (c->sm_mid + c->sm_bwd > MW_LDS_MAX) return mw_fail(CLRS_ERR_INVALID, "system too large for the one-workgroup-per-cluster solve kernels (a sharded solve with clusters + free variables beyond LDS)");
    const size_t lds = c->sm_mid + c->sm_bwd;
    MW_DISPATCH(c, {
        constexpr int KC = mw_kc(KK);
        // few clusters, one rank: dy is formed by every workgroup of the backward launch itself (one launch less on the chain of the iteration)
        const bool mid_in_bwd = q.N > 0 && !q.gathered && q.J <= 4;
        double *dy_mid = mode == 2 ? q.dy2 : d_dy;          // (the correction dy' has a buffer of its own; the backward launch adds it)
        if (q.N > 0 && !mid_in_bwd) {
            if (mode == 2 && !full_kc) hipLaunchKernelGGL((k_mw_solve_mid<KK, KC>), dim3(1), dim3(MW_NT), c->sm_mid, c->stream, q, d_rhs_y, dy_mid);
            else hipLaunchKernelGGL((k_mw_solve_mid<KK, KK>), dim3(1), dim3(MW_NT), c->sm_mid, c->stream, q, d_rhs_y, dy_mid);
        }
        const double *mid = mid_in_bwd ? d_rhs_y : (const double *)nullptr;
        if (mode == 0) MW_BWD(KK, 0);
        else if (mode == 1) { if (full_kc) MW_BWD(KK, 1); else MW_BWD(KC, 1); }
        else { if (full_kc) MW_BWD(KK, 2); else MW_BWD(KC, 2); }
    });
#undef MW_BWD
    MWCHECK(hipGetLastError());
    return 0;
}
extern "C" int clrs_mw_schur_solve_bwd_dev(clrs_mw_ctx *c, const double *d_rhs_y, double *d_dx, double *d_dy) {
    if (!c || !d_dx) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored || !c->fwd_done) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_solve_bwd before clrs_mw_schur_factor_finish / clrs_mw_schur_solve_fwd");
    const MwDev &q = c->d;
    if (q.N > 0 && (!d_rhs_y || !d_dy)) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    // split-phase callers with the refinement on: the launch also forms the residuals and the forward half of the correction, and leaves this rank's
    // partial u' in its gather slot -- after one more exchange of the u slots clrs_mw_schur_solve_refine_dev adds the correction (optional: without
    // that call (dx, dy) are the plain products' solution)
    const bool first_half = c->refine && c->split_rhs_x != nullptr;
    int rc = mw_solve_bwd(c, q, c->split_rhs_x, d_rhs_y, d_dx, d_dy, first_half ? 1 : 0, c->refine != 2);
    if (rc) return rc;
    if (first_half && q.gathered && q.N > 0) {
        MwDev q2 = q;
        q2.u = q.ub;
        MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_usum<KK>, dim3(1), dim3(MW_NT), 0, c->stream, q2));
        MWCHECK(hipGetLastError());
    }
    c->refine_ready = first_half;
    c->split_rhs_x = nullptr;
    if (c->timing) MWCHECK(hipEventRecord(c->ev[7], c->stream));
    c->fwd_done = false;
    return 0;
}
// second half of the refinement step for split-phase callers: after clrs_mw_schur_solve_bwd_dev and one more exchange of the u gather slots
extern "C" int clrs_mw_schur_solve_refine_dev(clrs_mw_ctx *c, const double *d_rhs_y, double *d_dx, double *d_dy) {
    if (!c || !d_dx) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (!c->refine) return 0;                             // clrs_config_set("mw_refine", 0): nothing to add
    if (!c->refine_ready) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_solve_refine before clrs_mw_schur_solve_fwd / clrs_mw_schur_solve_bwd");
    const MwDev &q = c->d;
    if (q.N > 0 && (!d_rhs_y || !d_dy)) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    MwDev q2 = q;
    q2.u = q.ub;
    c->refine_ready = false;
    return mw_solve_bwd(c, q2, nullptr, d_rhs_y, d_dx, d_dy, 2, c->refine != 2);
}

// one pass of the row-parallel solve (clusters or a Q beyond 64 rows, one rank): a launch per product
static int mw_solve_wide_once(clrs_mw_ctx *c, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy) {
    const MwDev &q = c->d;
    constexpr int RPW = MW_NT / MW_SW_L;
    const dim3 gP((c->maxP + RPW - 1) / RPW, q.J), gN((q.N + RPW - 1) / RPW), gX((unsigned)((q.xlen + RPW - 1) / RPW));
    MW_DISPATCH(c, {
        hipLaunchKernelGGL(k_mw_solve_wide<KK>, gP, dim3(MW_NT), 0, c->stream, q, 1, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
        if (q.N > 0) {
            hipLaunchKernelGGL(k_mw_solve_wide<KK>, gN, dim3(MW_NT), 0, c->stream, q, 2, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
            hipLaunchKernelGGL(k_mw_solve_wide<KK>, gN, dim3(MW_NT), 0, c->stream, q, 3, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
            hipLaunchKernelGGL(k_mw_solve_wide<KK>, gN, dim3(MW_NT), 0, c->stream, q, 4, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
            hipLaunchKernelGGL(k_mw_solve_wide<KK>, gX, dim3(MW_NT), 0, c->stream, q, 5, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
        }
        hipLaunchKernelGGL(k_mw_solve_wide<KK>, gP, dim3(MW_NT), 0, c->stream, q, 6, d_rhs_x, d_rhs_y, d_dx, d_dy, c->vz);
    });
    MWCHECK(hipGetLastError());
    return 0;
}
// The solve stage (src/solver.jl:1527-1582): one pass of products with the inverse factors, then (c->refine, the default) one step of iterative
// refinement against the assembled S_j and B (k_mw_refine's header): the backward error of the reference's substitutions at the latency of products.
extern "C" int clrs_mw_schur_solve_dev(clrs_mw_ctx *c, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy) {
    if (!c || !d_rhs_x || !d_dx) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored) return mw_fail(CLRS_ERR_STATE, "clrs_mw_schur_solve before clrs_mw_schur_factor");
    MwDev &q = c->d;
    if (q.N > 0 && (!d_rhs_y || !d_dy)) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    int rc = 0;
    const int refine = c->refine_skip_next ? 0 : c->refine;
    c->refine_skip_next = false;
    if (c->wide_solve && !q.gathered) {                  // large clusters or a large Q: one launch per product, rows over many workgroups
        if (c->timing) MWCHECK(hipEventRecord(c->ev[6], c->stream));
        if ((rc = mw_solve_wide_once(c, d_rhs_x, d_rhs_y, d_dx, d_dy))) return rc;
        if (refine) {
            constexpr int RPW = MW_NT / MW_SW_L;
            const int rowsP = (c->maxP + RPW - 1) / RPW, rowsN = (q.N + RPW - 1) / RPW;
            MW_DISPATCH(c, hipLaunchKernelGGL((k_mw_refine<KK, DD>), dim3(std::max(rowsP, rowsN), q.J + (q.N > 0 ? 1 : 0)), dim3(MW_NT), 0, c->stream, q, 1, d_rhs_x, d_dx, d_dy));
            MWCHECK(hipGetLastError());
            q.uadd = q.N > 0 ? q.u2 : nullptr;
            rc = mw_solve_wide_once(c, q.rx2, d_rhs_y, q.dx2, q.dy2);
            q.uadd = nullptr;
            if (rc) return rc;
            MW_DISPATCH(c, hipLaunchKernelGGL((k_mw_refine<KK, DD>), dim3((unsigned)std::min<i64>(256, (q.xlen + q.N + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, c->stream, q, 3, d_rhs_x, d_dx, d_dy));
            MWCHECK(hipGetLastError());
        }
        if (c->timing) MWCHECK(hipEventRecord(c->ev[7], c->stream));
        return 0;
    }
    // one workgroup per cluster: forward half (unless it rode on an earlier launch), [exchange of the partial u], backward half; the refinement's
    // residuals and forward half ride on the backward launch, its backward half is one more launch [and one more exchange]
    if (c->fwd_rode) {                                   // t_j, u_j of this right-hand side are there already (k_mw_potrf_q's launch, or k_mwi_rows_fwd)
        c->fwd_rode = false;
        c->fwd_done = true;
        if (q.gathered && q.N > 0) {                     // sharded: this rank's partial u into its gather slot, as clrs_mw_schur_solve_fwd_dev does behind its launch
            MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_usum<KK>, dim3(1), dim3(MW_NT), 0, c->stream, q));
            MWCHECK(hipGetLastError());
        }
    } else rc = clrs_mw_schur_solve_fwd_dev(c, d_rhs_x);
    if (rc) return rc;
    if (q.gathered && q.N > 0 && (rc = mw_allgather(c, 0, q.ug, (size_t)q.N * c->K, c->stream))) return rc;
    c->split_rhs_x = nullptr;
    if (!refine) { const int keep = c->refine; c->refine = 0; rc = clrs_mw_schur_solve_bwd_dev(c, d_rhs_y, d_dx, d_dy); c->refine = keep; return rc; }
    const bool full_kc = refine != 2;                  // 2: the correction in mw_kc(K) limbs (opt-in: valid while twice the lost bits fit in them)
    if ((rc = mw_solve_bwd(c, q, d_rhs_x, d_rhs_y, d_dx, d_dy, 1, full_kc))) return rc;
    MwDev q2 = q;
    q2.u = q.ub;                                         // (the first half of the step wrote its u' beside the u the other workgroups were still reading)
    if (q.gathered && q.N > 0) {
        MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_usum<KK>, dim3(1), dim3(MW_NT), 0, c->stream, q2));
        MWCHECK(hipGetLastError());
        if ((rc = mw_allgather(c, 0, q.ug, (size_t)q.N * c->K, c->stream))) return rc;
    }
    if ((rc = mw_solve_bwd(c, q2, d_rhs_x, d_rhs_y, d_dx, d_dy, 2, full_kc))) return rc;
    if (c->timing) MWCHECK(hipEventRecord(c->ev[7], c->stream));
    c->fwd_done = false;
    return 0;
}

extern "C" double *clrs_mw_S_buffer_dev(clrs_mw_ctx *c) { return c ? c->d.S : nullptr; }
extern "C" double *clrs_mw_AY_buffer_dev(clrs_mw_ctx *c) { return c ? c->d.AY : nullptr; }

// S_j (S layout) and the per-term pairings A_Y of the last assembly, planar limbs, to host memory (either pointer may be NULL): for
// callers of the device-pointer entry points (clrs_mw_schur_assemble_dev) that want to look at what was assembled
extern "C" int clrs_mw_get_S(clrs_mw_ctx *c, double *S_out, double *AY_out) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (!c->assembled) return mw_fail(CLRS_ERR_STATE, "clrs_mw_get_S before clrs_mw_schur_assemble (or after the factorisation has overwritten S)");
    MWCHECK(hipSetDevice(c->device));
    MWCHECK(hipStreamSynchronize(c->stream));
    if (S_out) MWCHECK(hipMemcpy(S_out, c->d.S, (size_t)c->d.Slen * c->K * sizeof(double), hipMemcpyDeviceToHost));
    if (AY_out && c->d.T) MWCHECK(hipMemcpy(AY_out, c->d.AY, (size_t)c->d.T * c->K * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// diagnostic (-DCLRS_MW_STAMPS builds): step stamps of the pipelined factorisations, [16 roles][40]: rows 0-7 the workgroups of cluster 0 in
// k_mw_factor_pipe, rows 8-15 those of Q in k_mw_potrf_q_pipe; columns 0..n-1 the top of step k, 39 start, 38 end (100 MHz wall clock); behind them
// [8 roles][32 steps][4 who][4 points]: the stamps inside the steps of cluster 0 (clrs_mw_pipe.hip.h; scripts/pipe_substamps.py)
extern "C" int clrs_mw_debug_pipe_stamps(clrs_mw_ctx *c, unsigned long long *out) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
#ifndef CLRS_MW_STAMPS
    return mw_fail(CLRS_ERR_STATE, "this library was built without -DCLRS_MW_STAMPS");
#endif
    MWCHECK(hipSetDevice(c->device));
    MWCHECK(hipStreamSynchronize(c->stream));
    if (!c->d.pipe_stamps) {
        double *p = nullptr;
        int rc = mw_dmalloc(c, &p, 16 * 40 + 8 * 32 * 4 * 4);
        if (rc) return rc;
        c->d.pipe_stamps = (unsigned long long *)p;
    } else if (out) MWCHECK(hipMemcpy(out, c->d.pipe_stamps, (16 * 40 + 8 * 32 * 4 * 4) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
// diagnostic: phase stamps (100 MHz wall clock) of wave 0 of the first workgroup of the next k_mws_pair launches; out[16] = the last ones
extern "C" int clrs_mw_debug_exact_stamps(clrs_mw_ctx *c, unsigned long long *out) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
#ifndef CLRS_MW_STAMPS
    return mw_fail(CLRS_ERR_STATE, "this library was built without -DCLRS_MW_STAMPS (the product kernels carry no phase stamps): CLRS_MW_STAMPS=1 builds the diagnostic variant");
#endif
    MWCHECK(hipSetDevice(c->device));
    MWCHECK(hipStreamSynchronize(c->stream));
    if (!c->mws.stamps) {
        double *p = nullptr;
        int rc = mw_dmalloc(c, &p, 16);
        if (rc) return rc;
        c->mws.stamps = (unsigned long long *)p;
    } else if (out) MWCHECK(hipMemcpy(out, c->mws.stamps, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int clrs_mw_get_timings(clrs_mw_ctx *c, double t[6]) {
    if (!c || !t) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipStreamSynchronize(c->stream));
    if (c->timing) {
        float ms = 0;
        const int pairs[6][2] = {{0, 1}, {2, 3}, {3, 3}, {3, 4}, {4, 5}, {6, 7}};      // schur, cholS + LinvB (one kernel), -, Q, cholQ, solve
        for (int i = 0; i < 6; i++) {
            if (pairs[i][0] == pairs[i][1]) { c->times[i] = 0; continue; }
            if (hipEventElapsedTime(&ms, c->ev[pairs[i][0]], c->ev[pairs[i][1]]) == hipSuccess) c->times[i] = ms * 1e-3;
        }
    }
    for (int i = 0; i < 6; i++) t[i] = c->times[i];
    return 0;
}

// ---- host-pointer entry points (planar K x len host arrays; copy, run, synchronise) ----------------------------------
extern "C" int clrs_mw_cholesky_blocks(clrs_mw_ctx *c, const double *X, double *Xchol) {
    if (!c || !X || !Xchol) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->d.xylen * c->K * sizeof(double);
    MWCHECK(hipMemcpyAsync(c->d_Xin, X, bytes, hipMemcpyHostToDevice, c->stream));
    int rc = clrs_mw_cholesky_blocks_dev(c, c->d_Xin, c->d_Xc);
    if (rc) return rc;
    MWCHECK(hipMemcpyAsync(Xchol, c->d_Xc, bytes, hipMemcpyDeviceToHost, c->stream));
    return clrs_mw_sync_status_cholesky(c);
}
extern "C" int clrs_mw_schur_assemble(clrs_mw_ctx *c, const double *Xchol, const double *Y, double *S_out, double *AY_out) {
    if (!c || !Xchol || !Y) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->d.xylen * c->K * sizeof(double);
    MWCHECK(hipMemcpyAsync(c->d_Xc, Xchol, bytes, hipMemcpyHostToDevice, c->stream));
    MWCHECK(hipMemcpyAsync(c->d_Y, Y, bytes, hipMemcpyHostToDevice, c->stream));
    // the substitutions need the reciprocal diagonal of chol(X): recomputed from the factor the caller passes
    int rc;
    if ((rc = mw_launch_xrd(c, c->d_Xc))) return rc;
    if ((rc = clrs_mw_schur_assemble_dev(c, c->d_Xc, c->d_Y))) return rc;
    if (S_out) MWCHECK(hipMemcpyAsync(S_out, c->d.S, (size_t)c->d.Slen * c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (AY_out && c->d.T) MWCHECK(hipMemcpyAsync(AY_out, c->d.AY, (size_t)c->d.T * c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int clrs_mw_schur_factor(clrs_mw_ctx *c) {
    int rc = clrs_mw_schur_factor_dev(c);
    if (rc) return rc;
    return clrs_mw_sync_status(c);
}
extern "C" int clrs_mw_get_factor(clrs_mw_ctx *c, double *L, double *LinvB, double *LQ) {
    if (!c) return mw_fail(CLRS_ERR_INVALID, "null context");
    if (!c->factored) return mw_fail(CLRS_ERR_STATE, "clrs_mw_get_factor before clrs_mw_schur_factor");
    MWCHECK(hipSetDevice(c->device));
    MWCHECK(hipStreamSynchronize(c->stream));
    const MwDev &q = c->d;
    const int K = c->K, N = q.N;
    if (L) MWCHECK(hipMemcpy(L, q.S, (size_t)q.Slen * K * sizeof(double), hipMemcpyDeviceToHost));
    if (LQ && N) MWCHECK(hipMemcpy(LQ, q.Q, (size_t)N * N * K * sizeof(double), hipMemcpyDeviceToHost));
    if (LinvB && N) {
        // device: stacked xlen x N; caller: per cluster P_j x N column-major, concatenated (as clrs_get_factor)
        std::vector<double> h((size_t)q.xlen * N * K);
        MWCHECK(hipMemcpy(h.data(), q.LB, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        const i64 plane = q.xlen * (i64)N;
        for (int l = 0; l < K; l++) {
            i64 off = 0;
            for (int j = 0; j < q.J; j++) {
                const int P = c->clu[j].P;
                for (int a = 0; a < N; a++)
                    for (int r = 0; r < P; r++) LinvB[l * plane + off + r + (i64)a * P] = h[l * plane + c->clu[j].coff + r + (i64)a * q.xlen];
                off += (i64)P * N;
            }
        }
    }
    return 0;
}
extern "C" int clrs_mw_schur_solve(clrs_mw_ctx *c, const double *rhs_x, const double *rhs_y, double *dx, double *dy) {
    if (!c || !rhs_x || !dx) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    const MwDev &q = c->d;
    const int K = c->K;
    MWCHECK(hipMemcpyAsync(c->d_rx, rhs_x, (size_t)q.xlen * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (q.N) {
        if (!rhs_y || !dy) return mw_fail(CLRS_ERR_INVALID, "null argument");
        MWCHECK(hipMemcpyAsync(c->d_ry, rhs_y, (size_t)q.N * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    int rc = clrs_mw_schur_solve_dev(c, c->d_rx, c->d_ry, c->d_dx, c->d_dy);
    if (rc) return rc;
    MWCHECK(hipMemcpyAsync(dx, c->d_dx, (size_t)q.xlen * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (q.N) MWCHECK(hipMemcpyAsync(dy, c->d_dy, (size_t)q.N * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

static int mw_launch_xrd(clrs_mw_ctx *c, const double *d_Xc) {
    if (c->d.NB == 0) return 0;
    MW_DISPATCH(c, hipLaunchKernelGGL(k_mw_xrd<KK>, dim3(c->d.NB), dim3(MW_NT), 0, c->stream, c->d, d_Xc));
    MWCHECK(hipGetLastError());
    c->xinv_valid = false;                  // the caller's factors: no inverse beside them, the assembly substitutes
    return 0;
}
// device-pointer form of the same (callers that bring their own Cholesky factors of X)
extern "C" int clrs_mw_set_xchol_dev(clrs_mw_ctx *c, const double *d_Xchol) {
    if (!c || !d_Xchol) return mw_fail(CLRS_ERR_INVALID, "null argument");
    MWCHECK(hipSetDevice(c->device));
    return mw_launch_xrd(c, d_Xchol);
}

// ---- linear dependencies of the constraints (the reference's preprocess!, src/pre_postprocessing.jl) ----------------------------

// X = Y = I in the xy layout (limb plane 0; the caller has cleared the planes): grid = blocks
static __global__ void k_mw_fill_identity(const MwDev q, double *__restrict__ Xc, double *__restrict__ Y) {
    const MwBlk &k = q.blk[blockIdx.x];
    for (int i = threadIdx.x; i < k.n; i += blockDim.x) {
        Xc[k.xyoff + i + (i64)i * k.n] = 1.0;
        Y[k.xyoff + i + (i64)i * k.n] = 1.0;
    }
}
// LB := B (the data's DK limb planes, the upper K - DK planes zero): grid-stride over the xlen x N entries
static __global__ void k_mw_b_to_lb(const MwDev q, int K, int DK) {
    const i64 plane = q.xlen * (i64)q.N;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < plane; e += (i64)gridDim.x * blockDim.x)
        for (int l = 0; l < K; l++) q.LB[l * plane + e] = l < DK ? q.B[l * q.Bp + e] : 0.0;
}

// G_j = S_j(X = I, Y = I) into the context's S buffer, by the context's own assembly kernels: entry (p, q) is sum_l <A_p, A_q>, the Gram matrix of
// the cluster's constraint matrices.  Uses the staging buffers of the host-pointer entry points only.
static int mw_constraint_gram_dev(clrs_mw_ctx *c) {
    MWCHECK(hipSetDevice(c->device));
    const size_t bytes = (size_t)std::max<i64>(c->d.xylen, 1) * c->K * sizeof(double);
    MWCHECK(hipMemsetAsync(c->d_Xc, 0, bytes, c->stream));
    MWCHECK(hipMemsetAsync(c->d_Y, 0, bytes, c->stream));
    if (c->d.NB) hipLaunchKernelGGL(k_mw_fill_identity, dim3(c->d.NB), dim3(MW_NT), 0, c->stream, c->d, c->d_Xc, c->d_Y);
    MWCHECK(hipGetLastError());
    int rc;
    if ((rc = mw_launch_xrd(c, c->d_Xc))) return rc;          // chol(I) = I with reciprocal diagonal 1: the assembly substitutes with unit factors
    return clrs_mw_schur_assemble_dev(c, c->d_Xc, c->d_Y);
}
extern "C" int clrs_mw_constraint_gram(clrs_mw_ctx *c, double *G_out) {
    if (!c || !G_out) return mw_fail(CLRS_ERR_INVALID, "null argument");
    int rc = mw_constraint_gram_dev(c);
    if (rc) return rc;
    MWCHECK(hipMemcpyAsync(G_out, c->d.S, (size_t)c->d.Slen * c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MWCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
// B^T B = sum_j B_j^T B_j (N x N, planar): the Q-Gram kernel of the factor stage applied to B itself (LinvB := B)
extern "C" int clrs_mw_free_gram(clrs_mw_ctx *c, double *Q_out) {
    if (!c || !Q_out) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (c->d.world > 1) return mw_fail(CLRS_ERR_STATE, "clrs_mw_free_gram on a sharded context");
    MWCHECK(hipSetDevice(c->device));
    MwDev q = c->d;
    if (q.N == 0) return 0;
    q.kf = c->K;                                             // all limbs, whatever the factor stage runs in
    const i64 plane = q.xlen * (i64)q.N;
    hipLaunchKernelGGL(k_mw_b_to_lb, dim3((unsigned)std::min<i64>(1024, (plane + MW_NT - 1) / MW_NT)), dim3(MW_NT), 0, c->stream, q, c->K, c->DK);
    MW_DISPATCH(c, { hipLaunchKernelGGL(k_mw_qgram<KK>, dim3((q.N * (q.N + 1) / 2 + MW_NT / MW_Q_W - 1) / (MW_NT / MW_Q_W)), dim3(MW_NT), 0, c->stream, q, MW_Q_W); });
    MWCHECK(hipGetLastError());
    MWCHECK(hipMemcpyAsync(Q_out, q.Qg + (i64)q.rank * c->K * q.N * q.N, (size_t)q.N * q.N * c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MWCHECK(hipStreamSynchronize(c->stream));
    c->factored = c->local_factored = false;                 // LB and the partial Q no longer belong to a factorisation
    return 0;
}

// One launch of k_mw_rank_reveal over `mats` (host list; lds flags and the LDS size are set here).  d_G: the matrices (overwritten where a matrix is not
// LDS-resident), d_Wk: workspace of the same shape, d_W / d_perm / d_rank / d_resid: outputs on the device.
static int mw_rank_launch(int K, hipStream_t stream, std::vector<MwRankMat> &mats, double *d_G, double *d_Wk, i64 gplane, double *d_W, int *d_perm, int *d_rank,
                          double *d_resid, i64 xplane) {
    size_t lds = 0;
    for (auto &m : mats) {
        if (m.n < 0 || m.ncand < 0 || m.ncand > m.n) return mw_fail(CLRS_ERR_INVALID, "rank reveal: need 0 <= ncand <= n");
        const size_t full = (size_t)MW_RANK_LDS(K, m.n);
        m.lds = full <= MW_LDS_MAX ? 1 : 0;
        lds = std::max(lds, m.lds ? full : (size_t)MW_RANK_SCR(K, m.n) * 8);
    }
    if (lds > MW_LDS_MAX) return mw_fail(CLRS_ERR_INVALID, "rank reveal: matrix too large (the pivots' scale factors and the permutation must fit in LDS)");
    if (mats.empty()) return 0;
    MwRankMat *d_m = nullptr;
    MWCHECK(hipMalloc((void **)&d_m, mats.size() * sizeof(MwRankMat)));
    hipError_t e = hipMemcpyAsync(d_m, mats.data(), mats.size() * sizeof(MwRankMat), hipMemcpyHostToDevice, stream);
#define MW_RANK_CASE(Kc)                                                                                                                            \
    case Kc:                                                                                                                                        \
        if (e == hipSuccess && lds > 48 * 1024) e = hipFuncSetAttribute((const void *)k_mw_rank_reveal<Kc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e == hipSuccess) hipLaunchKernelGGL(k_mw_rank_reveal<Kc>, dim3((unsigned)mats.size()), dim3(MW_PT), lds, stream, d_m, d_G, d_Wk, gplane, d_W, d_perm, d_rank, d_resid, xplane); \
        break;
    switch (K) {
        MW_RANK_CASE(4) MW_RANK_CASE(5) MW_RANK_CASE(6) MW_RANK_CASE(8) MW_RANK_CASE(10)
        default: (void)hipFree(d_m); return mw_fail(CLRS_ERR_INVALID, "rank reveal: limbs must be 4, 5, 6, 8 or 10");
    }
#undef MW_RANK_CASE
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_m);
    if (e != hipSuccess) return mw_fail(CLRS_ERR_HIP, std::string("rank reveal: ") + hipGetErrorString(e));
    return 0;
}

// device buffers of one call, released on every path
struct MwRankBufs {
    std::vector<void *> p;
    ~MwRankBufs() { for (void *x : p) (void)hipFree(x); }
    template <class T>
    hipError_t get(T **d, size_t count) {
        hipError_t e = hipMalloc((void **)d, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*d);
        return e;
    }
};

extern "C" int clrs_mw_rank_reveal(int device, int limbs, int nmat, const int32_t *n, const int32_t *ncand, const double *G, const double *tau, int32_t *perm,
                                   int32_t *rank, double *W, double *resid) {
    if (nmat < 0 || (nmat > 0 && (!n || !ncand || !G || !tau || !perm || !rank || !W || !resid))) return mw_fail(CLRS_ERR_INVALID, "null argument");
    if (nmat == 0) return 0;
    MWCHECK(hipSetDevice(device));
    std::vector<MwRankMat> mats(nmat);
    i64 gplane = 0, xplane = 0;
    for (int m = 0; m < nmat; m++) {
        if (n[m] < 0) return mw_fail(CLRS_ERR_INVALID, "rank reveal: negative size");
        mats[m] = MwRankMat{n[m], ncand[m], 0, 0, gplane, xplane, tau[m]};
        gplane += (i64)n[m] * n[m];
        xplane += n[m];
    }
    MwRankBufs bufs;
    double *d_G = nullptr, *d_Wk = nullptr, *d_W = nullptr, *d_resid = nullptr;
    int *d_perm = nullptr, *d_rank = nullptr;
    const size_t gb = (size_t)gplane * limbs, xb = (size_t)xplane * limbs;
    MWCHECK(bufs.get(&d_G, gb)); MWCHECK(bufs.get(&d_Wk, gb)); MWCHECK(bufs.get(&d_W, gb)); MWCHECK(bufs.get(&d_resid, xb));
    MWCHECK(bufs.get(&d_perm, (size_t)xplane)); MWCHECK(bufs.get(&d_rank, (size_t)nmat));
    MWCHECK(hipMemcpy(d_G, G, gb * sizeof(double), hipMemcpyHostToDevice));
    MWCHECK(hipMemset(d_W, 0, std::max<size_t>(gb, 1) * sizeof(double)));
    MWCHECK(hipMemset(d_resid, 0, std::max<size_t>(xb, 1) * sizeof(double)));
    int rc = mw_rank_launch(limbs, nullptr, mats, d_G, d_Wk, gplane, d_W, d_perm, d_rank, d_resid, xplane);
    if (rc) return rc;
    MWCHECK(hipMemcpy(perm, d_perm, (size_t)xplane * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(rank, d_rank, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(W, d_W, gb * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(resid, d_resid, xb * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// Gram + rank reveal per cluster without the Gram matrices leaving the device: S holds G_j and is factored in place (LDS-resident clusters: in LDS), Si is
// the workspace of the clusters beyond LDS, S0 receives the relations.  The context needs a new assembly before its next factorisation.
extern "C" int clrs_mw_constraint_dependencies(clrs_mw_ctx *c, const double *tau, int32_t *perm, int32_t *rank, double *W, double *resid) {
    if (!c || !tau || !perm || !rank || !W || !resid) return mw_fail(CLRS_ERR_INVALID, "null argument");
    int rc = mw_constraint_gram_dev(c);
    if (rc) return rc;
    const MwDev &q = c->d;
    const int K = c->K;
    std::vector<MwRankMat> mats(q.J);
    for (int j = 0; j < q.J; j++) mats[j] = MwRankMat{c->clu[j].P, c->clu[j].P, 0, 0, c->clu[j].Soff, c->clu[j].coff, tau[j]};
    MwRankBufs bufs;
    double *d_resid = nullptr;
    int *d_perm = nullptr, *d_rank = nullptr;
    MWCHECK(bufs.get(&d_resid, (size_t)q.xlen * K)); MWCHECK(bufs.get(&d_perm, (size_t)q.xlen)); MWCHECK(bufs.get(&d_rank, (size_t)q.J));
    MWCHECK(hipMemsetAsync(q.S0, 0, (size_t)std::max<i64>(q.Slen, 1) * K * sizeof(double), c->stream));
    MWCHECK(hipMemsetAsync(d_resid, 0, (size_t)std::max<i64>(q.xlen, 1) * K * sizeof(double), c->stream));
    rc = mw_rank_launch(K, c->stream, mats, q.S, q.Si, q.Slen, q.S0, d_perm, d_rank, d_resid, q.xlen);
    c->assembled = c->factored = c->local_factored = false;      // S, Si and S0 were used as work space
    if (rc) return rc;
    MWCHECK(hipMemcpy(perm, d_perm, (size_t)q.xlen * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(rank, d_rank, (size_t)q.J * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(W, q.S0, (size_t)q.Slen * K * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(resid, d_resid, (size_t)q.xlen * K * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ---- the general batched product (clrs_mw_gemm.hip.h): no context, host pointers, the buffers of one call released on every path ----
static_assert(sizeof(clrs_mw_gemm_job) == sizeof(MwGemmJob) && offsetof(clrs_mw_gemm_job, a_off) == offsetof(MwGemmJob, a_off) &&
              offsetof(clrs_mw_gemm_job, ldc) == offsetof(MwGemmJob, ldc), "MwGemmJob is clrs_mw_gemm_job");

// elements from the first to one past the last of a rows x cols column-major matrix with leading dimension ld (0 when it has none)
static i64 mw_gemm_extent(i64 rows, i64 cols, i64 ld) { return rows > 0 && cols > 0 ? (cols - 1) * ld + rows : 0; }

extern "C" int clrs_mw_gemm(int device, int limbs, int njobs, const clrs_mw_gemm_job *jobs, const double *A, int64_t a_plane, const double *B, int64_t b_plane,
                            double *C, int64_t c_plane) {
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return mw_fail(CLRS_ERR_INVALID, "gemm: limbs must be 4, 5, 6, 8 or 10");
    if (njobs < 0 || (njobs > 0 && !jobs)) return mw_fail(CLRS_ERR_INVALID, "gemm: null or negative job list");
    if (a_plane < 0 || b_plane < 0 || c_plane < 0) return mw_fail(CLRS_ERR_INVALID, "gemm: negative plane length");
    std::vector<int> tiles;                                   // (job, tile row, tile column) of every tile of every non-empty C
    std::vector<std::pair<i64, i64>> ranges;                  // [first, end) of every non-empty C
    bool reads_ab = false, reads_c = false;
    for (int t = 0; t < njobs; t++) {
        const clrs_mw_gemm_job &q = jobs[t];
        const std::string at = "gemm: job " + std::to_string(t) + ": ";
        if (q.m < 0 || q.n < 0 || q.k < 0) return mw_fail(CLRS_ERR_INVALID, at + "negative size");
        if (q.alpha != 1 && q.alpha != -1) return mw_fail(CLRS_ERR_INVALID, at + "alpha must be -1 or +1");
        if (q.beta < -1 || q.beta > 1) return mw_fail(CLRS_ERR_INVALID, at + "beta must be -1, 0 or +1");
        if (q.a_off < 0 || q.b_off < 0 || q.c_off < 0) return mw_fail(CLRS_ERR_INVALID, at + "negative offset");
        const i64 ra = q.transa ? q.k : q.m, ca = q.transa ? q.m : q.k, rb = q.transb ? q.n : q.k, cb = q.transb ? q.k : q.n;
        if (q.lda < ra || q.ldb < rb || q.ldc < q.m) return mw_fail(CLRS_ERR_INVALID, at + "leading dimension smaller than the rows it holds");
        const i64 ea = mw_gemm_extent(ra, ca, q.lda), eb = mw_gemm_extent(rb, cb, q.ldb), ec = mw_gemm_extent(q.m, q.n, q.ldc);
        if (ec == 0) continue;                                 // m = 0 or n = 0: nothing is read, nothing is written
        if (!C || (ea && !A) || (eb && !B)) return mw_fail(CLRS_ERR_INVALID, at + "null pool");
        if (q.a_off > a_plane || ea > a_plane - q.a_off || q.b_off > b_plane || eb > b_plane - q.b_off || q.c_off > c_plane || ec > c_plane - q.c_off) return mw_fail(CLRS_ERR_INVALID, at + "matrix leaves its plane");
        reads_ab = reads_ab || ea;
        reads_c = reads_c || q.beta != 0;
        ranges.emplace_back(q.c_off, q.c_off + ec);
        for (int tj = 0; tj < (q.n + MW_GEMM_T - 1) / MW_GEMM_T; tj++)
            for (int ti = 0; ti < (q.m + MW_GEMM_T - 1) / MW_GEMM_T; ti++) { tiles.push_back(t); tiles.push_back(ti); tiles.push_back(tj); }
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++)
        if (ranges[i].first < ranges[i - 1].second) return mw_fail(CLRS_ERR_INVALID, "gemm: the C ranges of two jobs overlap");
    if (tiles.empty()) return 0;
    MWCHECK(hipSetDevice(device));
    MwRankBufs bufs;
    const bool same = A == B && a_plane == b_plane;
    const size_t na = reads_ab ? (size_t)a_plane * limbs : 0, nb = reads_ab && !same ? (size_t)b_plane * limbs : 0, nc = (size_t)c_plane * limbs;
    double *d_A = nullptr, *d_B = nullptr, *d_C = nullptr;
    MwGemmJob *d_jobs = nullptr;
    int *d_tiles = nullptr;
    MWCHECK(bufs.get(&d_A, na)); MWCHECK(bufs.get(&d_B, nb)); MWCHECK(bufs.get(&d_C, nc));
    MWCHECK(bufs.get(&d_jobs, (size_t)njobs)); MWCHECK(bufs.get(&d_tiles, tiles.size()));
    if (na && A) MWCHECK(hipMemcpy(d_A, A, na * sizeof(double), hipMemcpyHostToDevice));
    if (nb && B) MWCHECK(hipMemcpy(d_B, B, nb * sizeof(double), hipMemcpyHostToDevice));
    // C goes up only when some job reads it (beta != 0); entries no job writes then come back as they went.  When no job reads C, the pool comes down into a
    // buffer of its own and only the m x n entries the jobs wrote are copied over the caller's.
    if (reads_c) MWCHECK(hipMemcpy(d_C, C, nc * sizeof(double), hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(d_jobs, jobs, (size_t)njobs * sizeof(MwGemmJob), hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice));
    const double *d_Bk = same ? d_A : d_B;
    const unsigned grid = (unsigned)(tiles.size() / 3);
#define MW_GEMM_CASE(Kc)                                                                                                                                          \
    case Kc:                                                                                                                                                      \
        hipLaunchKernelGGL(k_mw_gemm<Kc>, dim3(grid), dim3(MW_NT), MW_GEMM_LDS(Kc), nullptr, d_jobs, d_tiles, d_A, (mwi64)a_plane, \
                           d_Bk, (mwi64)b_plane, d_C, (mwi64)c_plane);                                                                                           \
        break;
    switch (limbs) { MW_GEMM_CASE(4) MW_GEMM_CASE(5) MW_GEMM_CASE(6) MW_GEMM_CASE(8) MW_GEMM_CASE(10) }
#undef MW_GEMM_CASE
    MWCHECK(hipGetLastError());
    MWCHECK(hipStreamSynchronize(nullptr));
    if (reads_c) {
        MWCHECK(hipMemcpy(C, d_C, nc * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    std::vector<double> back(nc);
    MWCHECK(hipMemcpy(back.data(), d_C, nc * sizeof(double), hipMemcpyDeviceToHost));
    for (int t = 0; t < njobs; t++) {
        const clrs_mw_gemm_job &q = jobs[t];
        if (q.m == 0) continue;
        for (int l = 0; l < limbs; l++)
            for (i64 j = 0; j < q.n; j++) {
                const i64 o = (i64)l * c_plane + q.c_off + j * q.ldc;
                memcpy(C + o, back.data() + o, (size_t)q.m * sizeof(double));
            }
    }
    return 0;
}

// ---- the SPD solve (clrs_mw_posv.hip.h): no context, host pointers, the buffers and events of one call released on every path ----
struct MwPosvEvents {
    std::vector<hipEvent_t> e;
    ~MwPosvEvents() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
    hipError_t get(size_t count) {
        for (size_t i = 0; i < count; i++) {
            hipEvent_t x;
            hipError_t r = hipEventCreate(&x);
            if (r != hipSuccess) return r;
            e.push_back(x);
        }
        return hipSuccess;
    }
};
static thread_local double t_posv_diag_ms = 0.0, t_posv_whole_ms = 0.0;
static thread_local int t_posv_timing = 0;      // clrs_mw_posv_times switches the per-panel events on for this thread's later calls

extern "C" int clrs_mw_posv_times(double *diag_ms, double *gemm_ms, double *whole_ms) {
    if (!diag_ms || !gemm_ms || !whole_ms) return mw_fail(CLRS_ERR_INVALID, "posv_times: null argument");
    t_posv_timing = 1;
    *diag_ms = t_posv_diag_ms;
    *gemm_ms = t_posv_whole_ms - t_posv_diag_ms;
    *whole_ms = t_posv_whole_ms;
    return 0;
}

extern "C" int clrs_mw_posv(int device, int limbs, int n, int nrhs, const double *A, int a_plane, const double *B, int b_plane, double *X, int x_plane,
                            int32_t *info) {
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return mw_fail(CLRS_ERR_INVALID, "posv: limbs must be 4, 5, 6, 8 or 10");
    if (n < 0 || nrhs < 0) return mw_fail(CLRS_ERR_INVALID, "posv: negative size");
    const i64 nn = (i64)n * n, nr = (i64)n * nrhs;
    if (a_plane < nn || b_plane < nr || x_plane < nr) return mw_fail(CLRS_ERR_INVALID, "posv: a plane is smaller than its matrix");
    if (nr == 0) return 0;
    if (!A || !B || !X || !info) return mw_fail(CLRS_ERR_INVALID, "posv: null argument");
    t_posv_diag_ms = t_posv_whole_ms = 0.0;
    const MwPosvPlan q = mw_posv_plan(n, nrhs);
    MWCHECK(hipSetDevice(device));
    MwRankBufs bufs;
    MwPosvEvents ev;
    double *d_pool = nullptr;
    MwGemmJob *d_jobs = nullptr;
    int *d_tiles = nullptr, *d_status = nullptr;
    MWCHECK(bufs.get(&d_pool, (size_t)q.plane * limbs));
    MWCHECK(bufs.get(&d_jobs, q.jobs.size())); MWCHECK(bufs.get(&d_tiles, q.tiles.size())); MWCHECK(bufs.get(&d_status, 1));
    const bool timing = t_posv_timing != 0;                   // two events per call; two more per diagonal launch only once the times were asked for
    MWCHECK(ev.get(2 + (timing ? 2 * (size_t)q.npanels : 0)));
    MWCHECK(hipMemset(d_pool, 0, (size_t)q.plane * limbs * sizeof(double)));
    MWCHECK(hipMemset(d_status, 0, sizeof(int)));
    for (int l = 0; l < limbs; l++) {
        MWCHECK(hipMemcpy(d_pool + (size_t)l * q.plane + q.s_off, A + (size_t)l * a_plane, (size_t)nn * sizeof(double), hipMemcpyHostToDevice));
        MWCHECK(hipMemcpy(d_pool + (size_t)l * q.plane + q.b_off, B + (size_t)l * b_plane, (size_t)nr * sizeof(double), hipMemcpyHostToDevice));
    }
    MWCHECK(hipMemcpy(d_jobs, q.jobs.data(), q.jobs.size() * sizeof(MwGemmJob), hipMemcpyHostToDevice));      // the tables of every launch, once
    MWCHECK(hipMemcpy(d_tiles, q.tiles.data(), q.tiles.size() * sizeof(int), hipMemcpyHostToDevice));
    MWCHECK(hipEventRecord(ev.e[0], nullptr));
    for (const MwPosvLaunch &ln : q.launches) {
        const int c0 = ln.panel * MW_POSV_T, nb = std::min(n - c0, MW_POSV_T);
        const i64 blk = c0 + (i64)c0 * n;
        if (ln.diag && timing) MWCHECK(hipEventRecord(ev.e[2 + 2 * ln.panel], nullptr));
#define MW_POSV_CASE(Kc)                                                                                                                                          \
    case Kc:                                                                                                                                                      \
        if (ln.diag)                                                                                                                                              \
            hipLaunchKernelGGL(k_mw_posv_diag<Kc>, dim3(1), dim3(MW_NT), MW_POSV_LDS(Kc), nullptr, d_pool, (mwi64)q.plane, (mwi64)(q.s_off + blk),                \
                               (mwi64)(q.l_off + blk), n, (mwi64)(q.w_off + (i64)ln.panel * MW_POSV_PL), nb, c0, d_status);                                       \
        else                                                                                                                                                      \
            hipLaunchKernelGGL(k_mw_gemm<Kc>, dim3((unsigned)ln.ntiles), dim3(MW_NT), MW_GEMM_LDS(Kc), nullptr, d_jobs, d_tiles + 3 * (size_t)ln.tile0, d_pool,   \
                               (mwi64)q.plane, d_pool, (mwi64)q.plane, d_pool, (mwi64)q.plane);                                                                   \
        break;
        switch (limbs) { MW_POSV_CASE(4) MW_POSV_CASE(5) MW_POSV_CASE(6) MW_POSV_CASE(8) MW_POSV_CASE(10) }
#undef MW_POSV_CASE
        MWCHECK(hipGetLastError());
        if (ln.diag && timing) MWCHECK(hipEventRecord(ev.e[3 + 2 * ln.panel], nullptr));
    }
    MWCHECK(hipEventRecord(ev.e[1], nullptr));
    MWCHECK(hipStreamSynchronize(nullptr));
    float ms = 0.f;
    MWCHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    t_posv_whole_ms = ms;
    for (int p = 0; timing && p < q.npanels; p++) {
        MWCHECK(hipEventElapsedTime(&ms, ev.e[2 + 2 * p], ev.e[3 + 2 * p]));
        t_posv_diag_ms += ms;
    }
    int status = 0;
    MWCHECK(hipMemcpy(&status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> back(status ? 0 : (size_t)nr * limbs);
    if (!status)
        for (int l = 0; l < limbs; l++)
            MWCHECK(hipMemcpy(back.data() + (size_t)l * nr, d_pool + (size_t)l * q.plane + q.x_off, (size_t)nr * sizeof(double), hipMemcpyDeviceToHost));
    for (int l = 0; l < limbs; l++) {                         // the outputs are written only once nothing can fail any more
        if (status) memset(X + (size_t)l * x_plane, 0, (size_t)nr * sizeof(double));
        else memcpy(X + (size_t)l * x_plane, back.data() + (size_t)l * nr, (size_t)nr * sizeof(double));
    }
    info[0] = status;
    info[1] = q.npanels;
    return 0;
}

// ---- kernel vectors of solution blocks (clrs_mw_kernel_vectors.hip.h): no context, host pointers, the buffers of one call released on every path ----
// the outputs of the rational rounding (clrs_mw_rational.hip.h); all null: the vectors are not rounded
struct MwKvRational {
    double errbound;
    double *num, *den;
    int32_t *status;
    double *Vq, *resid_max;
};

// the arguments and outputs of the rounding to a number field (clrs_mw_field_round.hip); rel, status, rung, err, info and Vq are pools over
// the plane like V: only the positions of the vectors' entries are written
struct MwKvField {
    int deg;
    const double *gpow;
    int bits;
    double errbound;
    int nd;
    int32_t *rel, *status, *rung;
    double *err, *Vq;
    int32_t *info;
    double *resid_max;
};
// clrs_mw_field_round.hip: the device part of clrs_mw_field_round on compact device pools
int mw_field_round_on_device(int limbs, int deg, const double *gpow, int count, const double *d_v, int bits, double errbound, int nd, int32_t *d_rel,
                             int32_t *d_status, int32_t *d_rung, double *d_err, double *d_vq, int32_t *d_info, double *kernel_ms);

// the entries of the vectors, gathered into a compact pool [limbs][count] and spread back over the plane
static __global__ void k_mw_kv_gather(const double *__restrict__ V, mwi64 plane, const mwi64 *__restrict__ idx, int count, int limbs, double *__restrict__ out) {
    const mwi64 i = (mwi64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const mwi64 o = idx[i];
    if (o < 0 || o >= plane) return;
    for (int l = 0; l < limbs; l++) out[(mwi64)l * count + i] = V[(mwi64)l * plane + o];
}
static __global__ void k_mw_kv_spread(const double *__restrict__ in, const mwi64 *__restrict__ idx, int count, int limbs, double *__restrict__ Vq, mwi64 plane) {
    const mwi64 i = (mwi64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const mwi64 o = idx[i];
    if (o < 0 || o >= plane) return;
    for (int l = 0; l < limbs; l++) Vq[(mwi64)l * plane + o] = in[(mwi64)l * count + i];
}

// the three entries: clrs_mw_kernel_vectors (rat == fld == nullptr), clrs_mw_kernel_vectors_rational (rat) and clrs_mw_kernel_vectors_field (fld)
static int mw_kernel_vectors_run(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual,
                                 double dual_max, int32_t *branch, int32_t *perm, int32_t *rank, int32_t *count, double *V, double *resid_max, double *v_max,
                                 double *pivot_resid, const MwKvRational *rat, const MwKvField *fld = nullptr) {
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: limbs must be 4, 5, 6, 8 or 10");
    if (nblk < 0 || plane < 0) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: negative block count or plane length");
    if (!(tau > 0.0)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: tau must be positive");
    if (nblk > 0 && (!n || !X || !Y || !branch || !perm || !rank || !count || !V || !resid_max || !v_max || !pivot_resid)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: null argument");
    if (rat && !(rat->errbound > 0.0)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: round_errbound must be positive");
    if (rat && nblk > 0 && (!rat->num || !rat->den || !rat->status || !rat->Vq || !rat->resid_max)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: null argument");
    if (fld && !(fld->errbound > 0.0)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: round_errbound must be positive");
    if (fld && (fld->deg < 2 || fld->deg > 4 || fld->bits < 1 || fld->nd < 1 || fld->nd > 20)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: the degree must lie in [2, 4], bits >= 1 and nd in [1, 20]");
    if (fld && nblk > 0 && (!fld->gpow || !fld->rel || !fld->status || !fld->rung || !fld->err || !fld->Vq || !fld->info || !fld->resid_max)) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: null argument");
    std::vector<MwRankMat> mats(nblk);
    std::vector<MwKvBlk> blks(nblk);
    i64 glen = 0, xlen = 0;
    for (int b = 0; b < nblk; b++) {
        if (n[b] < 0) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: negative size");
        mats[b] = MwRankMat{n[b], n[b], 0, 0, glen, xlen, tau};
        blks[b] = MwKvBlk{n[b], MW_KV_PRIMAL, 0, 0, glen, xlen};
        glen += (i64)n[b] * n[b];
        xlen += n[b];
    }
    if (glen > plane) return mw_fail(CLRS_ERR_INVALID, "kernel vectors: the blocks leave their plane");
    if (nblk == 0) return 0;
    // the branch of every block from limb plane 0, and the matrices to eliminate: X_b (dual) or Y_b (primal), copies -- Y is needed again for the residual
    const size_t pool = (size_t)plane * limbs, xb = (size_t)xlen * limbs;
    std::vector<double> G(pool);
    for (int b = 0; b < nblk; b++) {
        const i64 nn = (i64)n[b] * n[b], off = blks[b].off;
        bool dual = use_dual != 0;
        for (i64 e = 0; dual && e < nn; e++) dual = fabs(X[off + e]) <= dual_max;
        blks[b].branch = branch[b] = dual ? MW_KV_DUAL : MW_KV_PRIMAL;
        for (int l = 0; l < limbs; l++) memcpy(G.data() + (i64)l * plane + off, (dual ? X : Y) + (i64)l * plane + off, (size_t)nn * sizeof(double));
    }
    MWCHECK(hipSetDevice(device));
    MwRankBufs bufs;
    double *d_G = nullptr, *d_Wk = nullptr, *d_W = nullptr, *d_Y = nullptr, *d_V = nullptr, *d_resid = nullptr, *d_rmax = nullptr, *d_vmax = nullptr;
    int *d_perm = nullptr, *d_rank = nullptr, *d_tiles = nullptr;
    MwKvBlk *d_blks = nullptr;
    MwGemmJob *d_jobs = nullptr;
    MWCHECK(bufs.get(&d_G, pool)); MWCHECK(bufs.get(&d_Wk, pool)); MWCHECK(bufs.get(&d_W, pool)); MWCHECK(bufs.get(&d_Y, pool)); MWCHECK(bufs.get(&d_V, pool));
    MWCHECK(bufs.get(&d_resid, xb)); MWCHECK(bufs.get(&d_rmax, (size_t)xlen)); MWCHECK(bufs.get(&d_vmax, (size_t)xlen));
    MWCHECK(bufs.get(&d_perm, (size_t)xlen)); MWCHECK(bufs.get(&d_rank, (size_t)nblk)); MWCHECK(bufs.get(&d_blks, (size_t)nblk));
    MWCHECK(hipMemcpy(d_G, G.data(), pool * sizeof(double), hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(d_Y, Y, pool * sizeof(double), hipMemcpyHostToDevice));
    MWCHECK(hipMemcpy(d_V, V, pool * sizeof(double), hipMemcpyHostToDevice));        // entries outside n_b x count_b come back as they went
    MWCHECK(hipMemset(d_W, 0, std::max<size_t>(pool, 1) * sizeof(double)));
    MWCHECK(hipMemset(d_resid, 0, std::max<size_t>(xb, 1) * sizeof(double)));
    MWCHECK(hipMemset(d_rmax, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
    MWCHECK(hipMemset(d_vmax, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
    // the rounded vectors and what goes with them: uploaded like V, so that what the vectors do not cover comes back as it went
    double *d_num = nullptr, *d_den = nullptr, *d_Vq = nullptr, *d_rmax2 = nullptr, *d_vmax2 = nullptr;
    int *d_status = nullptr;
    mwi64 *d_idx = nullptr;
    if (fld) {
        MWCHECK(bufs.get(&d_Vq, pool)); MWCHECK(bufs.get(&d_rmax2, (size_t)xlen)); MWCHECK(bufs.get(&d_vmax2, (size_t)xlen));
        MWCHECK(hipMemcpy(d_Vq, fld->Vq, pool * sizeof(double), hipMemcpyHostToDevice));
        MWCHECK(hipMemset(d_rmax2, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
        MWCHECK(hipMemset(d_vmax2, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
    }
    if (rat) {
        MWCHECK(bufs.get(&d_num, (size_t)plane)); MWCHECK(bufs.get(&d_den, (size_t)plane)); MWCHECK(bufs.get(&d_status, (size_t)plane)); MWCHECK(bufs.get(&d_Vq, pool));
        MWCHECK(bufs.get(&d_rmax2, (size_t)xlen)); MWCHECK(bufs.get(&d_vmax2, (size_t)xlen));
        MWCHECK(hipMemcpy(d_num, rat->num, (size_t)plane * sizeof(double), hipMemcpyHostToDevice));
        MWCHECK(hipMemcpy(d_den, rat->den, (size_t)plane * sizeof(double), hipMemcpyHostToDevice));
        MWCHECK(hipMemcpy(d_status, rat->status, (size_t)plane * sizeof(int), hipMemcpyHostToDevice));
        MWCHECK(hipMemcpy(d_Vq, rat->Vq, pool * sizeof(double), hipMemcpyHostToDevice));
        MWCHECK(hipMemset(d_rmax2, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
        MWCHECK(hipMemset(d_vmax2, 0, std::max<size_t>(xlen, 1) * sizeof(double)));
    }
    // ONE elimination launch over all blocks (it returns synchronised)
    int rc = mw_rank_launch(limbs, nullptr, mats, d_G, d_Wk, plane, d_W, d_perm, d_rank, d_resid, xlen);
    if (rc) return rc;
    MWCHECK(hipMemcpy(rank, d_rank, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(perm, d_perm, (size_t)xlen * sizeof(int), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(pivot_resid, d_resid, xb * sizeof(double), hipMemcpyDeviceToHost));
    // the product R_b = Y_b V_b of every block that has vectors: jobs and tiles as clrs_mw_gemm builds them; R goes where the eliminated copies were
    double *d_R = d_G;
    std::vector<MwGemmJob> jobs;
    std::vector<int> tiles;
    std::vector<mwi64> idx;                                   // the positions of the vectors' entries in the plane (the numbers to round)
    for (int b = 0; b < nblk; b++) {
        const int nb = n[b], r = rank[b];
        if (r < 0 || r > nb) return mw_fail(CLRS_ERR_HIP, "kernel vectors: the elimination returned a rank outside 0 .. n");
        blks[b].rank = r;
        blks[b].count = count[b] = blks[b].branch == MW_KV_DUAL ? r : nb - r;
        if (count[b] == 0) continue;
        if (rat || fld) for (i64 e = 0; e < (i64)nb * count[b]; e++) idx.push_back(blks[b].off + e);
        const int t = (int)jobs.size();
        jobs.push_back(MwGemmJob{nb, count[b], nb, 0, 0, 1, 0, nb, nb, nb, blks[b].off, blks[b].off, blks[b].off});
        for (int tj = 0; tj < (count[b] + MW_GEMM_T - 1) / MW_GEMM_T; tj++)
            for (int ti = 0; ti < (nb + MW_GEMM_T - 1) / MW_GEMM_T; ti++) { tiles.push_back(t); tiles.push_back(ti); tiles.push_back(tj); }
    }
    MWCHECK(bufs.get(&d_jobs, jobs.size())); MWCHECK(bufs.get(&d_tiles, tiles.size()));
    MWCHECK(hipMemcpy(d_blks, blks.data(), (size_t)nblk * sizeof(MwKvBlk), hipMemcpyHostToDevice));
    if (!jobs.empty()) {
        MWCHECK(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(MwGemmJob), hipMemcpyHostToDevice));
        MWCHECK(hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice));
        const unsigned grid = (unsigned)(tiles.size() / 3);
#define MW_KV_CASE(Kc)                                                                                                                                            \
    case Kc:                                                                                                                                                      \
        hipLaunchKernelGGL(k_mw_kv_scatter<Kc>, dim3((unsigned)nblk), dim3(MW_NT), 0, nullptr, d_blks, d_perm, d_W, d_V, (mwi64)plane);                            \
        hipLaunchKernelGGL(k_mw_gemm<Kc>, dim3(grid), dim3(MW_NT), MW_GEMM_LDS(Kc), nullptr, d_jobs, d_tiles, d_Y, (mwi64)plane, d_V, (mwi64)plane, d_R,          \
                           (mwi64)plane);                                                                                                                         \
        break;
        switch (limbs) { MW_KV_CASE(4) MW_KV_CASE(5) MW_KV_CASE(6) MW_KV_CASE(8) MW_KV_CASE(10) }
#undef MW_KV_CASE
        hipLaunchKernelGGL(k_mw_kv_colmax, dim3((unsigned)nblk), dim3(MW_NT), 0, nullptr, d_blks, d_R, d_V, d_rmax, d_vmax);
        MWCHECK(hipGetLastError());
        if (rat) {
            // every entry of every vector rounded (one lane each), then the second check of the reference: Y_b Vq_b by the same job list (R is overwritten:
            // its maxima are taken) and its column maxima
            MWCHECK(bufs.get(&d_idx, idx.size()));
            MWCHECK(hipMemcpy(d_idx, idx.data(), idx.size() * sizeof(mwi64), hipMemcpyHostToDevice));
            const unsigned rgrid = (unsigned)((idx.size() + MW_NT - 1) / MW_NT);
#define MW_KV_CASE(Kc)                                                                                                                                            \
    case Kc:                                                                                                                                                      \
        hipLaunchKernelGGL(k_mw_rationalize<Kc>, dim3(rgrid), dim3(MW_NT), 0, nullptr, d_V, (mwi64)plane, d_idx, (int)idx.size(), rat->errbound, d_num, d_den,    \
                           d_status, d_Vq);                                                                                                                       \
        hipLaunchKernelGGL(k_mw_gemm<Kc>, dim3(grid), dim3(MW_NT), MW_GEMM_LDS(Kc), nullptr, d_jobs, d_tiles, d_Y, (mwi64)plane, d_Vq, (mwi64)plane, d_R,         \
                           (mwi64)plane);                                                                                                                         \
        break;
            switch (limbs) { MW_KV_CASE(4) MW_KV_CASE(5) MW_KV_CASE(6) MW_KV_CASE(8) MW_KV_CASE(10) }
#undef MW_KV_CASE
            hipLaunchKernelGGL(k_mw_kv_colmax, dim3((unsigned)nblk), dim3(MW_NT), 0, nullptr, d_blks, d_R, d_Vq, d_rmax2, d_vmax2);
            MWCHECK(hipGetLastError());
        }
        if (fld) {
            // every entry of every vector rounded to the field (one lane each, on a compact pool), the elements spread back into Vq, then the second check as above
            const int m = (int)idx.size(), D = fld->deg + 1;
            double *d_vc = nullptr, *d_vqc = nullptr, *d_errc = nullptr;
            int32_t *d_relc = nullptr, *d_statc = nullptr, *d_rungc = nullptr, *d_infoc = nullptr;
            MWCHECK(bufs.get(&d_idx, idx.size())); MWCHECK(bufs.get(&d_vc, (size_t)limbs * m)); MWCHECK(bufs.get(&d_vqc, (size_t)limbs * m));
            MWCHECK(bufs.get(&d_errc, (size_t)m)); MWCHECK(bufs.get(&d_relc, (size_t)fld->nd * D * m)); MWCHECK(bufs.get(&d_statc, (size_t)m));
            MWCHECK(bufs.get(&d_rungc, (size_t)m)); MWCHECK(bufs.get(&d_infoc, (size_t)2 * m));
            MWCHECK(hipMemcpy(d_idx, idx.data(), idx.size() * sizeof(mwi64), hipMemcpyHostToDevice));
            const unsigned ggrid = (unsigned)((idx.size() + MW_NT - 1) / MW_NT);
            hipLaunchKernelGGL(k_mw_kv_gather, dim3(ggrid), dim3(MW_NT), 0, nullptr, d_V, (mwi64)plane, d_idx, m, limbs, d_vc);
            MWCHECK(hipGetLastError());
            double kernel_ms = 0.0;
            rc = mw_field_round_on_device(limbs, fld->deg, fld->gpow, m, d_vc, fld->bits, fld->errbound, fld->nd, d_relc, d_statc, d_rungc, d_errc, d_vqc, d_infoc, &kernel_ms);
            if (rc) return rc;
            hipLaunchKernelGGL(k_mw_kv_spread, dim3(ggrid), dim3(MW_NT), 0, nullptr, d_vqc, d_idx, m, limbs, d_Vq, (mwi64)plane);
#define MW_KV_CASE(Kc)                                                                                                                                            \
    case Kc:                                                                                                                                                      \
        hipLaunchKernelGGL(k_mw_gemm<Kc>, dim3(grid), dim3(MW_NT), MW_GEMM_LDS(Kc), nullptr, d_jobs, d_tiles, d_Y, (mwi64)plane, d_Vq, (mwi64)plane, d_R,         \
                           (mwi64)plane);                                                                                                                         \
        break;
            switch (limbs) { MW_KV_CASE(4) MW_KV_CASE(5) MW_KV_CASE(6) MW_KV_CASE(8) MW_KV_CASE(10) }
#undef MW_KV_CASE
            hipLaunchKernelGGL(k_mw_kv_colmax, dim3((unsigned)nblk), dim3(MW_NT), 0, nullptr, d_blks, d_R, d_Vq, d_rmax2, d_vmax2);
            MWCHECK(hipGetLastError());
            MWCHECK(hipStreamSynchronize(nullptr));
            std::vector<int32_t> h_rel((size_t)fld->nd * D * m), h_stat((size_t)m), h_rung((size_t)m), h_info((size_t)2 * m);
            std::vector<double> h_err((size_t)m);
            MWCHECK(hipMemcpy(h_rel.data(), d_relc, h_rel.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(h_stat.data(), d_statc, h_stat.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(h_rung.data(), d_rungc, h_rung.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(h_info.data(), d_infoc, h_info.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(h_err.data(), d_errc, h_err.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int i = 0; i < m; i++) {
                const i64 o = idx[(size_t)i];
                for (int r = 0; r < fld->nd * D; r++) fld->rel[(i64)r * plane + o] = h_rel[(size_t)r * m + i];
                fld->status[o] = h_stat[(size_t)i];
                fld->rung[o] = h_rung[(size_t)i];
                fld->err[o] = h_err[(size_t)i];
                fld->info[o] = h_info[(size_t)i];
                fld->info[(i64)plane + o] = h_info[(size_t)m + i];
            }
            MWCHECK(hipMemcpy(fld->Vq, d_Vq, pool * sizeof(double), hipMemcpyDeviceToHost));
        }
        MWCHECK(hipStreamSynchronize(nullptr));
        MWCHECK(hipMemcpy(V, d_V, pool * sizeof(double), hipMemcpyDeviceToHost));
        if (rat) {
            MWCHECK(hipMemcpy(rat->num, d_num, (size_t)plane * sizeof(double), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(rat->den, d_den, (size_t)plane * sizeof(double), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(rat->status, d_status, (size_t)plane * sizeof(int), hipMemcpyDeviceToHost));
            MWCHECK(hipMemcpy(rat->Vq, d_Vq, pool * sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    if (rat) MWCHECK(hipMemcpy(rat->resid_max, d_rmax2, (size_t)xlen * sizeof(double), hipMemcpyDeviceToHost));
    if (fld) MWCHECK(hipMemcpy(fld->resid_max, d_rmax2, (size_t)xlen * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(resid_max, d_rmax, (size_t)xlen * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(v_max, d_vmax, (size_t)xlen * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int clrs_mw_kernel_vectors(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual,
                                      double dual_max, int32_t *branch, int32_t *perm, int32_t *rank, int32_t *count, double *V, double *resid_max, double *v_max,
                                      double *pivot_resid) {
    return mw_kernel_vectors_run(device, limbs, nblk, n, X, Y, plane, tau, use_dual, dual_max, branch, perm, rank, count, V, resid_max, v_max, pivot_resid, nullptr);
}

extern "C" int clrs_mw_kernel_vectors_rational(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau,
                                               int use_dual, double dual_max, double round_errbound, int32_t *branch, int32_t *perm, int32_t *rank,
                                               int32_t *count, double *V, double *resid_max, double *v_max, double *pivot_resid, double *num, double *den,
                                               int32_t *status, double *Vq, double *round_resid_max) {
    const MwKvRational rat{round_errbound, num, den, status, Vq, round_resid_max};
    return mw_kernel_vectors_run(device, limbs, nblk, n, X, Y, plane, tau, use_dual, dual_max, branch, perm, rank, count, V, resid_max, v_max, pivot_resid, &rat);
}

extern "C" int clrs_mw_kernel_vectors_field(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual,
                                            double dual_max, double round_errbound, int deg, const double *gpow, int bits, int nd, int32_t *branch, int32_t *perm,
                                            int32_t *rank, int32_t *count, double *V, double *resid_max, double *v_max, double *pivot_resid, int32_t *rel,
                                            int32_t *status, int32_t *rung, double *err, double *Vq, int32_t *info, double *round_resid_max) {
    const MwKvField fld{deg, gpow, bits, round_errbound, nd, rel, status, rung, err, Vq, info, round_resid_max};
    return mw_kernel_vectors_run(device, limbs, nblk, n, X, Y, plane, tau, use_dual, dual_max, branch, perm, rank, count, V, resid_max, v_max, pivot_resid, nullptr, &fld);
}

// ---- rounding to rationals (clrs_mw_rational.hip.h): no context, host pointers.  The device pool is compact (plane = count), so nothing behind the first
// `count` entries of any of the caller's planes is read or written ----
extern "C" int clrs_mw_rationalize(int device, int limbs, int count, const double *v, int plane, double errbound, double *num, double *den, int32_t *status,
                                   double *vq) {
    if (limbs != 4 && limbs != 5 && limbs != 6 && limbs != 8 && limbs != 10) return mw_fail(CLRS_ERR_INVALID, "rationalize: limbs must be 4, 5, 6, 8 or 10");
    if (count < 0) return mw_fail(CLRS_ERR_INVALID, "rationalize: negative count");
    if (plane < count) return mw_fail(CLRS_ERR_INVALID, "rationalize: the numbers leave their plane");
    if (!(errbound > 0.0)) return mw_fail(CLRS_ERR_INVALID, "rationalize: errbound must be positive");
    if (count > 0 && (!v || !num || !den || !status || !vq)) return mw_fail(CLRS_ERR_INVALID, "rationalize: null argument");
    if (count == 0) return 0;
    MWCHECK(hipSetDevice(device));
    MwRankBufs bufs;
    const size_t cnt = (size_t)count;
    double *d_v = nullptr, *d_vq = nullptr, *d_num = nullptr, *d_den = nullptr;
    int *d_status = nullptr;
    MWCHECK(bufs.get(&d_v, cnt * limbs)); MWCHECK(bufs.get(&d_vq, cnt * limbs)); MWCHECK(bufs.get(&d_num, cnt)); MWCHECK(bufs.get(&d_den, cnt));
    MWCHECK(bufs.get(&d_status, cnt));
    for (int l = 0; l < limbs; l++) MWCHECK(hipMemcpy(d_v + (size_t)l * cnt, v + (size_t)l * plane, cnt * sizeof(double), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((cnt + MW_NT - 1) / MW_NT);
#define MW_RAT_CASE(Kc)                                                                                                                                           \
    case Kc:                                                                                                                                                      \
        hipLaunchKernelGGL(k_mw_rationalize<Kc>, dim3(grid), dim3(MW_NT), 0, nullptr, d_v, (mwi64)count, (const mwi64 *)nullptr, count, errbound, d_num, d_den,   \
                           d_status, d_vq);                                                                                                                       \
        break;
    switch (limbs) { MW_RAT_CASE(4) MW_RAT_CASE(5) MW_RAT_CASE(6) MW_RAT_CASE(8) MW_RAT_CASE(10) }
#undef MW_RAT_CASE
    MWCHECK(hipGetLastError());
    MWCHECK(hipStreamSynchronize(nullptr));
    MWCHECK(hipMemcpy(num, d_num, cnt * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(den, d_den, cnt * sizeof(double), hipMemcpyDeviceToHost));
    MWCHECK(hipMemcpy(status, d_status, cnt * sizeof(int), hipMemcpyDeviceToHost));
    for (int l = 0; l < limbs; l++) MWCHECK(hipMemcpy(vq + (size_t)l * plane, d_vq + (size_t)l * cnt, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

#include "clrs_mw_ipm_host.inc"

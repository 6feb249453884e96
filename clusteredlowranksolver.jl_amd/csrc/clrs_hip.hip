// clrs_hip.hip -- host side of the C ABI (include/clrs_hip.h): context creation (vector
// de-duplication, gather tables, launch plan), and the per-iteration drivers that replay the plan.
//
// Design (MI355X-first, not a translation of the reference's j -> l -> r -> s serial walk):
//   * every step of the path is ONE grouped launch over all PSD blocks / clusters, driven by
//     device-resident descriptor tables that are built once at context creation;
//   * blocked Cholesky / triangular solves are level-synchronous across matrices: panel k of every
//     matrix is processed by the same launch;
//   * the explicit inverse of X (reference "method 3", src/solver.jl:1107-1119) is avoided:
//     V^T X^-1 V = (L^-1 V)^T (L^-1 V), one triangular solve + one MFMA contraction;
//   * each S entry is produced by exactly one thread (deterministic, no atomics);
//   * the launch sequences are static, so they can be captured into hipGraphs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/clrs_hip.h"
#include "clrs_kernels.hip.h"
#include "clrs_fused.hip.h"
#include "clrs_assemble_w3.hip.h"
#include "clrs_assemble_w4.hip.h"
#include "clrs_assemble_w5.hip.h"
#include "clrs_solve_small.hip.h"
#include "clrs_factor_small.hip.h"
#include "clrs_ipm.hip.h"

using namespace clrs;
typedef long long i64;

static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}
extern "C" void clrs_set_last_error(const char *msg) { g_last_error = msg ? msg : ""; }   // for the other translation units of the library (clrs_mw.hip)
#define HIPCHECK(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(CLRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

static const int INFO_NONE = 0x7f7f7f7f;

// process-wide knobs read at context creation (clrs_config_set)
static int g_cfg_fused_assemble = 1;
static int g_cfg_split_blocks = 1;      // fused general assembly: one workgroup per PSD block (partial S_j slabs, summed in block order) when the launch is far from filling the chip
static int g_cfg_fused_factor = 1;
static int g_cfg_wave_assemble = 1;
static int g_cfg_wave2_assemble = 1;
static int g_cfg_wave5_assemble = 1;   // k_cluster_assemble_w5: the register-resident form for 2 x 2 blocks of 16 x 16 sub-blocks with shared sample vectors (Nsphere_packing); 0: the general kernels
static int g_cfg_wave4_assemble = 1;   // k_cluster_assemble_w4: the register-resident form for simple blocks of up to 32 rows and up to 64 constraints; 0: the general kernels
static int g_cfg_wave3_assemble = 1;   // register-resident form of the cluster-per-wave assembly (U <= 32); 0: k_cluster_assemble_w2
static int g_cfg_dense_block = 1;
static int g_cfg_trsm_blockinv = 1;  // triangular solves with n > TRSM_IB through inverted diagonal blocks (plan_trsm_blockinv)
static int g_cfg_potrf_levels = 1;   // Cholesky of matrices beyond one block: one launch per block column (plan_potrf_levels)
static int g_cfg_pairing_tri = 1;    // staged low-rank blocks with W = V: lower triangles of the pairing matrices only
static int g_cfg_factor_aug = 1;     // clusters beyond one block, <= 512 free variables: L_j, L_j^-1 B_j and Q from one factorisation of [S_j .; B_j^T 0] each
static int g_cfg_dense_wave = 1;      // dense blocks with n <= 32 beyond k_dense_block: one wave per (block, matrix), k_dense_T32
static int g_cfg_factor_small = 1;      // factor + Q in one launch of one workgroup for <= 4 small clusters (0: k_cluster_factor + k_small_potrf)
static int g_cfg_solve_small_max = 32768;     // one-workgroup solve stage only up to this many doubles of operands (beyond: one workgroup per cluster, three launches)
static int g_cfg_ipm_wmfma = 3;         // device interior-point loop, bit 0: sum_i a_i A_i of a low-rank block as an MFMA contraction over its terms; bit 1: Z V by MFMA (0: per-entry loops)
int g_cfg_mw_stream_words = 1;        // multi-word interior-point iteration: its two streams synchronise through words that kernels store and await (1) or through events only (0: for counter-collection runs, whose profiler serialises kernels -- a kernel that waits for one that cannot start sits in its bounded polls); env CLRS_MW_STREAM_WORDS overrides
int g_cfg_mw_pipeline64 = 1;          // multi-word path: clusters of 33 .. 64 rows through the 64-row form of the pipelined factorisation (k_mw_factor_pipe64); 0: the one-workgroup kernels
int g_cfg_mw_zt_small_maxn = 64;       // multi-word path: T = Y V, Z = chol(X)^-1 V with two columns per workgroup and eight lanes per entry (instead of eight columns, two lanes) for blocks of at most this many rows
int g_cfg_modp_minors_chunk_bytes = 0; // clrs_modp_minors: the residue buffer of a chunk of primes stays below this many bytes; 0: the 256 MiB of clrs_modp_minors.hip.h (a small value makes a call take several chunks: for the tests)
int g_cfg_zz_gemm_chunk_bytes = 0;     // clrs_zz_gemm: the (lo, hi) buffer of a range of digits of B stays below this many bytes; 0: the 256 MiB of clrs_modp_zz_gemm.hip.h (a small value makes a call take several ranges: for the tests)
int g_cfg_liftm_chunk_bytes = 0;       // clrs_modp_dixon_lift_multi: the buffers of a chunk of columns stay below this many bytes; 0: the 256 MiB of clrs_modp_liftm.hip.h (a small value makes a call take several chunks: for the tests)
int g_cfg_lrsys_chunk_bytes = 0;       // clrs_zz_lowrank_system: the int64 sums of a chunk of rows stay below this many bytes; 0: the 256 MiB of clrs_modp_lrsys.hip.h (a small value makes a call take several chunks: for the tests)
int g_cfg_lll_launch_swaps = 0;        // clrs_zz_lll: a launch of k_zz_lll takes at most this many exchanges per lattice, then the host launches again; 0: the 1024 of clrs_zz_lll.hip (a small value cuts a reduction into many launches: for the tests)
int g_cfg_field_round_launch_rungs = 0;  // clrs_mw_field_round: a launch of k_mw_field_round advances a number by at most this many rungs, then the host launches again; 0: the 16 of clrs_mw_field_round_arith.h (the result does not depend on it)
int g_cfg_mw_zi_narrow = 1;          // multi-word interior-point iteration: k_mwi_Zi in workgroups of 256 threads (one wave per SIMD) with panels of half the width where the launch keeps a compute unit per workgroup (clrs_mw_zi_panels.h) -- 0: always 512 threads; read when the context is created
int g_cfg_mw_xinv_product = 1;        // multi-word interior-point iteration: X^-1 = Xi^T Xi formed once per iteration on the side stream (k_mwi_Xv) and applied by k_mwi_Zi as ONE product -- 0: Xi^T (Xi M), two triangular products per launch; read when the context is created
int g_cfg_mw_chain_hop = 1;           // multi-word interior-point iteration: the "last workgroup continues" hand-offs of k_mwi_Zi and k_mwi_step (MwIpmDev::hop) -- 0: release fences (mwk::wg_last_block), 1: write-through stores, a drain and one lane's acquire, 2: write-through stores and loads, no fence; read when the iteration is created
int g_cfg_mw_y_riders = 1;            // multi-word interior-point iteration: the Y pairings of the assembly (T = Y V, GY = V^T T) as riders of the Cholesky launch of the X blocks (k_mw_potrf_x_ride) in small contexts; 0: in k_mw_zt / k_mw_gram; read at context creation
int g_cfg_mw_skip_xfb = 1;            // multi-word path: k_mw_potrf_x leaves out the scaled triangles Xf / Xb (and U^T) in contexts where no substitution path can run (MwDev::no_xfb); 0: always formed; read at context creation
int g_cfg_mw_pipeline_x = 1;           // multi-word path: the Cholesky of the X (and Y) blocks through the pipelines of workgroups (k_mw_potrf_x_pipe) where every block carries its inverse factor; 0: k_mw_potrf_x
int g_cfg_mw_pipeline_x_min = 24;      // ... from this many rows of the largest block on (pipeline = 2: always)
int g_cfg_mw_sharded_factor_limbs = 1; // multi-word loop, sharded contexts: the reduced factor limbs of the mixed-precision refinement there too (the measured first-pass accuracy is gathered with the step lengths); 0: all limbs
int g_cfg_mw_pipeline = 1;            // multi-word path: Cholesky + inverse factor of matrices <= 32 rows as a pipeline of workgroups (clrs_mw_pipe.hip.h); 0: one workgroup chain per matrix
int g_cfg_mw_refine_predictor = 0;    // multi-word interior-point iteration: 1 = the PREDICTOR's solve takes the refinement step too (default: the corrector's only -- the predictor's direction sets beta_c and the second-order term, nothing that moves the iterate)
int g_cfg_mw_refine = 1;              // multi-word path: one step of iterative refinement of the solve stage (k_mw_refine); 0: products with the inverse factors only; 2: the correction in fewer limbs
int g_cfg_mw_affine_corrector = 1;    // multi-word interior-point iteration: the corrector's right-hand side as rhs0 + mu_c tau, with beta_c / mu_c formed on the side stream beside Z0 and its traces (clrs_mw_ipm_host.inc); 0: the corrector waits for mu_c
int g_cfg_mw_factor_limbs = 0;        // multi-word path: limbs of the factor stage and of the solve stage's products (mixed-precision refinement, clrs_mw_kernels.hip.h::mw_kf_of): 0 = automatic (reduced inside clrs_mw_ipm_* while the measured contraction allows, all limbs in the stand-alone entry points); a limb count = that count everywhere
int g_cfg_mw_exact_products = 1;      // multi-word path: pairing matrices through exact slice products on the matrix cores (k_mws_pair): 0 never, 1 when >= 256 blocks are eligible (one per compute unit: below, the chip is not full and the latency-oriented kernels win), 2 always
static int g_cfg_solve_small2 = 1;     // one-workgroup solve stage with all loads up front and single-wave triangular solves (0: k_solve_small)
static const int LDS_BUDGET_DOUBLES = 20000;   // of the 20480 doubles (160 KiB) a workgroup may claim

// ------------------------------------------------------------------------------------------------
// launch plan
// ------------------------------------------------------------------------------------------------
enum StepKind { STEP_MEMCPY, STEP_GEMM, STEP_TRSM, STEP_POTRF, STEP_GATHER_S, STEP_GATHER_SCALAR, STEP_SUB, STEP_MEMSET_INFO, STEP_ZERO_UPPER, STEP_FUSED_ASSEMBLE, STEP_SMALL_POTRF, STEP_CLUSTER_FACTOR, STEP_GEMV_T, STEP_CSOLVE_FWD, STEP_Q_SOLVE, STEP_CSOLVE_BWD, STEP_SUM_SLABS, STEP_ASSEMBLE_W1, STEP_GRAM_SMALL, STEP_ASSEMBLE_W2, STEP_SOLVE_SMALL, STEP_DENSE_BLOCK, STEP_ASSEMBLE_W3, STEP_FACTOR_SMALL, STEP_SUM_S_SLABS, STEP_TRTRI32, STEP_DENSE_T32, STEP_TRTRI_DIAG, STEP_COPY2D, STEP_CHOL_LEVEL, STEP_CHOL_PACK, STEP_CHOL_UNPACK, STEP_ASSEMBLE_W4, STEP_ASSEMBLE_W5, STEP_NKINDS };
static const char *const STEP_NAMES[STEP_NKINDS] = {"hipMemcpyAsync(D2D)", "k_gemm_f64_t", "k_trsm_diag", "k_potrf_diag", "k_schur_gather",
                                                    "k_gather_scalar", "k_sub", "hipMemsetAsync", "k_zero_upper", "k_cluster_assemble", "k_small_potrf", "k_cluster_factor", "k_gemv_t",
                                                    "k_cluster_solve_fwd", "k_q_solve", "k_cluster_solve_bwd", "k_sum_slabs", "k_cluster_assemble_w1", "k_gram_small", "k_cluster_assemble_w2", "k_solve_small", "k_dense_block", "k_cluster_assemble_w3", "k_factor_small", "k_sum_S_slabs", "k_trtri32", "k_dense_T32", "k_trtri_diag", "k_copy2d", "k_chol_level", "k_chol_pack", "k_chol_unpack", "k_cluster_assemble_w4", "k_cluster_assemble_w5"};
static const int KT_MAX_EVENTS = 8192;   // event pairs kept between two clrs_get_kernel_times calls

struct Step {
    StepKind kind;
    int grid = 0;
    void *d0 = nullptr, *d1 = nullptr, *d2 = nullptr;  // device descriptor tables
    void *dst = nullptr;
    const void *src = nullptr;
    size_t bytes = 0;
    i64 n = 0;
    int nmax = 0;
    int aux0 = 0, aux1 = 0;   // kind-specific (STEP_ASSEMBLE_W3: grid size, number of blocks)
    bool s_inverse = false;   // forms the inverted diagonal blocks of the factors L_j of S: skipped while those of the current factorisation exist
};

struct Plan {
    std::vector<Step> steps;
    hipGraphExec_t graph = nullptr;
    const void *captured[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // bindings baked into `graph`
    int launches() const { return (int)steps.size(); }
};

struct DeviceArena {  // bump allocator over one hipMalloc (static tables + work buffers)
    char *base = nullptr;
    size_t size = 0, used = 0;
};

struct TrsmJob {
    const double *L;
    int ldl, n;
    double *B;
    int ldb, nrhs;
};
struct PotrfJob {
    double *A;
    int lda, n, code;
    int stop = 0;     // > 0: factor the first `stop` block columns only (the trailing updates still reach the rest: a Schur complement)
};

struct BlockInfo {
    int j = 0, m = 1, delta = 1, n = 1, kind = 0;
    i64 xyoff = 0, t0 = 0, t1 = 0, d0 = 0, d1 = 0;
    std::vector<int> UR, UL, offR, offL;
    int URt = 0, ULt = 0;
    bool sym = false;
    bool sd_tri = false;      // dense block: only the lower tiles of the symmetric Sd = <A_i, X^-1 A_k Y> are formed (staged Gram GEMM)
    // offsets (in doubles) inside the work / static arenas
    i64 zr_off = -1, zl_off = -1, ty_off = -1, g_off = -1;  // ZR/ZL in the "solve" arena; TY; GX,GY
    int cnt = 0;
    i64 w_off = -1, tt_off = -1, sd_off = -1;
    int *d_tptr = nullptr;   // low rank: [P+1] CSR over the cluster's constraints into the sorted term arrays; dense: [cnt] constraint index
    bool fused = false;      // handled by k_cluster_assemble
};

struct IpmState;

struct clrs_ctx {
    int device = 0;
    int *h_info = nullptr;                             // pinned host copy of the two status words
    // pinned staging arena of the host-pointer entry points: a copy to or from pageable memory goes through the runtime's own
    // staging with a synchronisation per call (10-20 us for a few KB); one memcpy into pinned memory and an async copy do not
    char *pin = nullptr;
    size_t pin_cap = 0, pin_used = 0, pin_demand = 0;
    struct PinOut { void *user; const void *pinned; size_t bytes; };
    std::vector<PinOut> pin_out;
    IpmState *ipm = nullptr;                           // device-resident interior-point iteration (clrs_ipm_*), created on demand
    std::vector<int> h_term_p, h_dense_p;              // host copies of the description arrays the IPM tables are built from
    std::vector<double> h_term_lambda;
    int *d_ayL = nullptr, *d_ayR = nullptr;            // per original term: left / right expanded vector index of its pairing
    hipStream_t stream = nullptr;
    bool own_stream = true;
    // per-kernel HIP-event timing (clrs_set_kernel_timing): -2 off, -1 every step kind, k >= 0 only kind k
    int kt_kind = -2;
    std::vector<hipEvent_t> kt_ev;
    std::vector<int> kt_kinds;
    double kt_total[STEP_NKINDS] = {0};
    long long kt_count[STEP_NKINDS] = {0};
    int J = 0, N = 0, NB = 0;
    i64 T = 0, D = 0;
    std::vector<int> P;
    std::vector<i64> coff, Soff;
    i64 xylen = 0, xlen = 0, Slen = 0;
    std::vector<BlockInfo> blk;
    std::vector<void *> allocs;  // every hipMalloc, for destroy
    // device buffers
    std::vector<CholLevelJob> chol_jobs;           // jobs of the single-matrix k_chol_level launches (passed by value)
    std::map<const double *, std::pair<double *, double *>> s_inv;   // factor L_j of S -> its inverted diagonal blocks and their scratch (shared by the solve plans)
    std::vector<std::pair<i64, double *>> trsm_y_pool;               // scratch copies of the right-hand sides of plan_trsm_blockinv, by job position: the plans of a
                                                                    // context run one after the other on one stream, so the forward and the backward solve of a triangle share them
    bool s_inv_valid = false;                      // ... formed since the last factorisation (eager mode skips forming them again)
    std::vector<CholAugDesc> chol_aug;             // augmented factorisations [S; B^T] (k_chol_pack / k_chol_unpack, passed by value)
    double *d_Xc = nullptr, *d_Y = nullptr;        // inputs (xy layout)
    double *d_static = nullptr, *d_work = nullptr; // [Vexp | Astack] and [Z | W] (identical layouts: one memcpy)
    i64 solve_arena_len = 0;
    double *d_TY = nullptr, *d_G = nullptr, *d_TT = nullptr, *d_Sd = nullptr;
    double *d_S = nullptr, *d_B = nullptr, *d_LB = nullptr, *d_Q = nullptr;
    double *d_t = nullptr, *d_u = nullptr, *d_dy = nullptr, *d_rhsy = nullptr, *d_dx = nullptr, *d_rhsx = nullptr;
    double *d_AY = nullptr;
    i64 *d_ayidx = nullptr;
    int *d_info = nullptr;
    double *d_X = nullptr;  // scratch for clrs_cholesky_blocks
    Plan p_assemble, p_cholS, p_linvB, p_Q, p_cholQ, p_fwd, p_bwd, p_cholX;
    FTables ftables = {};
    W3Tables w3tables = {};
    W4Tables w4tables = {};
    W5Tables w5tables = {};
    CSolve8 solve8 = {};          // host copy of the (<= 8) CSolve descriptors: kernel argument of k_solve_small2
    struct SolveSmall2 {          // its staging job table, per phase: 0 = whole stage, 1 / 2 = before / after the exchange of u (sharded path)
        StageJobs jobs = {};
        int rx_job[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ry_job[2] = {-1, -1};     // [first, end) job ranges of rhs_x[j] / rhs_y
        bool ok = false;
    } ss2[3];
    Plan p_fwd_small, p_bwd_small;     // one-launch forms of p_fwd / p_bwd (k_solve_small2, phases 1 and 2)
    Plan p_factor_small;               // k_factor_small: the whole of clrs_schur_factor in one launch
    FSmallArgs fsmall = {};
    StageJobs fsmall_jobs = {};
    // caller-provided device pointers of the current call, read by the fused kernels at launch (no staging copies)
    const double *bind_X = nullptr, *bind_rhsx = nullptr, *bind_rhsy = nullptr;
    double *bind_Xchol = nullptr, *bind_dx = nullptr, *bind_dy = nullptr;
    double *d_dinvS = nullptr, *d_dinvQ = nullptr, *d_Qslabs = nullptr;
    bool q_slabs = false;     // k_cluster_factor leaves per-cluster partial Q slabs
    Plan p_cholQ_slabs, p_solve_all;
    bool fused_fs = false, fused_q = false, fused_x = false, all_assemble_fused = false;
    bool factored = false, assembled = false, local_factored = false;
    bool timing = false, graph_mode = false;
    hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double times[6] = {0, 0, 0, 0, 0, 0};
    bool times_pending = false, solve_time_pending = false;
    double cnt_bytes = 0, cnt_flops = 0, cnt_factor_flops = 0, cnt_solve_flops = 0;
    std::vector<char> cluster_fused;         // per cluster: assembled by the fused kernel
    int n_fused_clusters = 0, n_wave_clusters = 0, n_wave2_clusters = 0, n_wave4_clusters = 0, n_wave5_clusters = 0;
    std::vector<int> host_UR, host_UL;       // flattened per (block, r) for clrs_get_unique_counts
    std::vector<i64> host_U_off;
};

template <class T>
static int upload(clrs_ctx *c, const std::vector<T> &h, T **d) {
    *d = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    HIPCHECK(hipMalloc((void **)d, bytes));
    c->allocs.push_back(*d);
    if (!h.empty()) HIPCHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
static int dmalloc(clrs_ctx *c, double **d, i64 n) {
    size_t bytes = (size_t)std::max<i64>(n, 1) * sizeof(double);
    HIPCHECK(hipMalloc((void **)d, bytes));
    c->allocs.push_back(*d);
    HIPCHECK(hipMemset(*d, 0, bytes));
    return 0;
}

// ---- stage builders -----------------------------------------------------------------------------
// 128 x 128 or 64 x 64 tiles for one product: whichever finishes its last round of workgroups first, in units of one 64 x 64 tile on a
// CU of its own (scripts/gemm_probe.py).  Small tiles: 1024 resident (four per CU), the matrix pipe at 0.63 of its peak; a tile on
// the edge of C skips the MFMAs outside C and, dispatched first, hides behind the whole tiles on its CU (about 0.3 of a tile).
// Large tiles: 512 resident (two per CU, four units each) at 0.72, a lone one on a CU at 0.60; an edge tile is bound by the latency
// of its loads and takes as long as a whole one.  4096 x 4096: two rounds of large tiles; 4097 x 4097 (1089 large tiles: a third
// round) and 2049 x 2049 (289: 33 CUs with two) are faster with small ones.
static bool gemm_prefers_large_tiles(const GemmDesc &d) {
    if (d.M < 256 || d.N < 256) return false;
    const long long batch = std::max(1, d.pad0);
    auto count = [&](long long tm, long long tn) { return (d.lower_only ? tm * (tn + 1) / 2 : tm * tn) * batch; };
    const long long all64 = count((d.M + 63) / 64, (d.N + 63) / 64), full64 = count(d.M / 64, d.N / 64), all128 = count((d.M + 127) / 128, (d.N + 127) / 128);
    const double small = ((double)((full64 + 1023) / 1024) * 4.0 + 0.3 * 4.0 * (double)(all64 - full64) / 1024.0) / 0.63;
    const double large = all128 > 256 ? (double)((all128 + 511) / 512) * 8.0 / 0.72 : 4.0 / 0.60;
    return large < small;
}
static int add_gemm_stage(clrs_ctx *c, Plan &pl, const std::vector<GemmDesc> &descs) {
    // tile size per product: gemm_prefers_large_tiles
    for (int var = 11; var >= 0; var--) {                      // one launch per (tile size / offset width, transposes): template parameters of the kernel
        const int cls = var >> 2, vta = (var >> 1) & 1, vtb = var & 1;          // class 0: 64 x 64 tiles, 1: 128 x 128, 2: 64 x 64 with 64-bit offsets
        const int big = cls == 1;
        const int BM = big ? 128 : GEMM_BM, BN = big ? 128 : GEMM_BN;
        std::vector<GemmDesc> ds;
        std::vector<GemmTile> tiles;
        for (const GemmDesc &d : descs) {
            if (d.M <= 0 || d.N <= 0) continue;
            // the kernel addresses a tile's operands by 32-bit byte offsets from the tile's origin (gemm_offsets_reach): a product whose
            // leading dimensions are beyond the reach of the large tile takes the small one, beyond that the 64-bit instantiation
            int want = gemm_prefers_large_tiles(d) ? 1 : 0;
            if (want == 1 && !gemm_offsets_reach(d, 128)) want = 0;
            if (want == 0 && !gemm_offsets_reach(d, 64)) want = 2;
            if (want != cls || (d.ta != 0) != (vta == 1) || (d.tb != 0) != (vtb == 1)) continue;
            int id = (int)ds.size();
            ds.push_back(d);
            int tm = (d.M + BM - 1) / BM, tn = (d.N + BN - 1) / BN;
            int batch = std::max(1, d.pad0);   // batch count is encoded by the caller through pad0 (>=1)
            // tiles on the edge of C first: they skip most of their MFMAs and are bound by the latency of their loads, which costs nothing
            // while whole tiles share their CUs -- and a full tile's time at the tail of the launch when they come last
            const bool ragged_m = d.M % BM != 0, ragged_n = d.N % BN != 0;
            for (int edge = 1; edge >= 0; edge--)
                for (int b = 0; b < batch; b++)
                    for (int j = 0; j < tn; j++)
                        for (int i = 0; i < tm; i++) {
                            if (d.lower_only && (i + 1) * BM <= j * BN) continue;
                            const bool is_edge = (ragged_m && i == tm - 1) || (ragged_n && j == tn - 1);
                            if (is_edge == (edge == 1)) tiles.push_back(GemmTile{id, b, i, j});
                        }
        }
        if (tiles.empty()) continue;
        Step s;
        s.kind = STEP_GEMM;
        s.grid = (int)tiles.size();
        s.nmax = cls; s.aux0 = vta * 2 + vtb;
        GemmDesc *dd; GemmTile *dt;
        int rc;
        if ((rc = upload(c, ds, &dd))) return rc;
        if ((rc = upload(c, tiles, &dt))) return rc;
        s.d0 = dd; s.d1 = dt;
        pl.steps.push_back(s);
    }
    return 0;
}

static GemmDesc mk_gemm(int ta, int tb, int M, int N, int K, double alpha, const double *A, int lda, const double *B, int ldb,
                        double beta, double *C, int ldc, int batch = 1, i64 sA = 0, i64 sB = 0, i64 sC = 0, int lower_only = 0) {
    GemmDesc d;
    d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K; d.lda = lda; d.ldb = ldb; d.ldc = ldc;
    d.ta = ta; d.tb = tb; d.lower_only = lower_only; d.pad0 = batch; d.alpha = alpha; d.beta = beta;
    d.sA = sA; d.sB = sB; d.sC = sC;
    return d;
}

static int add_trsm_stage(clrs_ctx *c, Plan &pl, const std::vector<TrsmDesc> &descs) {
    std::vector<TrsmDesc> ds;
    std::vector<TrsmWork> work;
    for (const TrsmDesc &d : descs) {
        if (d.n <= 0 || d.nvec <= 0) continue;
        int id = (int)ds.size();
        ds.push_back(d);
        for (int ch = 0; ch * 64 < d.nvec; ch++) work.push_back(TrsmWork{id, ch});
    }
    if (work.empty()) return 0;
    Step s;
    s.kind = STEP_TRSM;
    s.grid = (int)work.size();
    TrsmDesc *dd; TrsmWork *dw;
    int rc;
    if ((rc = upload(c, ds, &dd))) return rc;
    if ((rc = upload(c, work, &dw))) return rc;
    s.d0 = dd; s.d1 = dw;
    pl.steps.push_back(s);
    return 0;
}

// Large triangles (n > TRSM_IB): the same solves through explicit inverses of the TRSM_IB x TRSM_IB diagonal blocks of L.
//   1. every 64 x 64 leaf of L inverted, all leaves of all problems in one launch (k_trtri_diag);
//   2. pairs of inverses joined, log2(TRSM_IB / 64) levels of two GEMM stages:  T = B A^-1,  off-diagonal block = -C^-1 T;
//   3. per TRSM_IB rows:  Y_k = op(Inv_k) B_k  (into a scratch copy of B),  B_rest -= op(L_rest,k) Y_k;  then Y copied back over B.
// n / TRSM_IB levels of two launches instead of n / 64: the level-synchronous chain of plan_trsm_chain is what bounds the staged regime
// (profiles/r02/g_staged_polyopt2048*), not its flops.  The products with the triangular inverse blocks run as full GEMMs
// (2 TRSM_IB n nrhs flops on top of the n^2 nrhs of the substitution).
// share: the triangles are the factors of S, solved with several times per factorisation -- their inverse blocks live in the context
// (one buffer per factor for all the solve plans) and the steps that form them are marked, so that only the first solve after a
// factorisation runs them.
static int plan_trsm_blockinv(clrs_ctx *c, Plan &pl, const std::vector<TrsmJob> &jobs, int trans, bool share) {
    constexpr int IB = TRSM_IB;
    int rc, maxob = 0;
    struct Aux { double *inv, *T, *Y; int nob; };
    std::vector<Aux> aux(jobs.size());
    std::vector<TrtriDesc> leaves;
    for (size_t q = 0; q < jobs.size(); q++) {
        const TrsmJob &j = jobs[q];
        Aux &a = aux[q];
        a.nob = (j.n + IB - 1) / IB;
        maxob = std::max(maxob, a.nob);
        auto hit = share ? c->s_inv.find(j.L) : c->s_inv.end();
        if (hit != c->s_inv.end()) { a.inv = hit->second.first; a.T = hit->second.second; }
        else {
            if ((rc = dmalloc(c, &a.inv, (i64)a.nob * IB * IB))) return rc;      // zeroed: the strict upper triangles stay zero
            if ((rc = dmalloc(c, &a.T, (i64)j.n * (IB / 2)))) return rc;
            if (share) c->s_inv[j.L] = {a.inv, a.T};
        }
        {   // the q-th job of every plan uses the q-th scratch of the context (jobs of ONE plan run side by side and need one each)
            const i64 need = (i64)j.n * j.nrhs;
            if (c->trsm_y_pool.size() <= q) c->trsm_y_pool.resize(q + 1, {0, nullptr});
            if (c->trsm_y_pool[q].first < need) {
                if ((rc = dmalloc(c, &c->trsm_y_pool[q].second, need))) return rc;
                c->trsm_y_pool[q].first = need;
            }
            a.Y = c->trsm_y_pool[q].second;
        }
        for (int o = 0; o < a.nob; o++) {
            const int r0 = o * IB, nb = std::min(IB, j.n - r0);
            for (int l0 = 0; l0 < nb; l0 += TRSM_NB) {
                TrtriDesc d;
                d.L = j.L + (r0 + l0) + (i64)(r0 + l0) * j.ldl; d.ldl = j.ldl; d.n = std::min(TRSM_NB, nb - l0); d.pad = 0;
                d.out = a.inv + (i64)o * IB * IB + l0 + (i64)l0 * IB; d.ldo = IB;
                leaves.push_back(d);
            }
        }
    }
    {
        Step s;
        s.kind = STEP_TRTRI_DIAG; s.grid = (int)leaves.size();
        TrtriDesc *dl;
        if ((rc = upload(c, leaves, &dl))) return rc;
        s.d0 = dl; s.s_inverse = share;
        pl.steps.push_back(s);
        HIPCHECK(hipFuncSetAttribute((const void *)k_trtri_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)trtri_diag_lds_bytes()));
    }
    for (int b = TRSM_NB; b < IB; b *= 2) {
        std::vector<GemmDesc> ga, gb;
        for (size_t q = 0; q < jobs.size(); q++) {
            const TrsmJob &j = jobs[q];
            const Aux &a = aux[q];
            i64 toff = 0;
            for (int o = 0; o < a.nob; o++) {
                const int r0 = o * IB, nb = std::min(IB, j.n - r0);
                double *inv = a.inv + (i64)o * IB * IB;
                for (int lo = 0; lo + b < nb; lo += 2 * b) {
                    const int mid = lo + b, hi = std::min(lo + 2 * b, nb), rows = hi - mid;
                    double *T = a.T + toff;
                    toff += (i64)rows * b;
                    ga.push_back(mk_gemm(0, 0, rows, b, b, 1.0, j.L + (r0 + mid) + (i64)(r0 + lo) * j.ldl, j.ldl, inv + lo + (i64)lo * IB, IB, 0.0, T, rows));
                    gb.push_back(mk_gemm(0, 0, rows, b, rows, -1.0, inv + mid + (i64)mid * IB, IB, T, rows, 0.0, inv + mid + (i64)lo * IB, IB));
                }
            }
        }
        const size_t first = pl.steps.size();
        if ((rc = add_gemm_stage(c, pl, ga))) return rc;
        if ((rc = add_gemm_stage(c, pl, gb))) return rc;
        for (size_t i = first; i < pl.steps.size(); i++) pl.steps[i].s_inverse = share;
    }
    for (int step = 0; step < maxob; step++) {
        std::vector<GemmDesc> gy, gu;
        for (size_t q = 0; q < jobs.size(); q++) {
            const TrsmJob &j = jobs[q];
            const Aux &a = aux[q];
            if (step >= a.nob) continue;
            const int k = trans ? a.nob - 1 - step : step, r0 = k * IB, nk = std::min(IB, j.n - r0);
            const double *inv = a.inv + (i64)k * IB * IB;
            gy.push_back(mk_gemm(trans ? 1 : 0, 0, nk, j.nrhs, nk, 1.0, inv, IB, j.B + r0, j.ldb, 0.0, a.Y + r0, j.n));
            if (!trans) {
                const int rem = j.n - (r0 + nk);
                if (rem > 0) gu.push_back(mk_gemm(0, 0, rem, j.nrhs, nk, -1.0, j.L + (r0 + nk) + (i64)r0 * j.ldl, j.ldl, a.Y + r0, j.n, 1.0, j.B + r0 + nk, j.ldb));
            } else if (r0 > 0)
                gu.push_back(mk_gemm(1, 0, r0, j.nrhs, nk, -1.0, j.L + r0, j.ldl, a.Y + r0, j.n, 1.0, j.B, j.ldb));
        }
        if ((rc = add_gemm_stage(c, pl, gy))) return rc;
        if ((rc = add_gemm_stage(c, pl, gu))) return rc;
    }
    std::vector<Copy2dDesc> cp;
    i64 most = 0;
    for (size_t q = 0; q < jobs.size(); q++) {
        const TrsmJob &j = jobs[q];
        cp.push_back(Copy2dDesc{aux[q].Y, j.B, j.n, j.ldb, j.n, j.nrhs});
        most = std::max(most, (i64)j.n * j.nrhs);
    }
    Step s;
    s.kind = STEP_COPY2D; s.grid = (int)cp.size(); s.aux0 = (int)std::min<i64>((most + 1023) / 1024, 4096);
    Copy2dDesc *dc;
    if ((rc = upload(c, cp, &dc))) return rc;
    s.d0 = dc;
    pl.steps.push_back(s);
    return 0;
}

// B <- L^-1 B (trans = 0) or L^-T B (trans = 1) for a list of independent problems, blocked by
// TRSM_NB, level-synchronous over the problems.
static int plan_trsm_chain(clrs_ctx *c, Plan &pl, const std::vector<TrsmJob> &jobs, int trans);
static int plan_trsm(clrs_ctx *c, Plan &pl, const std::vector<TrsmJob> &jobs, int trans, bool factors_of_S = false) {
    std::vector<TrsmJob> chain, big;
    for (const TrsmJob &j : jobs) {
        if (j.n <= 0 || j.nrhs <= 0) continue;
        const bool inv = g_cfg_trsm_blockinv && j.n > TRSM_IB && (i64)j.n * j.nrhs <= (i64)1 << 31;       // scratch copy of B: 16 GB at most
        (inv ? big : chain).push_back(j);
    }
    int rc;
    if (!chain.empty() && (rc = plan_trsm_chain(c, pl, chain, trans))) return rc;
    if (!big.empty() && (rc = plan_trsm_blockinv(c, pl, big, trans, factors_of_S))) return rc;
    return 0;
}
static int plan_trsm_chain(clrs_ctx *c, Plan &pl, const std::vector<TrsmJob> &jobs, int trans) {
    int maxp = 0;
    for (const TrsmJob &j : jobs) maxp = std::max(maxp, (j.n + TRSM_NB - 1) / TRSM_NB);
    int rc;
    for (int step = 0; step < maxp; step++) {
        std::vector<TrsmDesc> td;
        std::vector<GemmDesc> gd;
        for (const TrsmJob &j : jobs) {
            if (j.n <= 0 || j.nrhs <= 0) continue;
            int np = (j.n + TRSM_NB - 1) / TRSM_NB;
            if (step >= np) continue;
            int k = trans ? np - 1 - step : step;
            int r0 = k * TRSM_NB, nk = std::min(TRSM_NB, j.n - r0);
            TrsmDesc d;
            d.L = j.L + r0 + (i64)r0 * j.ldl; d.ldl = j.ldl; d.n = nk; d.B = j.B + r0; d.nvec = j.nrhs; d.trans = trans;
            d.es = 1; d.vs = j.ldb;
            td.push_back(d);
            if (!trans) {
                int rem = j.n - (r0 + nk);
                if (rem > 0)  // B[r0+nk:, :] -= L[r0+nk:, r0:r0+nk] B[r0:r0+nk, :]
                    gd.push_back(mk_gemm(0, 0, rem, j.nrhs, nk, -1.0, j.L + (r0 + nk) + (i64)r0 * j.ldl, j.ldl, j.B + r0, j.ldb, 1.0,
                                         j.B + r0 + nk, j.ldb));
            } else {
                if (r0 > 0)  // B[0:r0, :] -= L[r0:r0+nk, 0:r0]^T B[r0:r0+nk, :]
                    gd.push_back(mk_gemm(1, 0, r0, j.nrhs, nk, -1.0, j.L + r0, j.ldl, j.B + r0, j.ldb, 1.0, j.B, j.ldb));
            }
        }
        if ((rc = add_trsm_stage(c, pl, td))) return rc;
        if ((rc = add_gemm_stage(c, pl, gd))) return rc;
    }
    return 0;
}

// Matrices beyond one block: one launch per block column (k_chol_level) instead of the three of plan_potrf_chain, then the diagonal
// factors copied from their side buffer into the matrices.
static int plan_potrf_levels(clrs_ctx *c, Plan &pl, const std::vector<PotrfJob> &jobs, int *info) {
    int rc, maxp = 0;
    std::vector<double *> dbuf(jobs.size());
    auto stop_of = [](const PotrfJob &j) { const int np = (j.n + 63) / 64; return j.stop > 0 ? std::min(j.stop, np) : np; };
    for (size_t q = 0; q < jobs.size(); q++) {
        const int np = (jobs[q].n + 63) / 64;
        maxp = std::max(maxp, np);
        if ((rc = dmalloc(c, &dbuf[q], (i64)np * 4096))) return rc;
    }
    HIPCHECK(hipFuncSetAttribute((const void *)k_chol_level, hipFuncAttributeMaxDynamicSharedMemorySize, (int)chol_level_lds_bytes()));
    // launch lvl: block column lvl final; column workgroups for block column lvl + 1 (while it is to be factored), trailing tiles beyond
    for (int lvl = -1; lvl <= maxp - 2; lvl++) {
        std::vector<CholLevelJob> cj;
        std::vector<CholLevelWork> col, bulk;
        for (size_t q = 0; q < jobs.size(); q++) {
            const PotrfJob &j = jobs[q];
            const int np = (j.n + 63) / 64, cb = lvl + 1, stop = stop_of(j);
            if (cb >= np || cb > stop) continue;
            const bool closing = cb == stop;                       // nothing left to factor: the trailing update of block column lvl alone
            const int id = (int)cj.size(), bulk0 = closing ? cb : cb + 1;
            cj.push_back(CholLevelJob{j.A, dbuf[q], j.lda, j.n, lvl, j.code, bulk0, 0});
            if (!closing)
                for (int i = cb; i < np; i++) col.push_back(CholLevelWork{id, 0, i, 0});
            const int rb = bulk0 * 64;
            if (lvl >= 0 && rb < j.n) {
                const int nt = (j.n - rb + 127) / 128;
                for (int tj = 0; tj < nt; tj++)
                    for (int ti = tj; ti < nt; ti++) bulk.push_back(CholLevelWork{id, 1, ti, tj});
            }
        }
        if (col.empty() && bulk.empty()) continue;
        const int ncol = (int)col.size();
        col.insert(col.end(), bulk.begin(), bulk.end());       // the column workgroups (the critical path) are dispatched first
        Step s;
        s.kind = STEP_CHOL_LEVEL; s.grid = (int)col.size(); s.dst = info ? info : c->d_info;
        if (cj.size() == 1) {                                  // the kernel derives the same order from blockIdx.x
            c->chol_jobs.push_back(cj[0]);
            s.aux1 = 1; s.aux0 = ncol; s.n = (i64)c->chol_jobs.size() - 1;
        } else {
            CholLevelJob *dj; CholLevelWork *dw;
            if ((rc = upload(c, cj, &dj))) return rc;
            if ((rc = upload(c, col, &dw))) return rc;
            s.d0 = dj; s.d1 = dw;
        }
        pl.steps.push_back(s);
    }
    std::vector<Copy2dDesc> cp;
    for (size_t q = 0; q < jobs.size(); q++) {
        const PotrfJob &j = jobs[q];
        const int stop = stop_of(j);
        for (int r0 = 0, b = 0; r0 < j.n && b < stop; r0 += 64, b++) {
            const int m = std::min(64, j.n - r0);
            cp.push_back(Copy2dDesc{dbuf[q] + (i64)b * 4096, j.A + r0 + (i64)r0 * j.lda, 64, j.lda, m, m});
        }
    }
    Step s;
    s.kind = STEP_COPY2D; s.grid = (int)cp.size(); s.aux0 = 4;
    Copy2dDesc *dc;
    if ((rc = upload(c, cp, &dc))) return rc;
    s.d0 = dc;
    pl.steps.push_back(s);
    return 0;
}

// in-place lower Cholesky of a list of independent matrices, blocked by POTRF_NB, level-synchronous.
static int plan_potrf_chain(clrs_ctx *c, Plan &pl, const std::vector<PotrfJob> &jobs, int *info);
static int plan_potrf(clrs_ctx *c, Plan &pl, const std::vector<PotrfJob> &jobs, int *info = nullptr) {
    std::vector<PotrfJob> chain, big;
    for (const PotrfJob &j : jobs) ((g_cfg_potrf_levels && j.n > POTRF_NB) ? big : chain).push_back(j);
    int rc;
    if (!chain.empty() && (rc = plan_potrf_chain(c, pl, chain, info))) return rc;
    if (!big.empty() && (rc = plan_potrf_levels(c, pl, big, info))) return rc;
    return 0;
}
static int plan_potrf_chain(clrs_ctx *c, Plan &pl, const std::vector<PotrfJob> &jobs, int *info) {
    int maxp = 0;
    for (const PotrfJob &j : jobs) maxp = std::max(maxp, (j.n + POTRF_NB - 1) / POTRF_NB);
    int rc;
    for (int k = 0; k < maxp; k++) {
        std::vector<PotrfDesc> pd;
        std::vector<TrsmDesc> td;
        std::vector<GemmDesc> gd;
        for (const PotrfJob &j : jobs) {
            int r0 = k * POTRF_NB;
            if (r0 >= j.n) continue;
            int nk = std::min(POTRF_NB, j.n - r0), rem = j.n - r0 - nk;
            double *Akk = j.A + r0 + (i64)r0 * j.lda;
            pd.push_back(PotrfDesc{Akk, j.lda, nk, j.code, 0});
            if (rem > 0) {
                double *Pn = j.A + (r0 + nk) + (i64)r0 * j.lda;  // panel below the diagonal block
                TrsmDesc d;                                       // rows of the panel: x L_kk^T = b
                d.L = Akk; d.ldl = j.lda; d.n = nk; d.B = Pn; d.nvec = rem; d.trans = 0; d.es = j.lda; d.vs = 1;
                td.push_back(d);
                double *A22 = j.A + (r0 + nk) + (i64)(r0 + nk) * j.lda;
                gd.push_back(mk_gemm(0, 1, rem, rem, nk, -1.0, Pn, j.lda, Pn, j.lda, 1.0, A22, j.lda, 1, 0, 0, 0, 1));
            }
        }
        if (pd.empty()) continue;
        Step s;
        s.kind = STEP_POTRF;
        s.grid = (int)pd.size();
        s.dst = info ? info : c->d_info;
        PotrfDesc *dd;
        if ((rc = upload(c, pd, &dd))) return rc;
        s.d0 = dd;
        pl.steps.push_back(s);
        if ((rc = add_trsm_stage(c, pl, td))) return rc;
        if ((rc = add_gemm_stage(c, pl, gd))) return rc;
    }
    return 0;
}

static void add_memcpy(Plan &pl, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return;
    Step s;
    s.kind = STEP_MEMCPY;
    s.dst = dst; s.src = src; s.bytes = bytes;
    pl.steps.push_back(s);
}

// ---- plan execution -----------------------------------------------------------------------------
static int run_steps(clrs_ctx *c, const Plan &pl) {
    hipStream_t st = c->stream;
    for (const Step &s : pl.steps) {
        if (s.s_inverse && c->s_inv_valid && !c->graph_mode) continue;       // (a captured graph replays all of its steps)
        const bool timed = !c->graph_mode && (c->kt_kind == -1 || c->kt_kind == (int)s.kind) && (int)c->kt_kinds.size() < KT_MAX_EVENTS;
        if (timed) {
            const size_t need = 2 * (c->kt_kinds.size() + 1);
            while (c->kt_ev.size() < need) {
                hipEvent_t e;
                HIPCHECK(hipEventCreate(&e));
                c->kt_ev.push_back(e);
            }
            HIPCHECK(hipEventRecord(c->kt_ev[need - 2], st));
        }
        switch (s.kind) {
            case STEP_MEMCPY:
                HIPCHECK(hipMemcpyAsync(s.dst, s.src, s.bytes, hipMemcpyDeviceToDevice, st));
                break;
            case STEP_GEMM:
#define CLRS_GEMM_LAUNCH(BMN, TA, TB) \
    hipLaunchKernelGGL((k_gemm_f64_t<BMN, BMN, TA, TB>), dim3(s.grid), dim3(256), gemm_lds_bytes(BMN, BMN), st, (const GemmDesc *)s.d0, (const GemmTile *)s.d1)
#define CLRS_GEMM_LAUNCH_WIDE(TA, TB) \
    hipLaunchKernelGGL((k_gemm_f64_t<64, 64, TA, TB, unsigned long long>), dim3(s.grid), dim3(256), gemm_lds_bytes(64, 64), st, (const GemmDesc *)s.d0, (const GemmTile *)s.d1)
                switch (s.nmax * 4 + s.aux0) {
                    case 8: CLRS_GEMM_LAUNCH_WIDE(0, 0); break;
                    case 9: CLRS_GEMM_LAUNCH_WIDE(0, 1); break;
                    case 10: CLRS_GEMM_LAUNCH_WIDE(1, 0); break;
                    case 11: CLRS_GEMM_LAUNCH_WIDE(1, 1); break;
                    case 0: CLRS_GEMM_LAUNCH(64, 0, 0); break;
                    case 1: CLRS_GEMM_LAUNCH(64, 0, 1); break;
                    case 2: CLRS_GEMM_LAUNCH(64, 1, 0); break;
                    case 3: CLRS_GEMM_LAUNCH(64, 1, 1); break;
                    case 4: CLRS_GEMM_LAUNCH(128, 0, 0); break;
                    case 5: CLRS_GEMM_LAUNCH(128, 0, 1); break;
                    case 6: CLRS_GEMM_LAUNCH(128, 1, 0); break;
                    default: CLRS_GEMM_LAUNCH(128, 1, 1); break;
                }
#undef CLRS_GEMM_LAUNCH
#undef CLRS_GEMM_LAUNCH_WIDE
                break;
            case STEP_TRSM:
                hipLaunchKernelGGL(k_trsm_diag, dim3(s.grid), dim3(256), 0, st, (const TrsmDesc *)s.d0, (const TrsmWork *)s.d1);
                break;
            case STEP_POTRF:
                hipLaunchKernelGGL(k_potrf_diag, dim3(s.grid), dim3(256), 0, st, (const PotrfDesc *)s.d0, (int *)s.dst);
                break;
            case STEP_GATHER_S:
                if (s.aux0 >= 4)       // some cluster has four blocks or more: four lanes per entry walk them
                    hipLaunchKernelGGL(k_schur_gather<4>, dim3(s.grid), dim3(1024), 0, st, (const SClusterDesc *)s.d0, (const SBlockDesc *)s.d1, (const STile *)s.d2);
                else
                    hipLaunchKernelGGL(k_schur_gather<1>, dim3(s.grid), dim3(256), 0, st, (const SClusterDesc *)s.d0, (const SBlockDesc *)s.d1, (const STile *)s.d2);
                break;
            case STEP_GATHER_SCALAR:
                hipLaunchKernelGGL(k_gather_scalar, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, st, (double *)s.dst, (const double *)s.src,
                                   (const i64 *)s.d0, s.n);
                break;
            case STEP_SUB:
                hipLaunchKernelGGL(k_sub, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, st, (double *)s.dst, (const double *)s.src,
                                   (const double *)s.d0, (int)s.n);
                break;
            case STEP_MEMSET_INFO:
                HIPCHECK(hipMemsetAsync(s.dst ? s.dst : (void *)c->d_info, 0x7f, sizeof(int), st));
                break;
            case STEP_FUSED_ASSEMBLE:
                hipLaunchKernelGGL(k_cluster_assemble, dim3(s.grid), dim3(256), s.bytes, st, (const FCluster *)s.d0, (const FBlock *)s.d1, *(const FTables *)s.src);
                break;
            case STEP_DENSE_BLOCK:
                hipLaunchKernelGGL(k_dense_block, dim3(s.grid), dim3(256), s.bytes, st, (const DBlock *)s.d0, *(const FTables *)s.src);
                break;
            case STEP_TRTRI32:
                hipLaunchKernelGGL(k_trtri32, dim3(s.grid), dim3(64), 0, st, (const DenseTBlock *)s.d0);
                break;
            case STEP_DENSE_T32:
                hipLaunchKernelGGL(k_dense_T32, dim3(s.grid), dim3(64 * DT32_WAVES), dense_T32_lds_bytes(), st, (const DenseTBlock *)s.d0, (const DenseTPair *)s.d1);
                break;
            case STEP_TRTRI_DIAG:
                hipLaunchKernelGGL(k_trtri_diag, dim3(s.grid), dim3(256), trtri_diag_lds_bytes(), st, (const TrtriDesc *)s.d0);
                break;
            case STEP_CHOL_LEVEL:
                if (s.aux1 == 1) {       // one matrix: job by value (kept in the context), no tables
                    hipLaunchKernelGGL(k_chol_level, dim3(s.grid), dim3(CL_NT), chol_level_lds_bytes(), st, c->chol_jobs[(size_t)s.n], s.aux0,
                                       (const CholLevelJob *)nullptr, (const CholLevelWork *)nullptr, (int *)s.dst);
                } else
                    hipLaunchKernelGGL(k_chol_level, dim3(s.grid), dim3(CL_NT), chol_level_lds_bytes(), st, CholLevelJob{}, 0, (const CholLevelJob *)s.d0,
                                       (const CholLevelWork *)s.d1, (int *)s.dst);
                break;
            case STEP_CHOL_PACK:
                hipLaunchKernelGGL(k_chol_pack, dim3(s.grid), dim3(256), 0, st, c->chol_aug[(size_t)s.n]);
                break;
            case STEP_CHOL_UNPACK:
                hipLaunchKernelGGL(k_chol_unpack, dim3(s.grid), dim3(256), 0, st, c->chol_aug[(size_t)s.n]);
                break;
            case STEP_COPY2D:
                hipLaunchKernelGGL(k_copy2d, dim3(s.aux0, s.grid), dim3(256), 0, st, (const Copy2dDesc *)s.d0);
                break;
            case STEP_SOLVE_SMALL:
                if (s.aux0 >= 2) {
                    const int ph = s.aux0 - 2;
                    clrs_ctx::SolveSmall2 &q = c->ss2[ph];
                    // right-hand sides bound for this call: piece i of a vector starts 16 x (its destination offset - the first piece's) in
                    // (a pure zero-fill piece -- no valid rows -- reads and ignores the first entry)
                    auto piece_off = [&](int t, int first) -> long long {
                        const StageJob &jb = q.jobs.j[t];
                        return ((jb.meta >> 16) & 31) ? (long long)(jb.dst_ldd & 0xffff) - (long long)(q.jobs.j[first].dst_ldd & 0xffff) : 0;
                    };
                    for (int j = 0; j < c->J; j++)
                        for (int t = q.rx_job[j]; t < q.rx_job[8 + j]; t++) q.jobs.j[t].src = c->bind_rhsx + c->solve8.d[j].off + piece_off(t, q.rx_job[j]);
                    for (int t = q.ry_job[0]; t >= 0 && t < q.ry_job[1]; t++) q.jobs.j[t].src = c->bind_rhsy + piece_off(t, q.ry_job[0]);
#define CLRS_SS2(NJ, PH) hipLaunchKernelGGL((k_solve_small2<NJ, PH>), dim3(1), dim3(256), s.bytes, st, c->solve8, q.jobs, c->J, c->N, (int)c->xlen, c->bind_dx, c->bind_dy, c->d_t, c->d_u)
#define CLRS_SS2_NJ(PH)                                  \
    do {                                                 \
        if (q.jobs.n <= 8) CLRS_SS2(8, PH);              \
        else if (q.jobs.n <= 16) CLRS_SS2(16, PH);       \
        else if (q.jobs.n <= 24) CLRS_SS2(24, PH);       \
        else if (q.jobs.n <= 32) CLRS_SS2(32, PH);       \
        else CLRS_SS2(48, PH);                           \
    } while (0)
                    if (ph == 0) CLRS_SS2_NJ(0);
                    else if (ph == 1) CLRS_SS2_NJ(1);
                    else CLRS_SS2_NJ(2);
#undef CLRS_SS2_NJ
#undef CLRS_SS2
                    break;
                }
                hipLaunchKernelGGL(k_solve_small, dim3(1), dim3(256), s.bytes, st, (const CSolve *)s.d0, c->J, (const double *)c->d_Q, (const double *)c->d_dinvQ, c->N,
                                   (int)c->xlen, c->bind_rhsx, c->bind_rhsy, (const double *)c->d_LB, c->bind_dx, c->bind_dy, (int)s.n);
                break;
            case STEP_ASSEMBLE_W2: {
                const FTables *tb = (const FTables *)s.src;
                const int ncl = (int)s.n;
                const bool full = s.grid != 0;      // every low-rank block is exactly 16 x (16 UT)
                if (s.nmax <= 2 && full)
                    hipLaunchKernelGGL((k_cluster_assemble_w2<2, true>), dim3((ncl + 3) / 4), dim3(256), s.bytes, st, (const W2Cluster *)s.d0, (const W2Block *)s.d1, *tb, ncl);
                else if (s.nmax <= 2)
                    hipLaunchKernelGGL((k_cluster_assemble_w2<2, false>), dim3((ncl + 3) / 4), dim3(256), s.bytes, st, (const W2Cluster *)s.d0, (const W2Block *)s.d1, *tb, ncl);
                else
                    hipLaunchKernelGGL((k_cluster_assemble_w2<4, false>), dim3((ncl + 3) / 4), dim3(256), s.bytes, st, (const W2Cluster *)s.d0, (const W2Block *)s.d1, *tb, ncl);
                break;
            }
            case STEP_FACTOR_SMALL: {
#define CLRS_FS(NJ) hipLaunchKernelGGL(k_factor_small<NJ>, dim3(1), dim3(256), s.bytes, st, c->fsmall, c->fsmall_jobs, c->d_info)
                if (c->fsmall_jobs.n <= 8) CLRS_FS(8);
                else if (c->fsmall_jobs.n <= 16) CLRS_FS(16);
                else if (c->fsmall_jobs.n <= 24) CLRS_FS(24);
                else if (c->fsmall_jobs.n <= 32) CLRS_FS(32);
                else CLRS_FS(48);
#undef CLRS_FS
                break;
            }
            case STEP_ASSEMBLE_W3: {
                W3Tables tb = *(const W3Tables *)s.src;
                tb.Xc = c->ftables.Xc; tb.Y = c->ftables.Y;      // the iterates bound for this call (the caller's buffers or the context's)
                if (s.grid != 0)
                    hipLaunchKernelGGL((k_cluster_assemble_w3<true>), dim3(s.aux0), dim3(256), 0, st, (const int *)s.d0, (const W3Block *)s.d1, tb, (int)s.n, s.aux1);
                else
                    hipLaunchKernelGGL((k_cluster_assemble_w3<false>), dim3(s.aux0), dim3(256), 0, st, (const int *)s.d0, (const W3Block *)s.d1, tb, (int)s.n, s.aux1);
                break;
            }
            case STEP_ASSEMBLE_W4: {
                W4Tables tb = *(const W4Tables *)s.src;
                tb.Xc = c->ftables.Xc; tb.Y = c->ftables.Y;      // the iterates bound for this call
                if (s.nmax <= 3)
                    hipLaunchKernelGGL((k_cluster_assemble_w4<3>), dim3(s.aux0), dim3(256), s.bytes, st, (const int *)s.d0, (const W3Block *)s.d1, tb, (int)s.n, s.aux1, s.grid);
                else
                    hipLaunchKernelGGL((k_cluster_assemble_w4<4>), dim3(s.aux0), dim3(256), s.bytes, st, (const int *)s.d0, (const W3Block *)s.d1, tb, (int)s.n, s.aux1, s.grid);
                break;
            }
            case STEP_ASSEMBLE_W5: {
                W5Tables tb = *(const W5Tables *)s.src;
                tb.Xc = c->ftables.Xc; tb.Y = c->ftables.Y;      // the iterates bound for this call
                hipLaunchKernelGGL(k_cluster_assemble_w5, dim3(s.aux0), dim3(256), 0, st, (const int *)s.d0, (const W3Block *)s.d1, tb, (int)s.n, s.aux1);
                break;
            }
            case STEP_ASSEMBLE_W1: {
                const FTables *tb = (const FTables *)s.src;
                const int nw = (int)s.n, mb = (int)(intptr_t)s.dst;
                if (s.nmax <= 2)
                    hipLaunchKernelGGL(k_cluster_assemble_w1<2>, dim3(s.grid), dim3(64 * nw), s.bytes, st, (const WCluster *)s.d0, (const WBlock *)s.d1, *tb, nw, mb);
                else if (s.nmax <= 4)
                    hipLaunchKernelGGL(k_cluster_assemble_w1<4>, dim3(s.grid), dim3(64 * nw), s.bytes, st, (const WCluster *)s.d0, (const WBlock *)s.d1, *tb, nw, mb);
                else
                    hipLaunchKernelGGL(k_cluster_assemble_w1<8>, dim3(s.grid), dim3(64 * nw), s.bytes, st, (const WCluster *)s.d0, (const WBlock *)s.d1, *tb, nw, mb);
                break;
            }
            case STEP_SMALL_POTRF:
                if (s.n == 0)
                    hipLaunchKernelGGL(k_small_potrf, dim3(s.grid), dim3(256), s.bytes, st, (const SmallPotrf *)s.d0, c->bind_X, c->bind_Xchol, (int *)s.dst);
                else if (s.n == 1)
                    hipLaunchKernelGGL(k_small_potrf, dim3(s.grid), dim3(256), s.bytes, st, (const SmallPotrf *)s.d0, (const double *)c->d_Q, c->d_Q, (int *)s.dst);
                else   // Q = sum of the per-cluster slabs, factored in the same launch
                    hipLaunchKernelGGL(k_small_potrf, dim3(s.grid), dim3(256), s.bytes, st, (const SmallPotrf *)s.d0, (const double *)c->d_Qslabs, c->d_Q, (int *)s.dst);
                break;
            case STEP_GRAM_SMALL:
                hipLaunchKernelGGL(k_gram_small, dim3(c->N * c->N), dim3(256), 0, st, (const double *)c->d_LB, (int)c->xlen, (int)c->xlen, c->N, c->d_Q);
                break;
            case STEP_SUM_S_SLABS:
                hipLaunchKernelGGL(k_sum_S_slabs, dim3((unsigned)((s.n + 1023) / 1024), s.grid), dim3(256), 0, st, (const SSlabSum *)s.d0);
                break;
            case STEP_SUM_SLABS:
                hipLaunchKernelGGL(k_sum_slabs, dim3((unsigned)(((i64)c->N * c->N + 255) / 256)), dim3(256), 0, st, (const double *)c->d_Qslabs, (i64)c->N * c->N, c->J,
                                   (i64)c->N * c->N, c->d_Q);
                break;
            case STEP_CLUSTER_FACTOR:
                hipLaunchKernelGGL(k_cluster_factor, dim3(s.grid), dim3(256), s.bytes, st, (const CFactor *)s.d0, (int *)s.dst);
                break;
            case STEP_GEMV_T:
                hipLaunchKernelGGL(k_gemv_t, dim3((c->N + 3) / 4), dim3(256), 0, st, (const double *)c->d_LB, (int)c->xlen, (int)c->xlen, c->N, (const double *)c->d_t, c->d_u);
                break;
            case STEP_CSOLVE_FWD:
                hipLaunchKernelGGL(k_cluster_solve_fwd, dim3(s.grid), dim3(256), s.bytes, st, (const CSolve *)s.d0, c->bind_rhsx, c->d_t);
                break;
            case STEP_Q_SOLVE:
                hipLaunchKernelGGL(k_q_solve, dim3(1), dim3(256), s.bytes, st, (const double *)c->d_Q, (const double *)c->d_dinvQ, c->N, c->bind_rhsy, c->d_u, c->bind_dy,
                                   s.n ? (const double *)c->d_LB : (const double *)nullptr, (int)c->xlen, (int)c->xlen, (const double *)c->d_t);
                break;
            case STEP_CSOLVE_BWD:
                hipLaunchKernelGGL(k_cluster_solve_bwd, dim3(s.grid), dim3(256), s.bytes, st, (const CSolve *)s.d0, (const double *)c->bind_dy, (const double *)c->d_t, c->bind_dx);
                break;
            case STEP_ZERO_UPPER:
                hipLaunchKernelGGL(k_zero_upper, dim3((unsigned)((s.n + 255) / 256), (unsigned)s.grid), dim3(256), 0, st, (const PotrfDesc *)s.d0);
                break;
            default:
                break;
        }
        if (timed) {
            HIPCHECK(hipEventRecord(c->kt_ev[2 * c->kt_kinds.size() + 1], st));
            c->kt_kinds.push_back((int)s.kind);
        }
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

static int run_plan(clrs_ctx *c, Plan &pl) {
    if (pl.steps.empty()) return 0;
    if (!c->graph_mode) return run_steps(c, pl);
    if (!c->stream) return fail(CLRS_ERR_STATE, "graph mode cannot capture the default (null) stream: pass a stream of its own to clrs_set_stream");
    const void *now[8] = {c->bind_X, c->bind_Xchol, c->bind_rhsx, c->bind_rhsy, c->bind_dx, c->bind_dy, c->ftables.Xc, c->ftables.Y};
    if (pl.graph && std::memcmp(now, pl.captured, sizeof(now)) != 0) {   // the graph bakes the caller's pointers: re-capture
        hipGraphExecDestroy(pl.graph);
        pl.graph = nullptr;
    }
    if (!pl.graph) {
        std::memcpy(pl.captured, now, sizeof(now));
        hipGraph_t g;
        HIPCHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        int rc = run_steps(c, pl);
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc) return rc;
        if (e != hipSuccess) return fail(CLRS_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        HIPCHECK(hipGraphInstantiate(&pl.graph, g, nullptr, nullptr, 0));
        HIPCHECK(hipGraphDestroy(g));
    }
    HIPCHECK(hipGraphLaunch(pl.graph, c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// context creation
// ------------------------------------------------------------------------------------------------
static bool vec_eq(const double *a, const double *b, int n) {   // exact equality, like the reference's == (src/tools.jl:134)
    for (int i = 0; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

#include "clrs_ctx_create.inc"

typedef std::unique_ptr<clrs_ctx, void (*)(clrs_ctx *)> CtxOwner;   // destroys the context it still holds: the one failure path of whoever creates one

extern "C" int clrs_ctx_create(const clrs_sdp_desc *d, int device, clrs_ctx **out) {
    if (!d || !out) return fail(CLRS_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(CLRS_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(CLRS_ERR_NO_DEVICE, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    CtxOwner c(new clrs_ctx(), clrs_ctx_destroy);      // whatever a failed stage left behind goes with the context
    c->device = device;
    CtxBuild build;
    for (CtxStage stage : CTX_STAGES)
        if (int rc = stage(c.get(), d, build)) return rc;
    HIPCHECK(hipStreamSynchronize(c->stream));
    *out = c.release();
    return 0;
}

static void ipm_free(clrs_ctx *c);

extern "C" void clrs_ctx_destroy(clrs_ctx *c) {
    if (!c) return;
    ipm_free(c);
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    Plan *plans[] = {&c->p_assemble, &c->p_cholS, &c->p_linvB, &c->p_Q, &c->p_cholQ, &c->p_fwd, &c->p_bwd, &c->p_cholX, &c->p_cholQ_slabs, &c->p_solve_all, &c->p_fwd_small, &c->p_bwd_small, &c->p_factor_small};
    for (Plan *p : plans)
        if (p->graph) hipGraphExecDestroy(p->graph);
    for (void *p : c->allocs) hipFree(p);
    for (int i = 0; i < 10; i++)
        if (c->ev[i]) hipEventDestroy(c->ev[i]);
    for (hipEvent_t e : c->kt_ev) hipEventDestroy(e);
    if (c->h_info) (void)hipHostFree(c->h_info);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->stream && c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int clrs_get_dims(const clrs_ctx *c, clrs_dims *o) {
    if (!c || !o) return fail(CLRS_ERR_INVALID, "null argument");
    o->xy_len = c->xylen; o->x_len = c->xlen; o->S_len = c->Slen; o->n_terms = c->T; o->n_free = c->N;
    o->n_clusters = c->J; o->n_blocks = c->NB; o->reserved = 0;
    return 0;
}

extern "C" int clrs_get_unique_counts(const clrs_ctx *c, int32_t b, int32_t r, int32_t *nr, int32_t *nl) {
    if (!c || b < 0 || b >= c->NB) return fail(CLRS_ERR_INVALID, "block out of range");
    const BlockInfo &k = c->blk[b];
    if (k.kind != 0 || r < 0 || r >= k.m) return fail(CLRS_ERR_INVALID, "not a low-rank sub-block row");
    if (nr) *nr = k.UR[r];
    if (nl) *nl = k.UL[r];
    return 0;
}

// ------------------------------------------------------------------------------------------------
// per-iteration drivers
// ------------------------------------------------------------------------------------------------
static size_t PIN_LIMIT = (size_t)64 << 20;            // beyond this the caller's buffers are copied directly (bandwidth, not latency, matters there); "pin_limit" (tests)
// start of a host-pointer call: the arena is empty again; it grows here (never while pointers are handed out) to what the
// previous call asked for in total
static void pin_reset(clrs_ctx *c) {
    c->pin_used = 0;
    c->pin_out.clear();
    if (c->pin_demand > c->pin_cap && c->pin_demand <= PIN_LIMIT) {
        const size_t cap = std::min(PIN_LIMIT, std::max<size_t>((size_t)1 << 20, 2 * c->pin_demand));
        if (c->pin) { (void)hipHostFree(c->pin); c->pin = nullptr; c->pin_cap = 0; }
        if (hipHostMalloc((void **)&c->pin, cap, hipHostMallocDefault) == hipSuccess) c->pin_cap = cap;
        else c->pin = nullptr;
    }
    c->pin_demand = 0;
}
static void *pin_take(clrs_ctx *c, size_t bytes) {
    bytes = (bytes + 63) & ~(size_t)63;
    c->pin_demand += bytes;
    if (c->pin_used + bytes > c->pin_cap) return nullptr;      // the caller copies directly; the next call finds a larger arena
    void *p = c->pin + c->pin_used;
    c->pin_used += bytes;
    return p;
}
// host -> device through the arena (falls back to the direct copy when the arena cannot hold it)
static int h2d_staged(clrs_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return 0;
    void *p = pin_take(c, bytes);
    if (p) { std::memcpy(p, src, bytes); src = p; }
    HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}
// device -> host: lands in the arena, handed to the caller by d2h_finish after the stream has been synchronised
static int d2h_staged(clrs_ctx *c, void *user, const void *src, size_t bytes) {
    if (bytes == 0) return 0;
    void *p = pin_take(c, bytes);
    HIPCHECK(hipMemcpyAsync(p ? p : user, src, bytes, hipMemcpyDeviceToHost, c->stream));
    if (p) c->pin_out.push_back(clrs_ctx::PinOut{user, p, bytes});
    return 0;
}
static int d2h_finish(clrs_ctx *c) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (const clrs_ctx::PinOut &o : c->pin_out) std::memcpy(o.user, o.pinned, o.bytes);
    c->pin_out.clear();
    return 0;
}

static int read_info(clrs_ctx *c, int *status, int which = 0) {
    if (!c->h_info) HIPCHECK(hipHostMalloc((void **)&c->h_info, 2 * sizeof(int), hipHostMallocDefault));   // pinned: no staging copy behind the 4-byte read
    c->h_info[which] = INFO_NONE;
    HIPCHECK(hipMemcpyAsync(c->h_info + which, c->d_info + which, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    const int h = c->h_info[which];
    *status = (h == INFO_NONE) ? 0 : h;
    if (h != INFO_NONE) HIPCHECK(hipMemsetAsync(c->d_info + which, 0x7f, sizeof(int), c->stream));   // re-arm: the status is "since the last query"
    return 0;
}

static int collect_times(clrs_ctx *c) {
    if (c->times_pending) {
        for (int i = 0; i < 5; i++) {
            float ms = 0;
            int a = (i == 0) ? 0 : i + 1, b = (i == 0) ? 1 : i + 2;   // ev0-1: schur; ev2..7: cholS,LinvB,Q,cholQ boundaries
            if (hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) == hipSuccess) c->times[i] = ms * 1e-3;
        }
        c->times_pending = false;
    }
    if (c->solve_time_pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[7], c->ev[8]) == hipSuccess) c->times[5] = ms * 1e-3;
        c->solve_time_pending = false;
    }
    return 0;
}

extern "C" int clrs_schur_assemble_dev(clrs_ctx *c, const double *d_Xchol, const double *d_Y) {
    if (!c || !d_Xchol || !d_Y) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    if (c->all_assemble_fused) {   // the fused kernel reads the caller's buffers directly
        c->ftables.Xc = d_Xchol; c->ftables.Y = d_Y;
    } else {
        c->ftables.Xc = c->d_Xc; c->ftables.Y = c->d_Y;
        if (d_Xchol != c->d_Xc) HIPCHECK(hipMemcpyAsync(c->d_Xc, d_Xchol, sizeof(double) * c->xylen, hipMemcpyDeviceToDevice, c->stream));
        if (d_Y != c->d_Y) HIPCHECK(hipMemcpyAsync(c->d_Y, d_Y, sizeof(double) * c->xylen, hipMemcpyDeviceToDevice, c->stream));
    }
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[0], c->stream));
    int rc = run_plan(c, c->p_assemble);
    if (rc) return rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[1], c->stream));
    c->assembled = true; c->factored = false; c->local_factored = false; c->s_inv_valid = false;
    return 0;
}

extern "C" int clrs_schur_assemble(clrs_ctx *c, const double *Xchol, const double *Y, double *S_out, double *AY_out) {
    if (!c || !Xchol || !Y) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    pin_reset(c);
    if ((rc = h2d_staged(c, c->d_Xc, Xchol, sizeof(double) * c->xylen))) return rc;
    if ((rc = h2d_staged(c, c->d_Y, Y, sizeof(double) * c->xylen))) return rc;
    if ((rc = clrs_schur_assemble_dev(c, c->d_Xc, c->d_Y))) return rc;
    if (S_out && (rc = d2h_staged(c, S_out, c->d_S, sizeof(double) * c->Slen))) return rc;
    if (AY_out && c->T > 0 && (rc = d2h_staged(c, AY_out, c->d_AY, sizeof(double) * c->T))) return rc;
    return d2h_finish(c);
}

extern "C" int clrs_schur_factor_local_dev(clrs_ctx *c) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->assembled) return fail(CLRS_ERR_STATE, "clrs_schur_factor called before clrs_schur_assemble");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[2], c->stream));
    c->s_inv_valid = false;
    if ((rc = run_plan(c, c->p_cholS))) return rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[3], c->stream));
    if ((rc = run_plan(c, c->p_linvB))) return rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[4], c->stream));
    if ((rc = run_plan(c, c->p_Q))) return rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[5], c->stream));
    c->assembled = false;  // S now holds L
    c->factored = false;
    c->local_factored = true;      // L_j and LinvB_j are ready: clrs_schur_solve_fwd_dev may run before Q is summed and factored
    return 0;
}

extern "C" int clrs_schur_factor_finish_dev(clrs_ctx *c) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    if ((rc = run_plan(c, c->p_cholQ))) return rc;
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[6], c->stream)); c->times_pending = true; }
    c->factored = true;
    return 0;
}

extern "C" int clrs_sync_status(clrs_ctx *c) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    int st = 0;
    int rc = read_info(c, &st);
    if (rc) return rc;
    if (c->timing) collect_times(c);
    return st;
}

extern "C" int clrs_sync_status_cholesky(clrs_ctx *c) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    int st = 0;
    int rc = read_info(c, &st, 1);
    return rc ? rc : st;
}

extern "C" int clrs_schur_factor_dev(clrs_ctx *c) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (c->p_cholQ_slabs.steps.empty()) {   // no fused single-GPU shortcut: the two split phases back to back
        int rc = clrs_schur_factor_local_dev(c);
        return rc ? rc : clrs_schur_factor_finish_dev(c);
    }
    if (!c->assembled) return fail(CLRS_ERR_STATE, "clrs_schur_factor called before clrs_schur_assemble");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[2], c->stream));
    if (!c->p_factor_small.steps.empty()) {                           // everything in one launch (k_factor_small)
        if ((rc = run_plan(c, c->p_factor_small))) return rc;
        if (c->timing) { HIPCHECK(hipEventRecord(c->ev[3], c->stream)); HIPCHECK(hipEventRecord(c->ev[4], c->stream)); HIPCHECK(hipEventRecord(c->ev[5], c->stream)); }
    } else {
    c->s_inv_valid = false;
    if ((rc = run_plan(c, c->p_cholS))) return rc;                    // chol S_j, LinvB_j and the Q slabs: one launch
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[3], c->stream)); HIPCHECK(hipEventRecord(c->ev[4], c->stream)); HIPCHECK(hipEventRecord(c->ev[5], c->stream)); }
    if ((rc = run_plan(c, c->p_cholQ_slabs))) return rc;              // Q = sum of slabs, chol Q: one launch
    }
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[6], c->stream)); c->times_pending = true; }
    c->assembled = false;
    c->factored = true;
    return 0;
}

extern "C" int clrs_schur_factor(clrs_ctx *c) {
    int rc = clrs_schur_factor_dev(c);
    if (rc) return rc;
    return clrs_sync_status(c);
}

extern "C" int clrs_get_factor(clrs_ctx *c, double *L, double *LinvB, double *LQ) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored) return fail(CLRS_ERR_STATE, "no factorisation available");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (L) {
        std::vector<double> h((size_t)c->Slen);
        HIPCHECK(hipMemcpy(h.data(), c->d_S, sizeof(double) * c->Slen, hipMemcpyDeviceToHost));
        for (int j = 0; j < c->J; j++) {
            const int P = c->P[j];
            double *Sj = h.data() + c->Soff[j];
            for (int col = 0; col < P; col++)
                for (int r = 0; r < col; r++) Sj[r + (i64)col * P] = 0.0;   // tools.jl:100-105
        }
        std::memcpy(L, h.data(), sizeof(double) * c->Slen);
    }
    if (LinvB && c->N > 0) {
        std::vector<double> h((size_t)(c->xlen * c->N));
        HIPCHECK(hipMemcpy(h.data(), c->d_LB, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        i64 off = 0;
        for (int j = 0; j < c->J; j++) {
            for (int col = 0; col < c->N; col++)
                for (int r = 0; r < c->P[j]; r++) LinvB[off + r + (i64)col * c->P[j]] = h[(size_t)(c->coff[j] + r + (i64)col * c->xlen)];
            off += (i64)c->P[j] * c->N;
        }
    }
    if (LQ && c->N > 0) {
        HIPCHECK(hipMemcpy(LQ, c->d_Q, sizeof(double) * c->N * c->N, hipMemcpyDeviceToHost));
        for (int col = 0; col < c->N; col++)
            for (int r = 0; r < col; r++) LQ[r + (i64)col * c->N] = 0.0;
    }
    return 0;
}

extern "C" int clrs_schur_solve_fwd_dev(clrs_ctx *c, const double *d_rhs_x) {
    if (!c || !d_rhs_x) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored && !c->local_factored) return fail(CLRS_ERR_STATE, "clrs_schur_solve called before clrs_schur_factor");
    HIPCHECK(hipSetDevice(c->device));
    if (c->fused_fs) c->bind_rhsx = d_rhs_x;
    else if (d_rhs_x != c->d_rhsx) HIPCHECK(hipMemcpyAsync(c->d_rhsx, d_rhs_x, sizeof(double) * c->xlen, hipMemcpyDeviceToDevice, c->stream));
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[7], c->stream));
    const int rc = run_plan(c, c->p_fwd_small.steps.empty() ? c->p_fwd : c->p_fwd_small);
    if (!rc && !c->s_inv.empty()) c->s_inv_valid = true;
    return rc;
}

extern "C" int clrs_schur_solve_bwd_dev(clrs_ctx *c, const double *d_rhs_y, double *d_dx, double *d_dy) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored) return fail(CLRS_ERR_STATE, "clrs_schur_solve called before clrs_schur_factor");
    HIPCHECK(hipSetDevice(c->device));
    if (c->N > 0 && !d_rhs_y) return fail(CLRS_ERR_INVALID, "rhs_y is required when there are free variables");
    // the fused kernels read / write the caller's buffers; the staged ones work on the context's own
    const bool q_direct = c->fused_q && c->N > 0, x_direct = c->fused_fs;
    c->bind_rhsy = q_direct ? d_rhs_y : c->d_rhsy;
    c->bind_dy = (c->fused_q && d_dy) ? d_dy : c->d_dy;
    c->bind_dx = (x_direct && d_dx) ? d_dx : c->d_dx;
    if (c->N > 0 && !q_direct && d_rhs_y != c->d_rhsy)
        HIPCHECK(hipMemcpyAsync(c->d_rhsy, d_rhs_y, sizeof(double) * c->N, hipMemcpyDeviceToDevice, c->stream));
    int rc = run_plan(c, c->p_bwd_small.steps.empty() ? c->p_bwd : c->p_bwd_small);
    if (rc) return rc;
    if (!c->s_inv.empty()) c->s_inv_valid = true;
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[8], c->stream)); c->solve_time_pending = true; }
    if (!x_direct && d_dx && d_dx != c->d_t) HIPCHECK(hipMemcpyAsync(d_dx, c->d_t, sizeof(double) * c->xlen, hipMemcpyDeviceToDevice, c->stream));
    if (!c->fused_q && d_dy && c->N > 0 && d_dy != c->d_dy) HIPCHECK(hipMemcpyAsync(d_dy, c->d_dy, sizeof(double) * c->N, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int clrs_schur_solve_dev(clrs_ctx *c, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy) {
    if (!c || !d_rhs_x || !d_dx) return fail(CLRS_ERR_INVALID, "null argument");
    if (c->p_solve_all.steps.empty()) {
        int rc = clrs_schur_solve_fwd_dev(c, d_rhs_x);
        return rc ? rc : clrs_schur_solve_bwd_dev(c, d_rhs_y, d_dx, d_dy);
    }
    if (!c->factored) return fail(CLRS_ERR_STATE, "clrs_schur_solve called before clrs_schur_factor");
    if (c->N > 0 && (!d_rhs_y || !d_dy)) return fail(CLRS_ERR_INVALID, "rhs_y / dy are required when there are free variables");
    HIPCHECK(hipSetDevice(c->device));
    c->bind_rhsx = d_rhs_x; c->bind_rhsy = d_rhs_y; c->bind_dx = d_dx; c->bind_dy = d_dy;
    if (c->timing) HIPCHECK(hipEventRecord(c->ev[7], c->stream));
    int rc = run_plan(c, c->p_solve_all);
    if (rc) return rc;
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[8], c->stream)); c->solve_time_pending = true; }
    return 0;
}

extern "C" int clrs_schur_solve(clrs_ctx *c, const double *rhs_x, const double *rhs_y, double *dx, double *dy) {
    if (!c || !rhs_x || !dx) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->factored) return fail(CLRS_ERR_STATE, "clrs_schur_solve called before clrs_schur_factor");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    pin_reset(c);
    if ((rc = h2d_staged(c, c->d_rhsx, rhs_x, sizeof(double) * c->xlen))) return rc;
    if (c->N > 0) {
        if (!rhs_y || !dy) return fail(CLRS_ERR_INVALID, "null argument");
        if ((rc = h2d_staged(c, c->d_rhsy, rhs_y, sizeof(double) * c->N))) return rc;
    }
    if ((rc = clrs_schur_solve_dev(c, c->d_rhsx, c->d_rhsy, c->d_dx, c->d_dy))) return rc;
    if ((rc = d2h_staged(c, dx, c->d_dx, sizeof(double) * c->xlen))) return rc;
    if (c->N > 0 && (rc = d2h_staged(c, dy, c->d_dy, sizeof(double) * c->N))) return rc;
    return d2h_finish(c);
}

extern "C" int clrs_cholesky_blocks_dev(clrs_ctx *c, const double *d_X, double *d_Xchol) {
    if (!c || !d_X || !d_Xchol) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    if (c->fused_x) {              // one launch, caller's buffers
        c->bind_X = d_X; c->bind_Xchol = d_Xchol;
        return run_plan(c, c->p_cholX);
    }
    if (d_X != c->d_X) HIPCHECK(hipMemcpyAsync(c->d_X, d_X, sizeof(double) * c->xylen, hipMemcpyDeviceToDevice, c->stream));
    int rc = run_plan(c, c->p_cholX);
    if (rc) return rc;
    if (d_Xchol != c->d_X) HIPCHECK(hipMemcpyAsync(d_Xchol, c->d_X, sizeof(double) * c->xylen, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int clrs_cholesky_blocks(clrs_ctx *c, const double *X, double *Xchol) {
    if (!c || !X || !Xchol) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    int rc;
    pin_reset(c);
    if ((rc = h2d_staged(c, c->d_X, X, sizeof(double) * c->xylen))) return rc;
    if ((rc = clrs_cholesky_blocks_dev(c, c->d_X, c->d_X))) return rc;
    if ((rc = d2h_staged(c, Xchol, c->d_X, sizeof(double) * c->xylen))) return rc;
    int st = 0;
    if ((rc = read_info(c, &st, 1))) return rc;          // synchronises the stream: the factors have landed as well
    if ((rc = d2h_finish(c))) return rc;
    return st;
}

extern "C" double *clrs_q_buffer_dev(clrs_ctx *c) { return c ? c->d_Q : nullptr; }
extern "C" double *clrs_u_buffer_dev(clrs_ctx *c) { return c ? c->d_u : nullptr; }
extern "C" double *clrs_S_buffer_dev(clrs_ctx *c) { return c ? c->d_S : nullptr; }
extern "C" double *clrs_AY_buffer_dev(clrs_ctx *c) { return c ? c->d_AY : nullptr; }
extern "C" void *clrs_stream(clrs_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" int clrs_set_timing(clrs_ctx *c, int enabled) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    c->timing = enabled != 0;
    return 0;
}
extern "C" int clrs_get_timings(clrs_ctx *c, double t[6]) {
    if (!c || !t) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipStreamSynchronize(c->stream));
    collect_times(c);
    for (int i = 0; i < 6; i++) t[i] = c->times[i];
    return 0;
}
extern "C" int clrs_get_counters(const clrs_ctx *c, double *ab, double *af, double *ff, double *sf) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (ab) *ab = c->cnt_bytes;
    if (af) *af = c->cnt_flops;
    if (ff) *ff = c->cnt_factor_flops;
    if (sf) *sf = c->cnt_solve_flops;
    return 0;
}
extern "C" int clrs_set_graph_mode(clrs_ctx *c, int enabled) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    c->graph_mode = enabled != 0;
    return 0;
}
extern "C" int clrs_plan_info(const clrs_ctx *c, int32_t *na, int32_t *nf, int32_t *ns) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    if (na) *na = c->p_assemble.launches();
    if (nf) *nf = c->p_cholS.launches() + c->p_linvB.launches() + c->p_Q.launches() + c->p_cholQ.launches();
    if (ns) *ns = c->p_fwd.launches() + c->p_bwd.launches();
    return 0;
}

// ---- external stream / per-kernel timing -----------------------------------------------------------
extern "C" int clrs_set_stream(clrs_ctx *c, void *stream) {
    if (!c) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamSynchronize(c->stream));
    Plan *plans[] = {&c->p_assemble, &c->p_cholS, &c->p_linvB, &c->p_Q, &c->p_cholQ, &c->p_fwd, &c->p_bwd, &c->p_cholX, &c->p_cholQ_slabs, &c->p_solve_all, &c->p_fwd_small, &c->p_bwd_small, &c->p_factor_small};
    for (Plan *p : plans)
        if (p->graph) { hipGraphExecDestroy(p->graph); p->graph = nullptr; }   // graphs are re-captured on the new stream
    if (c->own_stream) HIPCHECK(hipStreamDestroy(c->stream));
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
    return 0;
}

static int kt_collect(clrs_ctx *c) {
    if (c->kt_kinds.empty()) return 0;
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->kt_kinds.size(); i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->kt_ev[2 * i], c->kt_ev[2 * i + 1]) == hipSuccess) {
            c->kt_total[c->kt_kinds[i]] += ms * 1e-3;
            c->kt_count[c->kt_kinds[i]]++;
        }
    }
    c->kt_kinds.clear();
    return 0;
}

extern "C" int clrs_set_kernel_timing(clrs_ctx *c, int kind) {
    if (!c || kind < -2 || kind >= STEP_NKINDS) return fail(CLRS_ERR_INVALID, "bad kernel kind");
    int rc = kt_collect(c);
    if (rc) return rc;
    c->kt_kind = kind;
    for (int k = 0; k < STEP_NKINDS; k++) { c->kt_total[k] = 0; c->kt_count[k] = 0; }
    return 0;
}

extern "C" int clrs_get_kernel_times(clrs_ctx *c, int max_kinds, double *seconds, int64_t *launches) {
    if (!c || !seconds || !launches) return fail(CLRS_ERR_INVALID, "null argument");
    int rc = kt_collect(c);
    if (rc) return rc;
    for (int k = 0; k < max_kinds && k < STEP_NKINDS; k++) { seconds[k] = c->kt_total[k]; launches[k] = c->kt_count[k]; }
    return STEP_NKINDS;
}

extern "C" int clrs_config_set(const char *key, int value) {
    if (!key) return fail(CLRS_ERR_INVALID, "null argument");
    if (!std::strcmp(key, "fused_assemble")) { g_cfg_fused_assemble = value; return 0; }
    if (!std::strcmp(key, "split_blocks")) { g_cfg_split_blocks = value; return 0; }
    if (!std::strcmp(key, "fused_factor")) { g_cfg_fused_factor = value; return 0; }
    if (!std::strcmp(key, "wave_assemble")) { g_cfg_wave_assemble = value; return 0; }
    if (!std::strcmp(key, "wave2_assemble")) { g_cfg_wave2_assemble = value; return 0; }
    if (!std::strcmp(key, "wave3_assemble")) { g_cfg_wave3_assemble = value; return 0; }
    if (!std::strcmp(key, "wave4_assemble")) { g_cfg_wave4_assemble = value; return 0; }
    if (!std::strcmp(key, "wave5_assemble")) { g_cfg_wave5_assemble = value; return 0; }
    if (!std::strcmp(key, "dense_block")) { g_cfg_dense_block = value; return 0; }
    if (!std::strcmp(key, "dense_wave")) { g_cfg_dense_wave = value; return 0; }
    if (!std::strcmp(key, "factor_aug")) { g_cfg_factor_aug = value; return 0; }
    if (!std::strcmp(key, "pairing_tri")) { g_cfg_pairing_tri = value; return 0; }
    if (!std::strcmp(key, "potrf_levels")) { g_cfg_potrf_levels = value; return 0; }
    if (!std::strcmp(key, "trsm_blockinv")) { g_cfg_trsm_blockinv = value; return 0; }
    if (!std::strcmp(key, "solve_small2")) { g_cfg_solve_small2 = value; return 0; }
    if (!std::strcmp(key, "factor_small")) { g_cfg_factor_small = value; return 0; }
    if (!std::strcmp(key, "pin_limit")) { PIN_LIMIT = (size_t)std::max(value, 0); return 0; }
    if (!std::strcmp(key, "ipm_wmfma")) { g_cfg_ipm_wmfma = value; return 0; }
    if (!std::strcmp(key, "solve_small_max")) { g_cfg_solve_small_max = value; return 0; }
    if (!std::strcmp(key, "mw_exact_products")) { g_cfg_mw_exact_products = value; return 0; }
    if (!std::strcmp(key, "mw_refine")) { g_cfg_mw_refine = value; return 0; }
    if (!std::strcmp(key, "mw_factor_limbs")) { g_cfg_mw_factor_limbs = value; return 0; }
    if (!std::strcmp(key, "mw_affine_corrector")) { g_cfg_mw_affine_corrector = value; return 0; }
    if (!std::strcmp(key, "mw_pipeline")) { g_cfg_mw_pipeline = value; return 0; }
    if (!std::strcmp(key, "mw_pipeline64")) { g_cfg_mw_pipeline64 = value; return 0; }
    if (!std::strcmp(key, "mw_zt_small_maxn")) { g_cfg_mw_zt_small_maxn = value; return 0; }
    if (!std::strcmp(key, "mw_pipeline_x")) { g_cfg_mw_pipeline_x = value; return 0; }
    if (!std::strcmp(key, "mw_pipeline_x_min")) { g_cfg_mw_pipeline_x_min = value; return 0; }
    if (!std::strcmp(key, "mw_sharded_factor_limbs")) { g_cfg_mw_sharded_factor_limbs = value; return 0; }
    if (!std::strcmp(key, "mw_stream_words")) { g_cfg_mw_stream_words = value; return 0; }
    if (!std::strcmp(key, "mw_zi_narrow")) { g_cfg_mw_zi_narrow = value; return 0; }
    if (!std::strcmp(key, "modp_minors_chunk_bytes")) { g_cfg_modp_minors_chunk_bytes = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "zz_gemm_chunk_bytes")) { g_cfg_zz_gemm_chunk_bytes = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "liftm_chunk_bytes")) { g_cfg_liftm_chunk_bytes = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "lrsys_chunk_bytes")) { g_cfg_lrsys_chunk_bytes = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "lll_launch_swaps")) { g_cfg_lll_launch_swaps = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "field_round_launch_rungs")) { g_cfg_field_round_launch_rungs = value < 0 ? 0 : value; return 0; }
    if (!std::strcmp(key, "mw_xinv_product")) { g_cfg_mw_xinv_product = value; return 0; }
    if (!std::strcmp(key, "mw_chain_hop")) { g_cfg_mw_chain_hop = value; return 0; }
    if (!std::strcmp(key, "mw_skip_xfb")) { g_cfg_mw_skip_xfb = value; return 0; }
    if (!std::strcmp(key, "mw_y_riders")) { g_cfg_mw_y_riders = value; return 0; }
    if (!std::strcmp(key, "mw_refine_predictor")) { g_cfg_mw_refine_predictor = value; return 0; }
    return fail(CLRS_ERR_INVALID, std::string("unknown configuration key ") + key);
}

#ifdef CLRS_W3_STAMPS
extern "C" int clrs_debug_cf_stamps(clrs_ctx *c, uint64_t out[16]) {
    if (!c || !out) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cf_stamps), 16 * sizeof(uint64_t)));
    return 0;
}
extern "C" int clrs_debug_ss2_stamps(clrs_ctx *c, uint64_t out[16]) {
    if (!c || !out) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ss2_stamps), 16 * sizeof(uint64_t)));
    return 0;
}
extern "C" int clrs_debug_w3_stamps(clrs_ctx *c, uint64_t out[16]) {
    if (!c || !out) return fail(CLRS_ERR_INVALID, "null argument");
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_w3_stamps), 16 * sizeof(uint64_t)));
    return 0;
}
#endif

extern "C" int clrs_debug_stamps(clrs_ctx *c, uint64_t out[64]) {
    if (!c || !out) return fail(CLRS_ERR_INVALID, "null argument");
    if (!c->ftables.stamps) { std::memset(out, 0, 64 * sizeof(uint64_t)); return 0; }
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemcpy(out, c->ftables.stamps, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int clrs_fused_clusters(const clrs_ctx *c) { return c ? c->n_fused_clusters : 0; }
extern "C" int clrs_wave_clusters(const clrs_ctx *c) { return c ? c->n_wave_clusters + c->n_wave2_clusters : 0; }
extern "C" int clrs_wave2_clusters(const clrs_ctx *c) { return c ? c->n_wave2_clusters : 0; }
extern "C" int clrs_wave4_clusters(const clrs_ctx *c) { return c ? c->n_wave4_clusters : 0; }
extern "C" int clrs_wave5_clusters(const clrs_ctx *c) { return c ? c->n_wave5_clusters : 0; }

extern "C" const char *clrs_kernel_name(int kind) { return (kind >= 0 && kind < STEP_NKINDS) ? STEP_NAMES[kind] : ""; }

extern "C" const char *clrs_strerror(int code) {
    switch (code) {
        case CLRS_OK: return "ok";
        case CLRS_ERR_INVALID: return "invalid argument or malformed SDP description";
        case CLRS_ERR_HIP: return "HIP runtime error";
        case CLRS_ERR_NO_DEVICE: return "no usable HIP device";
        case CLRS_ERR_STATE: return "call order violated";
        default: return code > 0 ? "factorisation failure (non-positive pivot)" : "unknown error";
    }
}
extern "C" const char *clrs_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *clrs_version(void) { return "clrs-hip 0.1.0 (gfx950)"; }

#include "clrs_ipm_host.inc"

// ------------------------------------------------------------------------------------------------
// test hooks
// ------------------------------------------------------------------------------------------------
static CtxOwner mini_ctx(int device) {
    CtxOwner c(new clrs_ctx(), clrs_ctx_destroy);
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) c.reset();
    if (!c) return c;
    (void)hipFuncSetAttribute((const void *)k_gemm_f64_t<128, 128, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_lds_bytes(128, 128));
    (void)hipFuncSetAttribute((const void *)k_gemm_f64_t<128, 128, 0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_lds_bytes(128, 128));
    (void)hipFuncSetAttribute((const void *)k_gemm_f64_t<128, 128, 1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_lds_bytes(128, 128));
    (void)hipFuncSetAttribute((const void *)k_gemm_f64_t<128, 128, 1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_lds_bytes(128, 128));
    std::vector<int> hi(1, INFO_NONE);
    if (upload(c.get(), hi, &c->d_info)) c.reset();
    return c;
}

extern "C" int clrs_test_gemm(int device, int ta, int tb, int M, int N, int K, double alpha, const double *A, int lda, const double *B,
                              int ldb, double beta, double *C, int ldc) {
    const CtxOwner own = mini_ctx(device);
    clrs_ctx *c = own.get();
    if (!c) return fail(CLRS_ERR_NO_DEVICE, "no device");
    int rc = 0;
    i64 na = (i64)lda * (ta ? M : K), nb = (i64)ldb * (tb ? K : N), nc = (i64)ldc * N;
    std::vector<double> hA(A, A + na), hB(B, B + nb), hC(C, C + nc);
    double *dA, *dB, *dC;
    if ((rc = upload(c, hA, &dA)) || (rc = upload(c, hB, &dB)) || (rc = upload(c, hC, &dC))) return rc;
    Plan pl;
    std::vector<GemmDesc> g;
    g.push_back(mk_gemm(ta, tb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc));
    if (!(rc = add_gemm_stage(c, pl, g)) && !(rc = run_steps(c, pl))) {
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(C, dC, sizeof(double) * nc, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(CLRS_ERR_HIP, "copy back failed");
    }
    return rc;
}

extern "C" int clrs_test_potrf(int device, int n, double *A, int lda) {
    const CtxOwner own = mini_ctx(device);
    clrs_ctx *c = own.get();
    if (!c) return fail(CLRS_ERR_NO_DEVICE, "no device");
    int rc = 0, st = 0;
    std::vector<double> hA(A, A + (i64)lda * n);
    double *dA;
    if ((rc = upload(c, hA, &dA))) return rc;
    Plan pl;
    std::vector<PotrfJob> pj;
    pj.push_back(PotrfJob{dA, lda, n, 1});
    if (!(rc = plan_potrf(c, pl, pj)) && !(rc = run_steps(c, pl)) && !(rc = read_info(c, &st))) {
        if (hipMemcpy(A, dA, sizeof(double) * (i64)lda * n, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(CLRS_ERR_HIP, "copy back failed");
    }
    return rc ? rc : st;
}

// ---- measurement hook: what a pure streaming kernel reaches at a given footprint and read : write mix -------------------------
// (bench.py reports the assembly kernel's HBM traffic per second beside this rate: the 8 TB/s of the data sheet is not reachable by
// any kernel -- beyond the 256 MiB Infinity Cache a plain copy runs at 5.0-5.8 TB/s on this part)
typedef double v2d_stream __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_stream_probe(const v2d_stream *__restrict__ a, const v2d_stream *__restrict__ b, v2d_stream *__restrict__ w,
                                                      long long nr, long long nw) {
    const long long stride = (long long)gridDim.x * 256, n = nr > nw ? nr : nw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += 4 * stride) {
        v2d_stream x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long k = i + u * stride;
            x[u] = y[u] = (v2d_stream){0.0, 0.0};
            if (k < nr) { x[u] = a[k]; y[u] = b[k]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long k = i + u * stride;
            if (k < nw) __builtin_nontemporal_store(x[u] + y[u], w + k);
        }
    }
}

extern "C" int clrs_test_stream(int device, long long read_bytes, long long write_bytes, int reps, double *avg_us) {
    if (read_bytes < 32 || write_bytes < 16 || reps < 1 || !avg_us) return fail(CLRS_ERR_INVALID, "clrs_test_stream: bad arguments");
    if (hipSetDevice(device) != hipSuccess) return fail(CLRS_ERR_NO_DEVICE, "no device");
    const long long nr = read_bytes / 32, nw = write_bytes / 16;        // 16-byte elements: two read streams of nr, one write stream of nw
    v2d_stream *a = nullptr, *b = nullptr, *w = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = nullptr;
    int rc = 0;
    auto ok = [&](hipError_t e, const char *what) { if (e != hipSuccess && !rc) rc = fail(CLRS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); return e == hipSuccess; };
    if (ok(hipMalloc(&a, nr * 16), "hipMalloc") && ok(hipMalloc(&b, nr * 16), "hipMalloc") && ok(hipMalloc(&w, nw * 16), "hipMalloc") &&
        ok(hipMemset(a, 0, nr * 16), "hipMemset") && ok(hipMemset(b, 0, nr * 16), "hipMemset") && ok(hipMemset(w, 0, nw * 16), "hipMemset") &&
        ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize") &&      // the fills (null stream) are done before the probe's own stream starts
        ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate") && ok(hipEventCreate(&e0), "hipEventCreate") && ok(hipEventCreate(&e1), "hipEventCreate")) {
        hipDeviceProp_t prop;
        int cus = 256;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus = prop.multiProcessorCount;
        const int grid = 2 * cus;
        for (int r = 0; r < 3; r++) hipLaunchKernelGGL(k_stream_probe, dim3(grid), dim3(256), 0, st, a, b, w, nr, nw);
        ok(hipEventRecord(e0, st), "hipEventRecord");
        for (int r = 0; r < reps; r++) hipLaunchKernelGGL(k_stream_probe, dim3(grid), dim3(256), 0, st, a, b, w, nr, nw);
        ok(hipEventRecord(e1, st), "hipEventRecord");
        ok(hipEventSynchronize(e1), "hipEventSynchronize");
        float ms = 0.f;
        if (ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime")) *avg_us = 1e3 * (double)ms / reps;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (w) (void)hipFree(w);
    return rc;
}

extern "C" int clrs_test_trsm(int device, int trans, int n, int nrhs, const double *L, int ldl, double *B, int ldb) {
    const CtxOwner own = mini_ctx(device);
    clrs_ctx *c = own.get();
    if (!c) return fail(CLRS_ERR_NO_DEVICE, "no device");
    int rc = 0;
    std::vector<double> hL(L, L + (i64)ldl * n), hB(B, B + (i64)ldb * nrhs);
    double *dL, *dB;
    if ((rc = upload(c, hL, &dL)) || (rc = upload(c, hB, &dB))) return rc;
    Plan pl;
    std::vector<TrsmJob> tj;
    tj.push_back(TrsmJob{dL, ldl, n, dB, ldb, nrhs});
    if (!(rc = plan_trsm(c, pl, tj, trans)) && !(rc = run_steps(c, pl))) {
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(B, dB, sizeof(double) * (i64)ldb * nrhs, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(CLRS_ERR_HIP, "copy back failed");
    }
    return rc;
}

// ---- the three fp64 smallest-eigenvalue routines of the step length on matrices given to them ---------------------------------
// A: `count` symmetric n x n matrices, column-major, both triangles, back to back; out[count]: their smallest eigenvalues.  One launch, one workgroup per
// matrix.  form 0: wg_min_eig32 (2 <= n <= 64) and form 1: wg_min_eig (1 <= n <= 128), the routines of k_mwi_step (clrs_mw_ipm.hip.h); form 2:
// ipm_min_eig, the second half of k_ipm_step (2 <= n <= 64).  Domain: entries of magnitude above about 2^-500 or zero -- below, the squares in x^T x
// underflow and the Householder vectors lose their accuracy; the iteration never sees such matrices (W = L^-1 dM L^-T of iterates of ordinary size).
int mw_test_min_eig_launch(int form, int n, int count, const double *dA, double *dOut);      // clrs_mw.hip (host side: clrs_mw_ipm_host.inc)
extern "C" int clrs_test_min_eig(int device, int form, int n, int count, const double *A, double *out) {
    if (!A || !out || count < 1) return fail(CLRS_ERR_INVALID, "clrs_test_min_eig: bad arguments");
    if (form < 0 || form > 2) return fail(CLRS_ERR_INVALID, "clrs_test_min_eig: form is 0 (wg_min_eig32), 1 (wg_min_eig) or 2 (the fp64 loop's routine)");
    if (form == 1 ? (n < 1 || n > 128) : (n < 2 || n > 64))
        return fail(CLRS_ERR_INVALID, form == 1 ? "clrs_test_min_eig: form 1 takes 1 <= n <= 128" : "clrs_test_min_eig: forms 0 and 2 take 2 <= n <= 64");
    if (hipSetDevice(device) != hipSuccess) return fail(CLRS_ERR_NO_DEVICE, "no device");
    const size_t bytes = sizeof(double) * (size_t)n * n * count;
    double *dA = nullptr, *dOut = nullptr;
    int rc = 0;
    auto ok = [&](hipError_t e, const char *what) { if (e != hipSuccess && !rc) rc = fail(CLRS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); return e == hipSuccess; };
    if (ok(hipMalloc(&dA, bytes), "hipMalloc") && ok(hipMalloc(&dOut, sizeof(double) * count), "hipMalloc") &&
        ok(hipMemcpy(dA, A, bytes, hipMemcpyHostToDevice), "hipMemcpy") && ok(hipMemset(dOut, 0, sizeof(double) * count), "hipMemset")) {
        if (form == 2) {
            const int n16 = (n + 15) & ~15, lda = n16 + 2;
            hipLaunchKernelGGL(k_ipm_test_min_eig, dim3(count), dim3(256), sizeof(double) * (size_t)(lda * (n16 + 8) + 2 * n16 + 144), nullptr, dA, dOut, n);
            ok(hipGetLastError(), "k_ipm_test_min_eig");
        } else rc = mw_test_min_eig_launch(form, n, count, dA, dOut);
        if (!rc && ok(hipDeviceSynchronize(), "hipDeviceSynchronize")) ok(hipMemcpy(out, dOut, sizeof(double) * count, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    if (dA) (void)hipFree(dA);
    if (dOut) (void)hipFree(dOut);
    return rc;
}

/*
 * clrs_hip.h -- C ABI of the MI355X-native interior-point hot path for clustered low-rank SDPs.
 *
 * This is the drop-in boundary for the ONE path of nanleij/ClusteredLowRankSolver.jl (v2.1.0) that
 * this repository accelerates: per-iteration Schur-complement assembly from low-rank constraint
 * matrices and the block-Cholesky factor/solve of the cluster-block-diagonal normal equations.
 * The reference has no FFI seam for this path (it is plain Julia mutating preallocated Arb buffers);
 * each entry point below names the reference function it replaces (paths relative to the reference
 * repository).  INTEGRATION.md shows the Julia `ccall` shim a maintainer would add.
 *
 * Conventions
 *   - plain C: pointers, sizes, int return codes; no C++/torch types.
 *   - all matrices are COLUMN-MAJOR fp64 (Julia `Matrix{Float64}` layout).
 *   - block-diagonal iterates X, Y (and the Cholesky factors of X) are passed as ONE array: the
 *     blocks (j,l) in the order of `clrs_sdp_desc`, each n x n column-major, concatenated
 *     ("xy layout", length sum n^2).
 *   - S / L_j are passed as one array: per cluster P_j x P_j column-major, concatenated ("S layout").
 *   - x-like vectors (rhs_x, dx) concatenate the clusters (length sum P_j).
 *   - indices are 0-based; constraint indices are cluster-local (the reference's `cs_map`,
 *     src/solver.jl:156-167, is applied by the caller).
 *   - one context per GPU / per process; a context is not thread-safe (like the reference's shared
 *     scratch `tempX`, `part_r`).
 *   - return value: 0 ok; >0 factorisation failure (see clrs_schur_factor); <0 an error from
 *     `clrs_strerror`.
 *   - host entry points take host pointers and synchronise before returning; `_dev` entry points
 *     take device pointers, enqueue on the context's stream and do NOT synchronise.
 */
#ifndef CLRS_HIP_H
#define CLRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLRS_OK 0
#define CLRS_ERR_INVALID (-1)      /* malformed description / argument */
#define CLRS_ERR_HIP (-2)          /* a HIP runtime call failed (message via clrs_last_error) */
#define CLRS_ERR_NO_DEVICE (-3)    /* no usable gfx950 device */
#define CLRS_ERR_STATE (-4)        /* call order violated (e.g. solve before factor) */

/*
 * Numeric description of a ClusteredLowRankSDP restricted to what the hot path reads:
 * replaces the traversal of `sdp.A[j][l][r,s][p]`, `sdp.B[j]` (src/interface.jl:807-819) done by
 * precompute_matrices_bilinear_pairings (src/solver.jl:985-1059).
 *
 * Blocks are listed cluster by cluster.  A low-rank block (kind 0) is an m x m grid of delta x delta
 * sub-blocks; each term t is one rank-1 piece lambda * vs * ws^T of A[j][l][r,s][p]
 * (LowRankMat, src/interface.jl:759-763).  The convention A[r,s][p] = A[s,r][p]^T
 * (src/solver.jl:1009) is required: for every term (p,r,s,rank) the term (p,s,r,rank) must exist.
 * A dense ("high rank") block (kind 1) has m == 1 and lists its matrices A[j][l][1,1][p].
 */
typedef struct clrs_sdp_desc {
    int32_t n_clusters;            /* J */
    int32_t n_free;                /* N, number of free variables (columns of B) */
    const int32_t *cluster_P;      /* [J] constraints per cluster */
    const double *B;               /* per cluster P_j x N column-major, concatenated */
    int32_t n_blocks;              /* total number of PSD blocks (j,l) */
    const int32_t *block_cluster;  /* [NB] cluster of each block (non-decreasing) */
    const int32_t *block_m;        /* [NB] sub-blocks per side */
    const int32_t *block_delta;    /* [NB] sub-block size; block side n = m*delta */
    const int32_t *block_kind;     /* [NB] 0 = low rank, 1 = dense */
    const int64_t *term_ptr;       /* [NB+1] CSR: terms of block b are term_ptr[b]..term_ptr[b+1]-1 */
    const int32_t *term_p;         /* [T] constraint index in the cluster */
    const int32_t *term_r;         /* [T] sub-block row */
    const int32_t *term_s;         /* [T] sub-block column */
    const int32_t *term_rank;      /* [T] index of the rank-1 piece inside A[r,s][p] */
    const double *term_lambda;     /* [T] */
    const int64_t *term_vec_ptr;   /* [T+1] offsets of the term's vectors in term_vs / term_ws */
    const double *term_vs;         /* delta doubles per term */
    const double *term_ws;         /* delta doubles per term */
    const int64_t *dense_ptr;      /* [NB+1] CSR over dense entries */
    const int32_t *dense_p;        /* [D] constraint index in the cluster */
    const int64_t *dense_A_ptr;    /* [D+1] offsets into dense_A */
    const double *dense_A;         /* n x n column-major per entry */
} clrs_sdp_desc;

typedef struct clrs_ctx clrs_ctx;

/* Sizes of the flat layouts, for buffer allocation by the caller. */
typedef struct clrs_dims {
    int64_t xy_len;    /* sum n^2 over blocks */
    int64_t x_len;     /* sum P_j */
    int64_t S_len;     /* sum P_j^2 */
    int64_t n_terms;   /* T */
    int32_t n_free;    /* N */
    int32_t n_clusters;
    int32_t n_blocks;
    int32_t reserved;
} clrs_dims;

/* Create a context on HIP device `device`: de-duplicates the sampled vectors, builds the gather
 * tables and the launch plan, uploads all static data and allocates every device buffer.
 * Replaces: precompute_matrices_bilinear_pairings (src/solver.jl:985-1059), the preallocation
 * block src/solver.jl:298-317 and ThreadingInfo (src/threadinginfo.jl:59-102). */
int clrs_ctx_create(const clrs_sdp_desc *desc, int device, clrs_ctx **out);
void clrs_ctx_destroy(clrs_ctx *ctx);
int clrs_get_dims(const clrs_ctx *ctx, clrs_dims *dims);

/* Number of unique right / left vectors of sub-block row r of block b after de-duplication
 * (sizes of rightvecs[j][l][r] / leftvecs[j][l][r], src/solver.jl:1018-1051). */
int clrs_get_unique_counts(const clrs_ctx *ctx, int32_t block, int32_t r, int32_t *n_right, int32_t *n_left);

/* Cluster sharding across GPUs (one process per GPU) is done by the caller: each rank creates its
 * context from the sub-description holding only ITS clusters (all N free variables), calls
 * clrs_schur_factor_local_dev, sums the partial Q (clrs_q_buffer_dev) over ranks with one RCCL
 * all-reduce and calls clrs_schur_factor_finish_dev; the solve is split the same way around the
 * all-reduce of the partial u = LinvB^T t (clrs_u_buffer_dev).  clrs_schur_solve_fwd_dev may be called right after
 * clrs_schur_factor_local_dev (it needs only L_j and LinvB_j), and the u buffer lies directly behind the Q buffer
 * (clrs_u_buffer_dev == clrs_q_buffer_dev + N * N): the exchange of Q can be deferred to the first solve after a
 * factorisation and merged with that solve's exchange of u into ONE all-reduce of N * N + N doubles, followed by
 * clrs_schur_factor_finish_dev and clrs_schur_solve_bwd_dev (clrs_amd.sharded.ShardedSchur does this). */

/* Lower Cholesky factors of all X blocks: Xchol_blk = chol(X_blk).
 * Replaces: the approx_cholesky!(X_inv_blk, X_blk) loop, src/solver.jl:388-399.
 * Returns 0, or b+1 for the first block whose pivot is not positive. */
int clrs_cholesky_blocks(clrs_ctx *ctx, const double *X, double *Xchol);

/* Schur complement assembly S[j][p,q] = sum_l <A_p, X^-1 A_q Y> from the Cholesky factors of X
 * (xy layout) and Y.  Optionally returns S (S layout, full symmetric) and the per-term bilinear
 * pairings w^T Y v (A_Y, length T, in term order).
 * Replaces: compute_S_integrated! (src/solver.jl:1062-1226). */
int clrs_schur_assemble(clrs_ctx *ctx, const double *Xchol, const double *Y, double *S_out, double *AY_out);

/* S_j = L_j L_j^T, LinvB_j = L_j^-1 B_j, Q = sum_j LinvB_j^T LinvB_j, Q = L_Q L_Q^T.
 * Replaces: steps 3-4 of compute_T_decomposition! (src/solver.jl:1244-1279).
 * Returns 0; j+1 if S_j is not positive definite ("S was not decomposed succesfully in block j",
 * :1249); n_clusters+1 if Q is not ("Q was not decomposed correctly", :1277). */
int clrs_schur_factor(clrs_ctx *ctx);

/* Copies of the factors for inspection / for the caller's buffers `S` (holding L_j), `LinvB`, `Q`
 * (holding L_Q) of compute_T_decomposition!.  Any pointer may be NULL.
 * L: S layout (strict upper triangles zero); LinvB: per cluster P_j x N column-major, concatenated;
 * LQ: N x N. */
int clrs_get_factor(clrs_ctx *ctx, double *L, double *LinvB, double *LQ);

/* Solve [S -B; B^T 0] (dx; dy) = (rhs_x; rhs_y) with the current factorisation.
 * Replaces: the "solve system" stage of compute_search_direction! (src/solver.jl:1527-1582). */
int clrs_schur_solve(clrs_ctx *ctx, const double *rhs_x, const double *rhs_y, double *dx, double *dy);

/* --- device-pointer / sharded variants (enqueue on the context stream, no synchronisation) --- */
int clrs_cholesky_blocks_dev(clrs_ctx *ctx, const double *d_X, double *d_Xchol);
int clrs_sync_status_cholesky(clrs_ctx *ctx);   /* blocks; status of the last clrs_cholesky_blocks_dev: 0 or block b+1 */
int clrs_schur_assemble_dev(clrs_ctx *ctx, const double *d_Xchol, const double *d_Y);
int clrs_schur_factor_dev(clrs_ctx *ctx);                     /* whole factorisation on one GPU (no exchange, no sync) */
int clrs_schur_solve_dev(clrs_ctx *ctx, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy);
int clrs_schur_factor_local_dev(clrs_ctx *ctx);               /* up to the local partial Q */
double *clrs_q_buffer_dev(clrs_ctx *ctx);                     /* N x N device buffer holding Q (partial, then total) */
int clrs_schur_factor_finish_dev(clrs_ctx *ctx);              /* Cholesky of the (summed) Q */
int clrs_schur_solve_fwd_dev(clrs_ctx *ctx, const double *d_rhs_x);   /* t = L^-1 rhs_x ; u = LinvB^T t (partial) */
double *clrs_u_buffer_dev(clrs_ctx *ctx);                     /* N doubles: the partial u, to be summed over ranks */
int clrs_schur_solve_bwd_dev(clrs_ctx *ctx, const double *d_rhs_y, double *d_dx, double *d_dy);
double *clrs_S_buffer_dev(clrs_ctx *ctx);                     /* S layout; holds S after assemble, L_j after factor */
double *clrs_AY_buffer_dev(clrs_ctx *ctx);                    /* [T] */
/* Blocks until the stream is idle and returns the factorisation status of the last factor call
 * (same codes as clrs_schur_factor). */
int clrs_sync_status(clrs_ctx *ctx);
void *clrs_stream(clrs_ctx *ctx);                             /* hipStream_t of the context */

/* --- device-resident interior-point iteration around the path -------------------------
 * The whole loop body of solvesdp (src/solver.jl:348-589) with x, y, X, Y and every intermediate in HBM: residuals
 * (:863-918, 961-983), search directions (:1474-1616, with the solves of this library), step lengths (:1620-1693) and the
 * update (:485-495).  The host sequences kernels and reads one record per iteration.  Available when every PSD block
 * fits in LDS (n <= ~48); otherwise clrs_ipm_create returns CLRS_ERR_INVALID and the caller keeps its own loop. */
typedef struct clrs_ipm_data {
    const double *C;      /* objective matrices, xy layout (sdp.C) */
    const double *c;      /* right-hand sides, x layout (sdp.c) */
    const double *b;      /* objective of the free variables [N] (sdp.b) */
    int32_t maximize;     /* sdp.maximize */
    int32_t reserved;
    double constant;      /* objective constant */
} clrs_ipm_data;
typedef struct clrs_ipm_params {   /* keyword arguments of solvesdp, src/solver.jl:100-127 */
    double beta_infeasible, beta_feasible, gamma;
    double dual_error_threshold, primal_error_threshold, max_complementary_gap, step_length_threshold;
    int32_t safe_step;
    int32_t corrector_only;   /* the reference's `correctoronly` keyword (src/solver.jl:121, 370-374, 945): mu_p = mu in the predictor's residual and no "optimal" termination
                               * (the loop ends on need_dual_feasible / need_primal_feasible, errors or max_iterations only).  clrs_mw_ipm_*; the fp64 loop refuses it */
} clrs_ipm_params;
typedef struct clrs_ipm_record {   /* one row of the reference's iteration table (:566-582) + status */
    int32_t iter, pd_feas, error_code, factor_status, cholesky_status;
    int32_t refine_bits;   /* clrs_mw_ipm_*: bits the FIRST pass of the corrector's refined solve was good to, -log2(max|correction| / max|solution|) over dx and dy
                            * (0: no refinement step ran).  With factors in fewer limbs (clrs_mw_options.factor_limbs) the library returns to all limbs when this
                            * falls below one limb plus a margin */
    double mu, d_obj, p_obj, gap, dual_error, primal_error, alpha_d, alpha_p, beta_c, max_P, max_p, max_d;
} clrs_ipm_record;
int clrs_ipm_create(clrs_ctx *ctx, const clrs_ipm_data *data);
int clrs_ipm_set_params(clrs_ctx *ctx, const clrs_ipm_params *params);
int clrs_ipm_init(clrs_ctx *ctx, double omega_p, double omega_d);            /* x = y = 0, X = omega_p I, Y = omega_d I */
int clrs_ipm_iterate(clrs_ctx *ctx, clrs_ipm_record *out);                   /* one iteration; error_code 0 / 1 / 3 / 4 as docs/src/solving.md:64-70 */
int clrs_ipm_get(clrs_ctx *ctx, double *x, double *y, double *X, double *Y); /* copy the iterate to the host (any pointer may be NULL) */
int clrs_ipm_debug(clrs_ctx *ctx, double out[32]);                           /* diagnostic builds only: kernel phase stamps */

/* Timings of the last assemble/factor calls in seconds, measured with HIP events on the context
 * stream: t[0..4] = schur, cholS, LinvB, Q, cholQ -- the 5-way split compute_T_decomposition!
 * returns (src/solver.jl:1282-1286); t[5] = last solve.  Enabled by clrs_set_timing(ctx, 1). */
int clrs_set_timing(clrs_ctx *ctx, int enabled);
int clrs_get_timings(clrs_ctx *ctx, double t[6]);

/* Algorithmic work of one Schur assembly (SURVEY.md section 8d formulas, with the de-duplicated
 * vector counts): bytes and flops; and of one factor + one solve. */
int clrs_get_counters(const clrs_ctx *ctx, double *assemble_bytes, double *assemble_flops,
                      double *factor_flops, double *solve_flops);

/* Run every later call on the caller's hipStream_t instead of the context's own stream (e.g. the
 * stream a collective library orders itself against).  The caller keeps ownership of the stream. */
int clrs_set_stream(clrs_ctx *ctx, void *hip_stream);

/* Per-kernel timing with HIP events recorded on the context stream around every launch of kernel
 * `kind` (-1: every kind, -2: off; resets the accumulators).  Only in eager (non-graph) mode.
 * clrs_get_kernel_times synchronises, fills seconds[k] / launches[k] for k < max_kinds and returns
 * the number of kinds; clrs_kernel_name(k) names them (the names rocprofv3 --kernel-trace shows). */
int clrs_set_kernel_timing(clrs_ctx *ctx, int kind);
int clrs_get_kernel_times(clrs_ctx *ctx, int max_kinds, double *seconds, int64_t *launches);
const char *clrs_kernel_name(int kind);

/* Process-wide knobs, read when a context is created.  "fused_assemble" (default 1): clusters whose blocks fit
 * in one CU's LDS are assembled by the fused per-cluster kernel; 0 forces the staged grouped-GEMM path.
 * clrs_fused_clusters returns how many clusters of the context the fused kernel takes. */
int clrs_config_set(const char *key, int value);
int clrs_fused_clusters(const clrs_ctx *ctx);
/* "wave_assemble" (default 1): among those, clusters made only of simple rank-1 blocks with n <= 16 and small dense
 * blocks are assembled with one wave per PSD block (k_cluster_assemble_w1); clrs_wave_clusters counts them. */
int clrs_wave_clusters(const clrs_ctx *ctx);
/* "wave2_assemble" (default 1 = automatic; 2 = always; 0 = never): of those, clusters whose low-rank blocks all use the same
 * constraint order (and whose dense blocks are 1 x 1) are assembled by ONE wave per cluster with S in registers.
 * "wave3_assemble" (default 1): with U = P <= 32 that wave is k_cluster_assemble_w3 -- MFMA accumulators reused as operands,
 * nothing but the row of chol(X) and S_j on its way out touches LDS, each wave walks a contiguous run of clusters with the next
 * block's loads in flight -- and "automatic" means always (it is also the fastest form for two clusters); otherwise
 * (U <= 64, or "wave3_assemble" = 0) it is the LDS-staged k_cluster_assemble_w2 and "automatic" means >= 64 clusters.
 * clrs_wave2_clusters counts the clusters either kernel takes. */
int clrs_wave2_clusters(const clrs_ctx *ctx);
/* "wave4_assemble" (default 1): clusters of the same kind (every low-rank block simple, U = P, one constraint order; dense blocks 1 x 1) with a block
 * of 17 .. 32 rows or 33 .. 64 constraints -- out of reach of k_cluster_assemble_w3 -- take k_cluster_assemble_w4 (csrc/clrs_assemble_w4.hip.h: two
 * row tiles, three or four column tiles, L^-1 V by blocks without forming L^-1); 0 leaves them on the general LDS-staged kernel.
 * clrs_wave4_clusters counts them (they are not in clrs_wave_clusters / clrs_wave2_clusters). */
int clrs_wave4_clusters(const clrs_ctx *ctx);
/* "wave5_assemble" (default 1): clusters whose PSD blocks are all 2 x 2 blocks of 16 x 16 sub-blocks carrying E_rs (x) v v^T on the same <= 32 sample vectors in
 * (0,0), (1,1) and the symmetrised off-diagonal pair (the matrix-valued constraints of Nsphere_packing) take k_cluster_assemble_w5
 * (csrc/clrs_assemble_w5.hip.h); clrs_wave5_clusters counts them. */
int clrs_wave5_clusters(const clrs_ctx *ctx);
/* "factor_small" (default 1): a context with ONE cluster (P, N <= 64) runs clrs_schur_factor as one launch of k_factor_small
 * (S_j and B_j staged in one trip, Q never leaves LDS before it is factored); 2 = also for 2-4 clusters, one wave per cluster
 * (slower than the workgroup-per-cluster kernels on the named problems: kept for measurement); 0 = never.
 * "split_blocks" (default 1): when at most 32 clusters take the general fused assembly (k_cluster_assemble), every PSD block
 * of a cluster gets a workgroup of its own (groups of blocks beyond 32 per cluster) that writes its contribution to S_j as a
 * slab; k_sum_S_slabs adds the slabs in block order, which reproduces the one-workgroup accumulation bit for bit; 0 = one
 * workgroup per cluster.
 * "solve_small_max" (default 32768): the one-workgroup solve stage (k_solve_small / k_solve_small2) is used while the operands
 * of a solve (L_j, LinvB, L_Q) stay below this many doubles; beyond, one workgroup per cluster in three launches.
 * "ipm_wmfma" (default 3): the device-resident interior-point loop (clrs_ipm_*) forms, for low-rank blocks that are large enough
 * and whose operands fit in LDS, (bit 0) sum_i a_i A_i as one MFMA contraction over the block's terms and (bit 1) Z V for the
 * per-term pairings as one MFMA product; 0 = per-entry loops.
 * "solve_small2" (default 1): contexts with <= 8 clusters whose factors fit in 150 KB of LDS run the solve stage as ONE launch
 * of k_solve_small2 (every operand staged in one trip to memory, one wave per triangular solve); 0 keeps k_solve_small.
 * "dense_wave" (default 1): dense blocks with n <= 32 beyond the LDS-resident kernel form X^-1 A Y with one wave per matrix
 * (k_trtri32 + k_dense_T32); 0 = two substitution launches and a batched GEMM.
 * "factor_aug" (default 1): a context whose clusters are all beyond one 64-wide block, with 1 .. 512 free variables, factors [S_j .; B_j^T 0] in one
 * blocked factorisation that stops before the corner: L^-1 B comes out as the panels of the appended block row, -Q as its Schur
 * complement (k_chol_pack, k_chol_level, k_chol_unpack); 0 = Cholesky of S, the substitution for L^-1 B and the Gram product apart.
 * "pairing_tri" (default 1): staged low-rank blocks whose left and right vectors coincide (W = V, one sub-block) compute only the
 * lower tiles of the symmetric pairing matrices V^T X^-1 V and V^T Y V, and staged dense blocks only the lower tiles of
 * <A_i, X^-1 A_k Y>; k_schur_gather mirrors its reads; 0 = full matrices.
 * "potrf_levels" (default 1): the staged Cholesky of a matrix beyond one 64-wide block runs ONE launch per block column
 * (k_chol_level); 0 = k_potrf_diag + k_trsm_diag + k_gemm_f64_t per block column.
 * "trsm_blockinv" (default 1): staged triangular solves with n > 512 go through inverted 512 x 512 diagonal blocks (k_trtri_diag
 * and GEMMs, n / 512 levels); 0 = 64-wide substitutions (n / 64 levels of k_trsm_diag + k_gemm_f64_t). */
/* Diagnostic builds (-DCLRS_FUSED_STAMPS) only: s_memtime stamps of the phases of workgroup 0 of the fused kernel. */
int clrs_debug_stamps(clrs_ctx *ctx, uint64_t out[64]);

/* Capture the per-iteration launch sequences into hipGraphs (1) or launch kernels one by one (0).  The default (null) stream cannot
 * be captured: with a caller's stream (clrs_set_stream) graph mode needs a stream of its own; calls fail with CLRS_ERR_STATE otherwise. */
int clrs_set_graph_mode(clrs_ctx *ctx, int enabled);

/* Name of the kernel that dominates the assembly for this context and the number of launches of one
 * assemble / factor / solve call (for profiling). */
int clrs_plan_info(const clrs_ctx *ctx, int32_t *n_launch_assemble, int32_t *n_launch_factor, int32_t *n_launch_solve);


/* =====================================================================================================================
 * The same path at the reference's working precision: multi-word fp64 ("limbs").
 *
 * The reference computes in Arb midpoints at `prec` bits (default 256: src/solver.jl:73,103; Cholesky on midpoints
 * src/tools.jl:59-107; products Arblib.approx_mul!, src/solver.jl:1125-1143) because the Schur complements of its
 * headline problems are not positive definite to fp64 accuracy (cohnelkies(8,15) fails at the first iterate in fp64 and
 * at 113 bits).  A clrs_mw_ctx runs the identical stages with every number an unevaluated sum of
 * `limbs` doubles (limbs = 2..6, 8, 10: ~104 / 157 / 209 / 262 / 315 / 420 / 525 bits); limbs = 5 covers the reference's default precision
 * (256), 6 its test at prec = 300, 10 the prec = 512 of its tutorial and example generators.
 *
 * Array format ("planar limbs"): an array of logical length len is limbs * len doubles, limb l of element i at
 * [l * len + i]; value_i = sum_l a[l * len + i], limb 0 the value rounded to fp64, |limb l+1| <= ulp(limb l).
 * Every layout of the fp64 API (xy layout, S layout, x-like vectors) is used unchanged for the logical array.
 * The problem description is the same clrs_sdp_desc (fp64 data: the sampled vectors, lambda, B, dense A_p are exact
 * doubles; the iterates and everything computed from them carry `limbs` words).
 * Return codes and failure semantics are those of the fp64 entry points they mirror.
 * ===================================================================================================================== */
typedef struct clrs_mw_ctx clrs_mw_ctx;

/* Replaces precompute_matrices_bilinear_pairings (src/solver.jl:985-1059) + the preallocation :298-317 for a solve at
 * `limbs` words per number. */
int clrs_mw_create(const clrs_sdp_desc *desc, int device, int limbs, clrs_mw_ctx **out);
/* The same with problem data beyond fp64: every `const double *` array of `desc` (B, term_lambda, term_vs, term_ws, dense_A)
 * is planar with `data_limbs` planes (1 or 2; plane length = the array's fp64 length).  The reference holds the sampled
 * problem at `prec` bits as well (convert_to_prec, src/interface.jl:1078-1112), and its headline problems need it: the
 * cohnelkies(8,15) SDP whose data are rounded to fp64 is a different, dual-infeasible problem. */
int clrs_mw_create_ex(const clrs_sdp_desc *desc, int data_limbs, int device, int limbs, clrs_mw_ctx **out);
/* The same with per-context choices instead of the process-wide clrs_config_set knobs (a field < 0, or opts == NULL: the knob's value):
 * exact_products 0 / 1 / 2 = pairing matrices through exact slice products on the matrix cores never / from 256 eligible blocks on / always;
 * refine 0 / 1 / 2 = iterative refinement of the solve stage off / one step (default) / one step with the correction in fewer limbs. */
typedef struct clrs_mw_options {
    int32_t exact_products;
    int32_t refine;
    int32_t pipeline;        /* factorisations of small matrices as a pipeline of workgroups: 0 never / 1 (default) the clusters' S_j of at most 32 rows, of 48 .. 64
                              * rows (the 64-row form; clrs_config_set("mw_pipeline64", 0) switches that form off) and Q from 9 rows on / 2 every S_j and Q of at
                              * most 64 / 32 rows, and at 8 and 10 limbs as well */
    int32_t refine_predictor; /* clrs_mw_ipm_*: 0 (default) the predictor's solve is one pass of products, the corrector's is refined; 1 both are refined */
    int32_t factor_limbs;    /* Mixed-precision iterative refinement: limbs of the FACTOR stage (L_j, L_j^-1, L^-1 B, Q, L_Q, L_Q^-1) and of the inverse-factor products of
                              * the solve stage; the residuals of the refinement step, S_j itself and the solution carry all `limbs`.  0 (default) = automatic: inside
                              * clrs_mw_ipm_* limbs - 1 for limbs = 5, 6 on the LDS-resident paths, while the measured first-pass accuracy (clrs_ipm_record.refine_bits)
                              * stays above one limb plus a margin, then all limbs; the stand-alone entry points (clrs_mw_schur_factor / _solve) use all limbs.
                              * `limbs` = never reduce; limbs - 1 (5, 6 limbs) = the reduced count in the stand-alone entry points as well */
    int32_t matmul_limbs;    /* The reference's `matmul_prec` keyword (src/solver.jl:125, 304, 312-313, 1125-1143): limbs of the products that form the pairing matrices
                              * (part_r = Y V, X^-1 V and bilinear_pairings = W^T part_r; here T = Y V, Z = chol(X)^-1 V, Z^T Z, V^T T) -- S_j is accumulated from them in all
                              * `limbs`, as the reference does at `prec`.  0 (default) = `limbs`; a smaller count is rounded up to the next on offer (from limbs / 2 up).
                              * With fewer limbs than `limbs` the exact slice products (exact_products) are off. */
    int32_t reserved[2];
} clrs_mw_options;
int clrs_mw_create_opts(const clrs_sdp_desc *desc, int data_limbs, int device, int limbs, const clrs_mw_options *opts, clrs_mw_ctx **out);
void clrs_mw_destroy(clrs_mw_ctx *ctx);
int clrs_mw_limbs(const clrs_mw_ctx *ctx);
int clrs_mw_get_dims(const clrs_mw_ctx *ctx, clrs_dims *dims);          /* logical lengths; dims->reserved = limbs */
/* number of unique sampled vectors of block b over all its sub-blocks (the union of rightvecs / leftvecs) */
int clrs_mw_get_unique_count(const clrs_mw_ctx *ctx, int32_t block, int32_t *n_unique);

/* approx_cholesky!(X_inv_blk, X_blk) for every block (src/solver.jl:388-399); 0 or b+1 */
int clrs_mw_cholesky_blocks(clrs_mw_ctx *ctx, const double *X, double *Xchol);
/* compute_S_integrated! (src/solver.jl:1062-1226) */
int clrs_mw_schur_assemble(clrs_mw_ctx *ctx, const double *Xchol, const double *Y, double *S_out, double *AY_out);
/* steps 3-4 of compute_T_decomposition! (src/solver.jl:1244-1279); 0, j+1 or n_clusters+1 */
int clrs_mw_schur_factor(clrs_mw_ctx *ctx);
int clrs_mw_get_factor(clrs_mw_ctx *ctx, double *L, double *LinvB, double *LQ);
int clrs_mw_debug_exact_stamps(clrs_mw_ctx *ctx, unsigned long long *out /* [16] */);   /* diagnostic: first call arms, later calls read the phase stamps of k_mws_pair */
int clrs_mw_debug_pipe_stamps(clrs_mw_ctx *ctx, unsigned long long *out /* [16 * 40] */);   /* diagnostic builds (-DCLRS_MW_STAMPS) only: DESIGN.md section 5.5 */
int clrs_mw_get_S(clrs_mw_ctx *ctx, double *S_out, double *AY_out);   /* S_j and A_Y of the last (device-pointer) assembly -> host; NULL pointers are skipped */
/* Linear dependencies of the constraints (the reference's preprocess!, src/pre_postprocessing.jl).
 * clrs_mw_constraint_gram: G_j = S_j(X = I, Y = I), entry (p, q) = sum_l <A_p, A_q> -- the Gram matrix of the cluster's constraint matrices -- in the planar S
 *   layout, by the context's own assembly kernels.  Only the staging buffers of the host-pointer entry points are written.
 * clrs_mw_free_gram: B^T B = sum_j B_j^T B_j, N x N column-major, planar [limbs][N * N] (nothing is written when N = 0).
 * clrs_mw_rank_reveal: diagonally pivoted Cholesky of `nmat` symmetric positive semidefinite matrices (host pointers; limbs 4, 5, 6, 8 or 10).  Matrix m is
 *   n[m] x n[m] column-major at offset sum_{m' < m} n[m']^2 of G, planar [limbs][sum n^2]; only indices < ncand[m] may become pivots; the elimination stops when
 *   the largest remaining candidate diagonal is <= tau[m].  Outputs: perm (concatenated, n[m] entries each: the pivots in pivot order, then the rest in original
 *   order), rank[m] = r, W (same offsets and planes as G: the r x (n - r) matrix G11^-1 G12, column-major with leading dimension r, in the first r (n - r)
 *   entries of the matrix's range) and resid (planar [limbs][sum n]: the remaining diagonal of the n - r non-pivots, in the first n - r entries of the range).
 * clrs_mw_constraint_dependencies: Gram + rank reveal per cluster (every constraint a candidate) without the Gram matrices leaving the device; tau [J], perm and
 *   resid in the x layout, rank [J], W in the planar S layout.  The context needs a new assembly before its next factorisation.
 * clrs_mw_gemm: a batch of independent products C <- beta C + alpha op(A) op(B) in `limbs` limbs (4, 5, 6, 8 or 10), one launch, no context (host pointers): the
 *   substitution of the preprocessing and any other product of matrices outside a context.  A, B, C are planar pools: limb l of element o of a pool is
 *   pool[l * plane + o], so a pool is limbs * plane doubles; A and B may be the same pool.  Job i: op(A) is m x k, op(B) is k x n, C is m x n; the matrices are
 *   column-major with leading dimensions lda, ldb, ldc at element offsets a_off, b_off, c_off of their pools (op = transpose when transa / transb is nonzero: A is
 *   then stored k x m); alpha is -1 or +1, beta is -1, 0 or +1 (exact scalings).  Every entry is summed in one fixed order (r ascending, one renormalisation, then
 *   one multi-word add of beta C), so results are reproducible bit for bit.  beta = 0 never reads C; rows m .. ldc - 1 of C are never written; k = 0 gives
 *   C <- beta C; m = 0 or n = 0 is a no-op.  CLRS_ERR_INVALID (message: clrs_last_error): limbs not on offer, alpha / beta out of range, a negative size or offset,
 *   a leading dimension smaller than the rows it holds, a matrix that leaves its plane, null pools with a non-empty job, or two jobs whose C ranges
 *   [c_off, c_off + (n - 1) ldc + m) overlap (the ranges as intervals: interleaved outputs are refused too).
 * clrs_mw_posv: the solution X of A X = B for a dense symmetric positive definite A in `limbs` limbs (4, 5, 6, 8 or 10), no context, host pointers (DESIGN.md
 *   section 26; the regularised normal equations of the reference's roundx, src/rounding.jl:537-568).  A is planar [limbs][a_plane]: an n x n column-major matrix
 *   of which only the lower triangle is read; B is [limbs][b_plane] and X [limbs][x_plane]: n x nrhs column-major, leading dimension n.  A left-looking blocked
 *   Cholesky with panels of 16 columns: the diagonal blocks by k_mw_posv_diag (one workgroup, L11 and its inverse from one elimination), every other step a
 *   product by the kernel of clrs_mw_gemm, the launches in a fixed order on one stream, so results are reproducible bit for bit and the columns of X do not
 *   depend on nrhs.  info[0] = 0, or 1 + j with j the first column whose pivot was not positive (or not finite): the first n nrhs entries of every plane of X
 *   are then 0.  info[1]: the number of panels.  Only those entries of X and info[0 .. 1] are written.  n = 0 or nrhs = 0 touches nothing.  CLRS_ERR_INVALID
 *   before any device call, outputs untouched: limbs not on offer, n < 0 or nrhs < 0, a_plane < n n, b_plane or x_plane < n nrhs, a null pointer with
 *   n nrhs > 0.  Every device buffer of the call is released on every path.
 * clrs_mw_posv_times: the device times of this thread's last clrs_mw_posv in milliseconds: the diagonal launches, the product launches (the rest of the span)
 *   and the span from the first launch to the last.  The events around the diagonal launches are recorded only in calls made after this thread's first
 *   clrs_mw_posv_times (until then diag_ms is 0 and gemm_ms the whole span): a call that nobody times records two events.
 * clrs_mw_kernel_vectors: kernel vectors of the PSD blocks of a solution (step 1 of the reference's exact_solution, detecteigenvectors, src/rounding.jl:575-642;
 *   DESIGN.md section 12), host pointers, no context.  X and Y are planar [limbs][plane] in the xy layout: block b is n[b] x n[b] column-major at offset
 *   sum_{b' < b} n[b']^2 (plane >= sum n^2).  Per block one branch, chosen from limb plane 0: dual (branch[b] = 1) when use_dual != 0 and max |X_b| <= dual_max
 *   (the caller passes 1 / sqrt(kernel_round_errbound)): X_b is eliminated by the diagonally pivoted elimination of clrs_mw_rank_reveal (every index a candidate,
 *   stop at pivots <= tau = kernel_errbound), rank r, count[b] = r vectors, vector c has 1 at perm[c], W[c, a] at perm[r + a], 0 at the other pivots; primal
 *   (branch[b] = 0) otherwise: Y_b is eliminated, rank r, count[b] = n - r vectors, vector a has 1 at perm[r + a], -W[c, a] at perm[c], 0 at the other
 *   non-pivots.  Outputs: perm (concatenated, n[b] entries each) and rank[b] of the eliminated matrix; V (planar [limbs][plane], block b at its offset): the
 *   vectors as an n[b] x count[b] column-major matrix in the original index order -- the entries of V outside it are left as they were passed in; resid_max and
 *   v_max ([sum n], block b at offset sum_{b' < b} n[b'], count[b] entries each, 0 behind them): per vector max_i |head (Y_b V_b)[i, v]| -- the product by the
 *   kernel of clrs_mw_gemm in its fixed summation order, so clrs_mw_gemm on the returned vectors restates it bit for bit -- and max_i |head V_b[i, v]|; pivot_resid
 *   (planar [limbs][sum n]): the remaining diagonal of the n - r non-pivots of the eliminated matrix, as clrs_mw_rank_reveal returns it.  CLRS_ERR_INVALID before
 *   anything is launched: limbs not on offer, a negative count, size or plane, blocks that leave their plane, a null pointer, tau <= 0 (or NaN), and the size
 *   limit of clrs_mw_rank_reveal.
 * clrs_mw_rationalize: the first `count` numbers of a planar pool v [limbs][plane] rounded to rationals by continued fractions (what the
 *   reference's roundx -> clindep does per entry for the field QQ, src/rounding.jl:470-512).  Per number: the convergents p_k / q_k of |v|, the first with
 *   |q_k |v| - p_k| < errbound (evaluated in `limbs` limbs from v itself); num = +-p_k (the sign of v), den = q_k >= 1, exact integers in fp64.  status 0: found;
 *   1: no convergent with p, q < 2^53 meets the bound within 96 steps; 2: the head of v is NaN or Inf (1 and 2: num = den = 0).  vq [limbs][plane]: num / den in
 *   `limbs` limbs (0 where den = 0).  Entry i < count of num, den, status and of every plane of vq is written and nothing behind them.  CLRS_ERR_INVALID before
 *   anything is launched: limbs not on offer, count < 0, plane < count, a null pointer with count > 0, errbound <= 0 (or NaN).
 * clrs_mw_kernel_vectors_rational: clrs_mw_kernel_vectors (the same arguments, steps and outputs, bit for bit) followed on the device by the rounding of every
 *   entry of every vector with errbound = round_errbound (the reference's kernel_round_errbound) and by the reference's second check (src/rounding.jl:630-639).
 *   Further outputs, in the layout of V (block b at its offset, n[b] x count[b] column-major; what the vectors do not cover is left as passed in): num, den
 *   ([plane]), status ([plane]), Vq ([limbs][plane]: the rounded vectors num / den), and round_resid_max ([sum n], the layout of resid_max): per vector
 *   max_i |head (Y_b Vq_b)[i, v]|, the product again by the kernel of clrs_mw_gemm.  CLRS_ERR_INVALID as for clrs_mw_kernel_vectors, and for
 *   round_errbound <= 0 (or NaN) or a null output.
 * clrs_modp_rref: the reduced row-echelon form of a matrix over the field of integers mod a prime p, 2 <= p < 2^23 (what the reference's
 *   find_pivots_modular asks of Nemo.rref, src/rounding.jl:313-333), host pointers, no context.  A: nrows x ncols row-major, residues in [0, p).  pivots has
 *   capacity min(nrows, ncols): its first *rank entries receive the 0-based pivot columns, ascending; the entries behind them stay as passed in.  R, where not
 *   null, receives the reduced row-echelon form (row-major, residues in [0, p), the pivot rows first in pivot order, rows >= *rank zero).  The arithmetic is
 *   exact, so the result is the unique reduced row-echelon form and reproducible bit for bit.  An empty matrix gives *rank = 0 and touches nothing else.
 *   CLRS_ERR_INVALID before anything is allocated or launched: a negative size, nrows * ncols >= 2^31, p < 2, p >= 2^23 or p composite, a null A, pivots or
 *   rank with a non-empty matrix, a residue outside [0, p).  Every device buffer is released on every path.
 * clrs_modp_dixon_lift: the p-adic lifting of Dixon's exact solve of the integer system A x = b, A n x n (what the reference asks of
 *   Nemo._solve_dixon, src/rounding.jl:274, 351, 360), host pointers, no context.  Integers are balanced base-2^24 digits, little-endian, every digit in
 *   [-2^23, 2^23): A_digits is [nd][n][n] (row-major planes), b_limbs [nbl][n].  On the device: C = A^-1 mod p (the elimination of clrs_modp_rref on
 *   [A mod p | I]), r_0 = b, and `steps` times x_k = C (r_k mod p) mod p, r_{k+1} = (r_k - A x_k) / p, the division exact.  X ([steps][n]) receives the x_k,
 *   residues in [0, p); r_limbs ([nrl][n], nrl = max(nbl, nd + 1) + 1) the last residual, so that A sum_k x_k p^k = b - p^steps r exactly.  info[0]: the rank
 *   of A mod p; info[1]: the steps done, 0 when the rank is below n (then the call returns 0 with X and r_limbs untouched: the caller takes another prime),
 *   else `steps`; info[2]: divisions that left a remainder; info[3]: residuals that left their limbs.  Either of the last two non-zero: CLRS_ERR_HIP (they
 *   cannot be, for digits and limbs as described).  n = 0 returns at once with rank 0.  CLRS_ERR_INVALID before anything is allocated: n < 0 or n > 32767,
 *   nd < 1, nbl < 1 (or more than 32767 limbs), steps < 0, p no prime in [2, 2^23), a digit outside [-2^23, 2^23), a null pointer with n > 0 (X may be null
 *   when steps = 0).  Every device buffer is released on every path.
 * clrs_modp_dixon_reconstruct: the rational reconstruction of the entries of a lifted solution, host pointers, no context.  X
 *   ([steps][n], residues in [0, p)) is what clrs_modp_dixon_lift returned; N_limbs (nN) and D_limbs (nD) are the bounds as little-endian digits in
 *   [0, 2^24).  Per entry i, on the device: x_i = sum_k X[k][i] p^k by Horner, then the half-extended Euclidean algorithm on (m = p^steps, x_i) stopped at the
 *   first remainder r <= N, with cofactor t (r = t x_i mod m).  Accepted (status[i] = 0) when 0 < |t| <= D and p does not divide both r and t (gcd(r, t)
 *   is a power of p): the entry is sign(t) r / |t|, num ([n][nl]) holds the digits in [0, 2^24) of r, den ([n][nl]) those of |t|, neg[i] = 1 when the
 *   numerator is negative.  Rejected (status[i] = 1): the rows of num and den are zero.  x_limbs, where not null, is [n][nx], nx >= the limbs of p^steps,
 *   and receives the digits of x_i.  info[0]: the limbs of p^steps; info[1]: the largest number of quotient steps of an entry (a quotient is taken in pieces
 *   of at most 24 bits, one step each); info[2]: their total, saturating at 2^31 - 1; info[3]: entries that met an impossibility (a negative remainder, a
 *   cofactor past its row, steps without end): non-zero gives CLRS_ERR_HIP.  n = 0 returns at once.  CLRS_ERR_INVALID before anything is allocated: n < 0
 *   or n > 32767, steps < 1 (or p^steps beyond 32767 limbs), p no prime in [2, 2^23), a null pointer (x_limbs may be null), nN, nD or nl outside
 *   [1, 32767], a digit outside [0, 2^24), nl below the limbs of max(N, D), a residue outside [0, p), nx too small.  Every device buffer is released on every path.
 * clrs_modp_dixon_reconstruct_times: the milliseconds the calling thread's last clrs_modp_dixon_reconstruct spent in its two kernels (Horner, Euclid).
 * clrs_modp_minors: the n leading principal minors of a symmetric integer matrix mod each of nprimes primes (the device half of an exact
 *   positive-definiteness check, what the reference's is_valid_solution asks of checkpd_cholesky, src/rounding.jl:367-415, 447-472), host pointers, no context.
 *   digits is [nd][n][n]: nd row-major planes of balanced base-2^24 digits, little-endian, every digit in [-2^23, 2^23], every plane symmetric.  primes holds
 *   nprimes distinct primes in [2, 2^23).  minors is [nprimes][n]: row q receives minor_1 .. minor_n mod primes[q], in [0, primes[q]), the running products of
 *   the pivots of the elimination L D L^T mod that prime, WITHOUT exchanges (leading minors do not survive them).  breakdown[q] is 0, or the 1-based order k of
 *   the first minor that is 0 mod primes[q]: row q is then valid up to and including position k, where it holds 0, and holds -1 behind it.  info[0]: the LDS
 *   bytes of a workgroup (one workgroup per prime, the matrix resident in LDS: hence n <= CLRS_MODP_MINORS_MAX_N); info[1]: workgroups launched; info[2]:
 *   primes that broke down; info[3]: impossibilities (a pivot or a minor that is no residue): non-zero gives CLRS_ERR_HIP and leaves minors and breakdown
 *   untouched.  CLRS_ERR_INVALID before any device call: n outside [1, 128], nd outside [1, 32767], nprimes outside [1, 65535], a null pointer, a digit outside
 *   [-2^23, 2^23], planes that are not symmetric, a modulus that is no prime in [2, 2^23), a repeated prime.  Every device buffer is released on every path.
 *   clrs_config_set("modp_minors_chunk_bytes", b): the primes are taken in chunks whose residues (8 n^2 bytes per prime) stay below b bytes (0, the default: 256 MiB).
 * clrs_modp_minors_times: the milliseconds of the calling thread's last clrs_modp_minors: in the residue kernel, in the L D L^T kernel, and from the first
 *   upload to the last download (device events).
 * clrs_modp_minors_field: clrs_modp_minors for a symmetric matrix over a number field QQ(g), M = sum_j M_j g^j with integer M_j (the
 *   device half of rounding.checkpd_field, where the reference's checkpd_cholesky(A; FF, g), src/rounding.jl:417-472, embeds at Arb balls), host pointers, no
 *   context.  deg in [2, 4] is the degree of the (monic) minimal polynomial f of g.  digits is [deg][nd][n][n]: the planes of M_0 .. M_(deg-1) as
 *   clrs_modp_minors takes them, every plane symmetric.  primes holds nprimes distinct primes in [2, 2^23) and roots ([nprimes][deg]) deg distinct numbers
 *   in [0, p) per prime: the roots of f mod p (the function does not check that they are; any distinct points give the minors of M evaluated there).
 *   minors is [nprimes][deg][n] and breakdown [nprimes][deg]: for the pair (prime q, root i) what clrs_modp_minors returns for the integer matrix
 *   sum_j M_j roots[q][i]^j mod primes[q], with the same conventions.  info as clrs_modp_minors, counted per pair: [1] = nprimes deg workgroups.
 *   CLRS_ERR_INVALID before any device call, nothing written: deg outside [2, 4], n outside [1, 128], nd outside [1, 32767], nprimes outside [1, 65535], a null
 *   pointer, a digit outside [-2^23, 2^23], a plane that is not symmetric, a modulus that is no prime in [2, 2^23), a repeated prime, a root outside [0, p),
 *   two equal roots of one prime.  The chunks of clrs_config_set("modp_minors_chunk_bytes", b) hold 8 n^2 deg bytes per prime.
 * clrs_modp_minors_field_times: the milliseconds of the calling thread's last clrs_modp_minors_field, as clrs_modp_minors_times gives them.
 * clrs_modp_field_frobenius: out ([nprimes][deg]) receives, per prime, the coefficients in [0, p) of x^p mod (f, p), f = sum_j minpoly[j] x^j of degree
 *   deg in [2, 4] (minpoly[deg] != 0), one lane per prime; -1 throughout where p divides minpoly[deg].  A prime that divides neither the leading coefficient
 *   nor the discriminant splits f into deg distinct linear factors iff the row is (0, 1, 0, ..).  nprimes in [1, 2^20]; the primes need not be distinct.
 *   CLRS_ERR_INVALID before any device call: deg, nprimes out of range, a null pointer, minpoly[deg] = 0, a modulus that is no prime in [2, 2^23).
 * clrs_modp_field_adjugate: the determinant and the adjugate of a square matrix over a number field, M = sum_j M_j g^j with integer M_j, at every (prime,
 *   root) pair (the device half of rounding.inverse_field, the reference's inv(B) of the basis change, src/rounding.jl:834-836), host
 *   pointers, no context.  deg, digits ([deg][nd][n][n], the planes NOT symmetric), primes and roots as clrs_modp_minors_field takes them, and the primes
 *   descending.  adj is [nprimes][deg][n][n]: matrix (q, i) receives det M(r) M(r)^-1 mod p in [0, p) for r = roots[q][i], p = primes[q], row-major; det
 *   ([nprimes][deg]) receives det M(r) mod p.  A pair whose matrix is singular mod p has det 0, adj -1 throughout and breakdown[q][i] = c + 1, c the first
 *   column that depends on the columns before it mod p; breakdown is 0 otherwise.  One workgroup per pair, the matrix resident in LDS, Gauss-Jordan with
 *   row exchanges (the first non-zero entry of a column among the rows not yet used); every output is independent of the pivots chosen.  info[0]: the LDS
 *   bytes of a workgroup; info[1]: workgroups launched (nprimes deg); info[2]: singular pairs; info[3]: impossibilities (a pivot, a determinant or an entry
 *   that is no residue): non-zero gives CLRS_ERR_HIP and leaves adj, det and breakdown untouched.  CLRS_ERR_INVALID before any device call, nothing
 *   written: deg outside [2, 4], n outside [1, 128], nd outside [1, 32767], nprimes outside [1, 65535], a null pointer, a digit outside [-2^23, 2^23], a
 *   modulus that is no prime in [2, 2^23), primes that do not descend (a repeated prime among them), a root outside [0, p), two equal roots of one prime.
 *   The chunks of clrs_config_set("modp_minors_chunk_bytes", b) hold 8 n^2 deg bytes of residues per prime.
 * clrs_modp_field_adjugate_times: the milliseconds of the calling thread's last clrs_modp_field_adjugate: in the residue kernel, in the Gauss-Jordan
 *   kernel, and from the first upload to the last download (device events).
 * clrs_zz_gemm: C = A B over the integers (the exact matrix arithmetic around the steps above: Gram matrices, normal equations, the
 *   checks A x == b), host pointers, no context.  A is [nda][m][k], B [ndb][k][n], C [ndc][m][n]: row-major planes of balanced base-2^24 digits, little-endian.
 *   Input digits lie in [-2^23, 2^23]; C receives the unique representation with every digit ((v + 2^23) mod 2^24) - 2^23.  info[0]: entries of C that do not
 *   fit in ndc digits: non-zero gives CLRS_ERR_INVALID and leaves C untouched; info[1]: ranges of digits of B the product was taken in (the (lo, hi) buffer of a
 *   range, 16 nda m n bytes per digit of B, stays below 256 MiB, or below clrs_config_set("zz_gemm_chunk_bytes", b); never less than one digit per range);
 *   info[2]: GEMM workgroups launched; info[3]: impossibilities (a flushed accumulator that is no integer, or of magnitude >= 2^53): non-zero gives
 *   CLRS_ERR_HIP and leaves C untouched.  CLRS_ERR_INVALID before any device call: a negative size, nda, ndb or ndc outside [1, 32767], an operand or result of
 *   2^31 elements or more (nda m and ndb n likewise, less one tile of 64), min(nda, ndb) k >= 2^30, a null pointer with a non-empty operand (info is always
 *   needed), a digit outside [-2^23, 2^23].  m, n or k equal to 0 gives zeros without touching a device.  Every device buffer is released on every path.
 * clrs_zz_gemm_times: the milliseconds of the calling thread's last clrs_zz_gemm: in the GEMM kernel, in the combine and carry kernels, and from the first
 *   upload to the last download (device events).
 * clrs_modp_dixon_lift_multi: clrs_modp_dixon_lift for a matrix of right-hand sides, A X = B with B n x m (the exact solve behind the
 *   inverse over QQ of the reference's basis_transformations, src/rounding.jl:836), host pointers, no context.  A_digits is [nd][n][n], B_limbs [nbl][n][m],
 *   X [steps][n][m] (residues in [0, p)), R_limbs [nrl][n][m] with nrl = max(nbl, nd + 1) + 1: per column j exactly what clrs_modp_dixon_lift gives for
 *   b = B[:, j].  Both products of a step are fp64 MFMA GEMMs (k_liftm_x: X_k = A^-1 R_k mod p; k_zz_gemm: A X_k as (lo, hi) pairs), the residual update is
 *   one thread per entry.  The columns are taken in chunks whose buffers (per column 16 nd n + 16 n + 4 (nrl + 1) n bytes) stay below 256 MiB, or below
 *   clrs_config_set("liftm_chunk_bytes", b); never less than one column per chunk; the result does not depend on the chunks.  info (6 ints): [rank of A mod p,
 *   steps done, divisions that left a remainder, residuals that left their limbs, chunks of columns, GEMM pairs found impossible]; a non-zero count in
 *   info[2], info[3] or info[5] gives CLRS_ERR_HIP.  rank < n: no error, nothing lifted, X and R_limbs untouched.  CLRS_ERR_INVALID before any device call,
 *   outputs untouched: what clrs_modp_dixon_lift refuses, m < 0, an operand or result (nd n^2, nbl n m, steps n m, (nrl + 1) n m) of 2^31 elements or more.
 *   n == 0 or m == 0: nothing to lift, info = [0, steps, 0, 0, 0, 0] without touching a device (the rank of A is then not examined).  Every device buffer is
 *   released on every path.
 * clrs_modp_dixon_lift_multi_times: the milliseconds of the calling thread's last clrs_modp_dixon_lift_multi: in k_liftm_x, in k_zz_gemm and in k_liftm_r
 *   over all steps and chunks, and from the first upload to the last download (device events).
 * clrs_zz_lowrank_system: the rows of the rational linear system of the rounding chain from low-rank constraint matrices (the
 *   reference's partial_linearsystem, src/interface.jl:1354-1535, cleared of denominators), host pointers, no context.  U is [ndu][n][T], W [ndw][n][T]: one
 *   column per low-rank term, row-major planes of balanced base-2^24 digits, little-endian, digits in [-2^23, 2^23]; row i of the system owns the terms
 *   rowptr[i] .. rowptr[i + 1] - 1 (rowptr has R + 1 entries, non-decreasing, from 0 to T); column c is the pair (col_a[c], col_b[c]), 0 <= a <= b < n.
 *   C [ndc][R][nc] receives C[i, c] = 2^(a != b) sum_t U[a, t] W[b, t] in the unique digits of clrs_zz_gemm.  The digit index lies in the k-extent of the
 *   fp64 MFMA (k_lrsys_tile: one workgroup per row and 16 x 16 tile of pairs that holds a selected column), int64 digit sums, one carry walk per entry.  info[0]:
 *   entries that do not fit in ndc digits: non-zero gives CLRS_ERR_INVALID and leaves C untouched; info[1]: chunks of rows (the sums of a chunk,
 *   8 (ndu + ndw - 1) nc bytes per row, stay below 256 MiB, or below clrs_config_set("lrsys_chunk_bytes", b); never less than one row per chunk; the result
 *   does not depend on the chunks); info[2]: tile workgroups launched; info[3]: impossibilities as in clrs_zz_gemm: non-zero gives CLRS_ERR_HIP and leaves C
 *   untouched.  CLRS_ERR_INVALID before any device call, C untouched: a negative size, ndu, ndw or ndc outside [1, 32767], U, W, C, n^2 or
 *   (ndu + ndw - 1) nc of 2^31 elements or more, a null pointer (rowptr and info are always needed), a rowptr that does not start at 0, end at T or that
 *   decreases, (most terms of a row) min(ndu, ndw) >= 2^14, a pair with a > b or an index outside [0, n), a digit outside [-2^23, 2^23].  R, nc or T equal to
 *   0 gives zeros without touching a device; a row without terms is a row of zeros.  Every device buffer is released on every path.
 * clrs_zz_lowrank_system_times: the milliseconds of the calling thread's last clrs_zz_lowrank_system: in k_lrsys_tile, in k_lrsys_carry, and from the first
 *   upload to the last download (device events).
 * clrs_zz_lll: LLL reduction of a batch of nb independent integer lattices (the reduction of the kernel vectors of the rounding chain,
 *   the reference's simplify_kernelvectors / reduction_step, src/rounding.jl:860-1104), host pointers, no context.  Lattice b is given by rows[b] <= 128
 *   independent rows of cols[b] <= 256 columns in nd <= 20 planes of balanced base-2^24 digits, [nd][rows[b]][cols[b]] row-major, little-endian, digits in
 *   [-2^23, 2^23], the lattices packed one after the other in in_digits; out_digits has the same layout and receives the reduced rows of the lattices that
 *   end with status 0 (nothing else of it is written).  Dot products run over the first cols_gram[b] columns only, row operations act on all columns (an
 *   identity appended behind cols_gram columns comes back as the transformation).  One workgroup of 256 threads per lattice.  The rows change by exact
 *   integer operations only (b_k <- b_k - X b_j with an integer X, and exchanges); the Gram-Schmidt data that choose them are floating point of `limbs` fp64
 *   words (2, 4 or 6), size reduction to |mu| <= eta and Lovasz's test with delta.  info is [nb][8]: info[b][0] the status -- 0 reduced; 1 a cap was reached
 *   (max_swaps exchanges, or 64 size-reduction passes at one index); 2 the arithmetic gave up (a diagonal r_kk that is not positive and finite, a non-finite
 *   value, a pass of quotients that did not shrink the row of mu): more limbs may help, the rows may be dependent; 3 an entry left its nd digits --
 *   info[b][1] exchanges, info[b][2] size-reduction passes, info[b][3] launches, info[b][4] the index reached.  A launch takes at most 1024 exchanges per
 *   lattice, or clrs_config_set("lll_launch_swaps", n), then the host launches again; the result does not depend on n.  CLRS_ERR_INVALID before any device
 *   call, outputs untouched: a negative size, more than 128 rows or 256 columns, cols_gram outside [0, cols] (or 0 for a lattice with rows), nd outside
 *   [1, 20], limbs other than 2, 4, 6, delta outside (1/4, 1], eta outside [1/2, sqrt(delta)), max_swaps < 0, planes of 2^31 elements or more, a null
 *   pointer, a digit outside [-2^23, 2^23].  nb == 0 touches nothing; a batch whose lattices all have 0 rows gives status 0 without touching a device.
 *   Every device buffer is released on every path.
 * clrs_zz_lll_times: the milliseconds of the calling thread's last clrs_zz_lll: in k_zz_lll over all launches, and from the first upload to the last
 *   download (device events).
 * clrs_mw_field_round: round `count` multi-word numbers to the number field QQ(g) of degree deg = 2 .. 4 by integer relations (the
 *   reference's roundx(x, g, deg) -> clindep -> lindep per entry of a kernel vector, src/rounding.jl:481-534), host pointers, no context: the degree-d
 *   counterpart of clrs_mw_rationalize.  gpow is planar [limbs][deg], limb l of g^k at gpow[l * deg + k]; v planar [limbs][plane].  Per number the first
 *   rung p = 1, 6, 11, .. <= min(bits, 53 limbs - 16) at which the first row a of an LLL-reduced basis ((delta, eta) = (0.99, 0.51)) of the lattice
 *   [I | floor(2^p (v, 1, g, .., g^(deg-1)))] has |a_0 v + a_1 + a_2 g + .. + a_deg g^(deg-1)| < errbound, that quantity evaluated in `limbs` limbs from the
 *   numbers as given.  The lattice of a rung is the reduced basis of the rung before with its last column carried five bits further (exact integers of nd
 *   balanced base-2^24 digits; one lane per number, the state in a lane-strided workspace).  rel is [nd][deg + 1][plane] int32: digit s of a_k of number i
 *   at rel[(s * (deg + 1) + k) * plane + i]; status [plane]: 0 found; 1 no rung gave a relation; 2 a limb of v is NaN or Inf; 3 the Gram-Schmidt data were
 *   unusable or a cap was hit (64 size-reduction passes per visit, 4096 exchanges per rung); 4 an entry left its nd digits, or |v| >= 2^22; 5 the accepted
 *   relation has a_0 = 0 (the powers of g are dependent to this accuracy).  rung [plane]: the bits of the rung the number ended at; err [plane]: the
 *   residual there (0 for statuses 2, 3, 4); vq planar [limbs][plane]: -(a_1 + a_2 g + ..) / a_0 for status 0, else 0; info [2][plane]: exchanges, rungs
 *   visited.  rel is 0 unless the status is 0 or 5.  Entry i < count of every plane is written and nothing behind them.  A launch advances a number by at
 *   most 16 rungs, or clrs_config_set("field_round_launch_rungs", n), then the host launches again; the result does not depend on n.  CLRS_ERR_INVALID before
 *   any device call, outputs untouched: limbs other than 4, 5, 6, 8, 10, deg outside [2, 4], count < 0, plane < count, errbound not positive, bits < 1, nd
 *   outside [1, 20], a null pointer with count > 0, a power of g that is not finite or not below 2^22.  count == 0 touches nothing.  Every device buffer is
 *   released on every path.
 * clrs_mw_kernel_vectors_field: clrs_mw_kernel_vectors with the same arguments and the same outputs, bit for bit, followed on the device by
 *   clrs_mw_field_round (deg, gpow, bits, nd, errbound = round_errbound) of every entry of every vector and by the reference's second check Y_b Vq_b
 *   (src/rounding.jl:630-639) by the kernel of clrs_mw_gemm: the shape of clrs_mw_kernel_vectors_rational, whose scaffold it shares.  rel [nd][deg + 1][plane],
 *   status, rung, err [plane], info [2][plane] and Vq [limbs][plane] are pools over the plane like V: the entries of the vectors (block b: n_b x count_b from
 *   its offset, column-major) are written, everything else comes back as it went.  round_resid_max [sum n]: per vector max_i |head (Y_b Vq_b)[i, v]|.
 *   CLRS_ERR_INVALID as for clrs_mw_kernel_vectors, and for round_errbound not positive, deg outside [2, 4], bits < 1, nd outside [1, 20], a null output,
 *   a power of g that is not finite or not below 2^22.
 * clrs_mw_field_round_times: the milliseconds of the calling thread's last clrs_mw_field_round: in k_mw_field_round over all launches, and from the first
 *   upload to the last download (device events).
 * clrs_mw_minpoly: for each of `count` multi-word numbers v an integer polynomial of degree deg = 1 .. 4 with root v, by an integer relation among the
 *   number's own powers (the reference's min_poly(v, d) -> clindep -> lindep, src/find_field.jl:111-113, src/rounding.jl:481-509):
 *   the numeric core of find_field.  Host pointers, no context; v planar [limbs][plane].  The powers u = (1, v, v^2, .., v^deg) are formed once by the
 *   multi-word product, u_k = u_(k-1) v.  Per number the first rung p = 1, 6, 11, .. <= min(bits, 53 limbs - 16) at which the first row a of an
 *   LLL-reduced basis ((delta, eta) = (0.99, 0.51)) of [I | floor(2^p u)] has |a_0 + a_1 u_1 + .. + a_deg u_deg| < errbound, evaluated in `limbs` limbs
 *   from the powers as formed.  The ladder, the lattice arithmetic, the caps and the workspace discipline are those of clrs_mw_field_round; the digits of
 *   the fixed-point images of the powers are the lane's own.  rel is [nd][deg + 1][plane] int32, coefficients low to high: digit s of a_k of number i at
 *   rel[(s * (deg + 1) + k) * plane + i]; status [plane]: 0 found; 1 no rung gave a relation; 2 a limb of v is NaN or Inf; 3 the Gram-Schmidt data were
 *   unusable or a cap was hit; 4 an entry left its nd digits, or a power has |u_k| >= 2^22; 5 the accepted relation has a_deg = 0 or a_0 = 0 (v satisfies a
 *   relation of lower degree to this accuracy, or is 0).  rung [plane]: the bits of the rung the number ended at; err [plane]: the residual there (0 for
 *   statuses 2, 3, 4); info [2][plane]: exchanges, rungs visited.  rel is 0 unless the status is 0 or 5.  Entry i < count of every plane is written and
 *   nothing behind them.  Launches are cut as for clrs_mw_field_round (clrs_config_set("field_round_launch_rungs", n)); the result does not depend on n.
 *   CLRS_ERR_INVALID before any device call, outputs untouched: limbs other than 4, 5, 6, 8, 10, deg outside [1, 4], count < 0, plane < count, errbound
 *   not positive, bits < 1, nd outside [1, 20], a null pointer with count > 0.  count == 0 touches nothing.  Every device buffer is released on every path.
 * clrs_mw_minpoly_times: the milliseconds of the calling thread's last clrs_mw_minpoly: in k_mw_minpoly over all launches, and from the first upload to
 *   the last download (device events). */
#define CLRS_MODP_MINORS_MAX_N 128
int clrs_mw_constraint_gram(clrs_mw_ctx *ctx, double *G_out);
int clrs_mw_free_gram(clrs_mw_ctx *ctx, double *Q_out);
int clrs_mw_rank_reveal(int device, int limbs, int nmat, const int32_t *n, const int32_t *ncand, const double *G, const double *tau, int32_t *perm, int32_t *rank,
                        double *W, double *resid);
int clrs_mw_constraint_dependencies(clrs_mw_ctx *ctx, const double *tau, int32_t *perm, int32_t *rank, double *W, double *resid);
typedef struct clrs_mw_gemm_job {
    int32_t m, n, k, transa, transb, alpha, beta, lda, ldb, ldc;
    int64_t a_off, b_off, c_off;
} clrs_mw_gemm_job;
int clrs_mw_gemm(int device, int limbs, int njobs, const clrs_mw_gemm_job *jobs, const double *A, int64_t a_plane, const double *B, int64_t b_plane, double *C,
                 int64_t c_plane);
int clrs_mw_posv(int device, int limbs, int n, int nrhs, const double *A, int a_plane, const double *B, int b_plane, double *X, int x_plane, int32_t *info);
int clrs_mw_posv_times(double *diag_ms, double *gemm_ms, double *whole_ms);
int clrs_mw_kernel_vectors(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual, double dual_max,
                           int32_t *branch, int32_t *perm, int32_t *rank, int32_t *count, double *V, double *resid_max, double *v_max, double *pivot_resid);
int clrs_mw_rationalize(int device, int limbs, int count, const double *v, int plane, double errbound, double *num, double *den, int32_t *status, double *vq);
int clrs_mw_kernel_vectors_rational(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual,
                                    double dual_max, double round_errbound, int32_t *branch, int32_t *perm, int32_t *rank, int32_t *count, double *V,
                                    double *resid_max, double *v_max, double *pivot_resid, double *num, double *den, int32_t *status, double *Vq,
                                    double *round_resid_max);
int clrs_modp_rref(int device, int nrows, int ncols, int p, const int32_t *A, int32_t *pivots, int32_t *rank, int32_t *R);
int clrs_modp_dixon_lift(int device, int n, int p, int nd, const int32_t *A_digits, int nbl, const int32_t *b_limbs, int steps, int32_t *X, int32_t *r_limbs,
                         int32_t *info);
int clrs_modp_dixon_reconstruct(int device, int n, int p, int steps, const int32_t *X, int nN, const int32_t *N_limbs, int nD, const int32_t *D_limbs, int nl,
                                int32_t *num, int32_t *den, int32_t *neg, int32_t *status, int nx, int32_t *x_limbs, int32_t *info);
int clrs_modp_dixon_reconstruct_times(double *horner_ms, double *euclid_ms);
int clrs_modp_minors(int device, int n, int nd, const int32_t *digits, int nprimes, const int32_t *primes, int32_t *minors, int32_t *breakdown, int32_t *info);
int clrs_modp_minors_times(double *residues_ms, double *ldl_ms, double *total_ms);
int clrs_modp_minors_field(int device, int n, int deg, int nd, const int32_t *digits, int nprimes, const int32_t *primes, const int32_t *roots, int32_t *minors,
                           int32_t *breakdown, int32_t *info);
int clrs_modp_minors_field_times(double *residues_ms, double *ldl_ms, double *total_ms);
int clrs_modp_field_frobenius(int device, int deg, const int64_t *minpoly, int nprimes, const int32_t *primes, int32_t *out);
int clrs_modp_field_adjugate(int device, int n, int deg, int nd, const int32_t *digits, int nprimes, const int32_t *primes, const int32_t *roots, int32_t *adj,
                             int32_t *det, int32_t *breakdown, int32_t *info);
int clrs_modp_field_adjugate_times(double *residues_ms, double *gj_ms, double *total_ms);
int clrs_zz_gemm(int device, int m, int k, int n, int nda, const int32_t *A, int ndb, const int32_t *B, int ndc, int32_t *C, int32_t *info);
int clrs_zz_gemm_times(double *gemm_ms, double *combine_ms, double *whole_ms);
int clrs_modp_dixon_lift_multi(int device, int n, int m, int p, int nd, const int32_t *A_digits, int nbl, const int32_t *B_limbs, int steps, int32_t *X,
                               int32_t *R_limbs, int32_t *info);
int clrs_modp_dixon_lift_multi_times(double *x_ms, double *gemm_ms, double *r_ms, double *whole_ms);
int clrs_zz_lowrank_system(int device, int n, int T, int R, const int32_t *rowptr, int ndu, const int32_t *U, int ndw, const int32_t *W, int nc,
                           const int32_t *col_a, const int32_t *col_b, int ndc, int32_t *C, int32_t *info);
int clrs_zz_lowrank_system_times(double *tile_ms, double *carry_ms, double *whole_ms);
int clrs_zz_lll(int device, int nb, const int32_t *rows, const int32_t *cols, const int32_t *cols_gram, int nd, const int32_t *in_digits, int32_t *out_digits,
                double delta, double eta, int limbs, int max_swaps, int32_t *info);
int clrs_zz_lll_times(double *kernel_ms, double *whole_ms);
int clrs_mw_field_round(int device, int limbs, int deg, const double *gpow, int count, const double *v, int plane, int bits, double errbound, int nd,
                        int32_t *rel, int32_t *status, int32_t *rung, double *err, double *vq, int32_t *info);
int clrs_mw_field_round_times(double *kernel_ms, double *whole_ms);
int clrs_mw_minpoly(int device, int limbs, int deg, int count, const double *v, int plane, int bits, double errbound, int nd, int32_t *rel, int32_t *status,
                    int32_t *rung, double *err, int32_t *info);
int clrs_mw_minpoly_times(double *kernel_ms, double *whole_ms);
int clrs_mw_kernel_vectors_field(int device, int limbs, int nblk, const int32_t *n, const double *X, const double *Y, int plane, double tau, int use_dual,
                                 double dual_max, double round_errbound, int deg, const double *gpow, int bits, int nd, int32_t *branch, int32_t *perm,
                                 int32_t *rank, int32_t *count, double *V, double *resid_max, double *v_max, double *pivot_resid, int32_t *rel, int32_t *status,
                                 int32_t *rung, double *err, double *Vq, int32_t *info, double *round_resid_max);
/* the solve stage of compute_search_direction! (src/solver.jl:1527-1582) */
int clrs_mw_schur_solve(clrs_mw_ctx *ctx, const double *rhs_x, const double *rhs_y, double *dx, double *dy);

/* device-pointer variants: planar device arrays, enqueue on the context stream, no synchronisation.
 * clrs_mw_schur_assemble_dev uses the reciprocal Cholesky diagonals the last clrs_mw_cholesky_blocks_dev left in the
 * context; a caller that brings factors of X from elsewhere calls clrs_mw_set_xchol_dev first. */
int clrs_mw_cholesky_blocks_dev(clrs_mw_ctx *ctx, const double *d_X, double *d_Xchol);
int clrs_mw_sync_status_cholesky(clrs_mw_ctx *ctx);
int clrs_mw_set_xchol_dev(clrs_mw_ctx *ctx, const double *d_Xchol);
int clrs_mw_schur_assemble_dev(clrs_mw_ctx *ctx, const double *d_Xchol, const double *d_Y);
int clrs_mw_schur_factor_dev(clrs_mw_ctx *ctx);
int clrs_mw_sync_status(clrs_mw_ctx *ctx);
int clrs_mw_schur_solve_dev(clrs_mw_ctx *ctx, const double *d_rhs_x, const double *d_rhs_y, double *d_dx, double *d_dy);
double *clrs_mw_S_buffer_dev(clrs_mw_ctx *ctx);      /* planar S layout: S after assemble, L_j after factor */
double *clrs_mw_AY_buffer_dev(clrs_mw_ctx *ctx);     /* planar [T] */
void *clrs_mw_stream(clrs_mw_ctx *ctx);
int clrs_mw_set_stream(clrs_mw_ctx *ctx, void *hip_stream);

/* Cluster sharding (one process per GPU): a context created from the description of ITS clusters only (all N
 * free variables) is told its place with clrs_mw_set_shard.  The two sums over all clusters, Q = sum_j LinvB_j^T LinvB_j
 * (src/solver.jl:1268-1269) and u = sum_j LinvB_j^T t_j (:1550-1553), are formed from per-rank partial sums that are ALL-GATHERED
 * (limb planes cannot be all-reduced: a sum of limbs is not the limbs of the sum) and added in rank order by every rank, so all
 * ranks hold bit-identical Q, L_Q, dy.  Either the caller moves the slots (split-phase entry points; any transport), or the
 * library does it with RCCL on the context stream after clrs_mw_comm_init, in which case clrs_mw_schur_factor_dev and
 * clrs_mw_schur_solve_dev are collective calls: one all-gather of limbs*N*N doubles per factorisation, one of limbs*N per solve. */
int clrs_comm_unique_id(void *id128);                                     /* ncclGetUniqueId: 128 bytes, to be distributed by the caller */
int clrs_mw_set_shard(clrs_mw_ctx *ctx, int rank, int world);
int clrs_mw_comm_init(clrs_mw_ctx *ctx, const void *id128, int rank, int world);   /* clrs_mw_set_shard + ncclCommInitRank */
int clrs_mw_comm_destroy(clrs_mw_ctx *ctx);
/* Diagnostic (collective over the communicator): microseconds per all-gather of the three message sizes of one sharded iteration -- us[0] partial Q,
 * us[1] partial u, us[2] one scalar record -- from HIP events around `reps` exchanges back to back on the context's stream; info = rank, world, backend
 * (0 none, 1 RCCL, 2 in-process group).  bench.py reports them beside the N-GPU rate. */
int clrs_mw_comm_probe(clrs_mw_ctx *ctx, int reps, double us[3], int info[3]);
/* The interior-point iteration of a sharded context (clrs_mw_ipm_*) exchanges on two streams: a second communicator (a second unique
 * id, same rank and world) serves its side stream. */
int clrs_mw_comm_init_side(clrs_mw_ctx *ctx, const void *id128);
/* In-process stand-in for the communicators: `world` contexts of ONE process on ONE device, each driven by its own host thread (a
 * collective call blocks until every rank of the group has issued it).  For tests on a single GPU (RCCL refuses two ranks on one
 * device); the exchange is the same all-gather into rank-ordered slots. */
typedef struct clrs_mw_local_group clrs_mw_local_group;
int clrs_mw_local_group_create(int world, int device, clrs_mw_local_group **out);
void clrs_mw_local_group_destroy(clrs_mw_local_group *group);
int clrs_mw_comm_init_local(clrs_mw_ctx *ctx, clrs_mw_local_group *group, int rank);
int clrs_mw_schur_factor_local_dev(clrs_mw_ctx *ctx);                     /* L_j, LinvB_j, partial Q into slot `rank` */
double *clrs_mw_q_gather_dev(clrs_mw_ctx *ctx);                           /* [world][limbs * N * N] */
int clrs_mw_schur_factor_finish_dev(clrs_mw_ctx *ctx);                    /* Q = sum of the slots, Cholesky of Q */
int clrs_mw_schur_solve_fwd_dev(clrs_mw_ctx *ctx, const double *d_rhs_x);  /* t = L^-1 rhs_x, partial u into slot `rank` */
double *clrs_mw_u_gather_dev(clrs_mw_ctx *ctx);                           /* [world][limbs * N] */
int clrs_mw_schur_solve_bwd_dev(clrs_mw_ctx *ctx, const double *d_rhs_y, double *d_dx, double *d_dy);
/* The solve stage multiplies with explicit inverse factors and then takes one step of iterative refinement against the assembled S_j and B,
 * which gives (dx, dy) the backward error of the reference's substitutions (src/solver.jl:1538, 1557, 1567-1572) -- clrs_mw_schur_solve[_dev] do
 * both (clrs_mw_options.refine, or clrs_config_set("mw_refine", 0 / 1 / 2) before the context is created: no step / one step, the default / one step
 * with the correction in fewer limbs -- cheaper, and as good while twice the bits the products lose fit in those limbs: DESIGN.md section 5.5).
 * Split-phase callers: clrs_mw_schur_solve_bwd_dev leaves this rank's partial u' of the correction in slot `rank` of the u gather buffer; after ONE
 * MORE exchange of that buffer this call adds the correction to dx, dy (without it they are the plain products' solution). */
int clrs_mw_schur_solve_refine_dev(clrs_mw_ctx *ctx, const double *d_rhs_y, double *d_dx, double *d_dy);

/* HIP-event timings of the last calls, seconds: t[0] schur, t[1] cholS + LinvB (one kernel), t[2] 0, t[3] Q, t[4] cholQ,
 * t[5] last solve (the split compute_T_decomposition! returns, src/solver.jl:1282-1286). */
int clrs_mw_set_timing(clrs_mw_ctx *ctx, int enabled);
int clrs_mw_get_timings(clrs_mw_ctx *ctx, double t[6]);
/* algorithmic multi-word multiply-adds of one assembly / factorisation / solve */
int clrs_mw_get_counters(const clrs_mw_ctx *ctx, double *assemble_muladds, double *factor_muladds, double *solve_muladds);

/* The interior-point iteration around the path at the same precision (the loop body of solvesdp, src/solver.jl:348-589, as
 * clrs_ipm_* above but with every iterate and intermediate in `limbs` words; the step-length eigenvalue alone is taken in
 * fp64, as the reference's Float64 Lanczos does, src/solver.jl:1659).  C, c, b are fp64; x, y, X, Y of clrs_mw_ipm_get / _set
 * are planar limbs.  clrs_mw_ipm_create may be called again on the same context with other objective data.
 * Available when every PSD block fits in LDS at this limb count. */
int clrs_mw_ipm_create(clrs_mw_ctx *ctx, const clrs_ipm_data *data);
int clrs_mw_ipm_create_ex(clrs_mw_ctx *ctx, const clrs_ipm_data *data, int data_limbs);   /* C, c, b planar with data_limbs planes */
int clrs_mw_ipm_set_params(clrs_mw_ctx *ctx, const clrs_ipm_params *params);
int clrs_mw_ipm_init(clrs_mw_ctx *ctx, double omega_p, double omega_d);
int clrs_mw_ipm_set(clrs_mw_ctx *ctx, const double *x, const double *y, const double *X, const double *Y);   /* warm start, src/solver.jl:202-239 */
int clrs_mw_ipm_iterate(clrs_mw_ctx *ctx, clrs_ipm_record *out);
int clrs_mw_ipm_get(clrs_mw_ctx *ctx, double *x, double *y, double *X, double *Y);
int clrs_mw_ipm_objectives(clrs_mw_ctx *ctx, double *out /* [3 * limbs]: d_obj, p_obj, gap */);
/* Cluster-sharded iteration (one context per rank, each created from its own clusters and ALL free variables): the scalars that are sums,
 * maxima or minima over all clusters -- mu (src/solver.jl:369), the errors (:441-442), p = +-b - B^T x (:899-916), beta_c (:429), the step
 * lengths (:1684-1686), the objectives (:793-804) -- travel as one small record per rank and stage through all-gathers the library issues
 * itself and are reduced in rank order by every rank: x, X, Y stay sharded, y and every scalar are bit-identical on all ranks.  This call
 * supplies what a rank cannot know: the row count of X over all clusters, the cluster count of the whole problem, and the global numbers
 * (0-based) of its clusters / PSD blocks for failure codes (NULL: local numbers). */
int clrs_mw_ipm_set_global(clrs_mw_ctx *ctx, int rows_of_X_global, int clusters_global, const int32_t *cluster_ids, const int32_t *block_ids);
/* The whole loop with its termination test (src/solver.jl:348-589, 921-950) in one call: at most max_iterations iterations from the
 * current iterate, enqueued one ahead of the record the host waits for (the device evaluates the same test and freezes the iterate once
 * it holds, so the device never idles between iterations).  records[i] (i < max_records) = table row of the i-th iteration of this call;
 * *n_iter = iterations run; *error_code = 0, 1 / 3 / 4 as clrs_mw_ipm_iterate reports them, or 2 = max_iterations reached (:362-366). */
typedef struct clrs_ipm_stop {
    double duality_gap_threshold;                 /* with the error thresholds of clrs_ipm_params */
    int32_t need_dual_feasible, need_primal_feasible, max_iterations, reserved;
} clrs_ipm_stop;
int clrs_mw_ipm_solve(clrs_mw_ctx *ctx, const clrs_ipm_stop *stop, clrs_ipm_record *records, int max_records, int *n_iter, int *error_code);
/* The same loop with a callback per record: `on_record(record, user)` runs on the calling thread as the host reads the record of an iteration (the device
 * is one iteration further by then) -- the live iteration table of `verbose = true` (src/solver.jl:566-582) without giving up the one-call loop.  The
 * callback must not call into this context.  on_record and records may be NULL. */
typedef void (*clrs_ipm_record_fn)(const clrs_ipm_record *record, void *user);
int clrs_mw_ipm_solve_cb(clrs_mw_ctx *ctx, const clrs_ipm_stop *stop, clrs_ipm_record_fn on_record, void *user, clrs_ipm_record *records, int max_records, int *n_iter, int *error_code);
/* error_code of clrs_mw_ipm_iterate / clrs_mw_ipm_solve: 0; 1 / 3 / 4 as the reference's (docs/src/solving.md:64-70); 2 = max_iterations; and 5 = a wait
 * between the two streams of the iteration ran past its wall-clock bound (30 s: a hang, e.g. under a profiler that serialises kernels -- there, or to rule
 * it out, clrs_config_set("mw_stream_words", 0) / CLRS_MW_STREAM_WORDS=0 makes new contexts synchronise through events only); the iterate is not moved. */

const char *clrs_strerror(int code);
const char *clrs_last_error(void);
void clrs_set_last_error(const char *msg);   /* used by the library's own translation units */
const char *clrs_version(void);

/* Test hook: C = alpha * op(A) op(B) + beta * C through the grouped fp64 MFMA GEMM kernel
 * (host pointers).  Used by tests/ to check the kernel in isolation. */
int clrs_test_gemm(int device, int ta, int tb, int M, int N, int K, double alpha, const double *A, int lda,
                   const double *B, int ldb, double beta, double *C, int ldc);
/* Test hooks for the blocked dense kernels (host pointers, in place): lower Cholesky of an n x n
 * matrix (returns 0 or 1 on a non-positive pivot), and B <- L^-1 B / L^-T B. */
int clrs_test_potrf(int device, int n, double *A, int lda);
int clrs_test_trsm(int device, int trans, int n, int nrhs, const double *L, int ldl, double *B, int ldb);
/* Test hooks of the step length (src/solver.jl:1620-1693).
 * The three fp64 smallest-eigenvalue routines on matrices given to them: A holds `count` symmetric n x n matrices (column-major, both
 * triangles, back to back), out[count] receives their smallest eigenvalues; one launch, one workgroup per matrix.  form 0: the routine of the
 * multi-word step kernel for n <= 64 (2 <= n <= 64); form 1: its routine for larger blocks (1 <= n <= 128); form 2: the routine of the fp64
 * loop's step kernel (2 <= n <= 64).  Other sizes: CLRS_ERR_INVALID.  Domain: entries above about 2^-500 in magnitude, or zero (below, the
 * squares in x^T x underflow). */
int clrs_test_min_eig(int device, int form, int n, int count, const double *A, double *out);
/* The step-length stage of one multi-word iteration on matrices given to it (after clrs_mw_ipm_create; unsharded contexts): X, Y, dX, dY
 * (planar limbs, limbs x xy_len each) are uploaded into the iteration's buffers, the iteration's Cholesky launch and its step-length launches
 * run with the plan the context chose, and eig[2 * n_blocks] receives what they leave per block: lambda_min(L^-1 dM L^-T) - 1e-5 (dM / M
 * for 1 x 1 blocks, 0 for a block whose M is not positive definite), (X, dX) of every block first, then (Y, dY).  info[8] = {form of the
 * congruence (0: substitutions, 1: Y factored inside the launch, 2: inverse factors, 3: inverse factors through tiled products), W in LDS,
 * tiled products, column panels per congruence, limbs of the factors, failure flag, 0, 0}.  The iterate is overwritten: clrs_mw_ipm_init or
 * clrs_mw_ipm_set before the next solve. */
int clrs_mw_test_step_eig(clrs_mw_ctx *ctx, const double *X, const double *Y, const double *dX, const double *dY, double *eig, int32_t *info);

/* Measurement hook: average duration (us, HIP events, `reps` back-to-back launches) of a pure streaming kernel that reads
 * `read_bytes` (two streams) and writes `write_bytes` (one stream, non-temporal) of freshly allocated device memory: the rate a
 * bandwidth-bound kernel of that footprint and read : write mix can reach on this device.  bench.py reports the assembly kernel's
 * HBM traffic per second beside it (`roofline.copy_roof`). */
int clrs_test_stream(int device, long long read_bytes, long long write_bytes, int reps, double *avg_us);

#ifdef __cplusplus
}
#endif
#endif /* CLRS_HIP_H */

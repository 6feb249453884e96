# ClusteredLowRankHIP.jl -- thin ccall shim binding the reference's hot path to libclrs_hip.so.
#
# NOT a copy of the reference: it depends on ClusteredLowRankSolver.jl, converts its `ClusteredLowRankSDP`
# into the C description once per solve, and provides drop-in methods with the reference's names and
# argument meaning for the two functions on the path:
#
#     compute_T_decomposition!(sdp, S, A_Y, X_inv, Y, ..., cs_map; prec)        (src/solver.jl:1229-1287)
#     the "solve system" stage of compute_search_direction!                     (src/solver.jl:1527-1582)
#
# Host orchestration stays in Julia (Arb).  The device computes in multi-word fp64: a number is `limbs` doubles
# (limbs = 5 covers the reference's default prec = 256; include/clrs_hip.h, clrs_mw_*), an array is PLANAR,
# limb l of element i at [l * len + i].  At the boundary every Arb midpoint is split into its limbs (`limbs_of`),
# results come back as limbs and are summed into the caller's Arb buffers (`arb_of`); the problem data cross the
# boundary as 2 limbs (double-double).  `limbs = 1` selects the plain fp64 entry points (clrs_*), which cannot factor
# the 2d = 30 sphere-packing problems (DESIGN.md section 2).
# The exact solve of the rounding pipeline (`solve_dixon`, at the end of this file) takes and returns Nemo matrices.
# This file cannot be executed in the build container (no Julia there); INTEGRATION.md is the contract and
# tests/test_abi_cpu.py checks the struct below against include/clrs_hip.h.
module ClusteredLowRankHIP

using Libdl
using Arblib
import Nemo
import ClusteredLowRankSolver
const CLRS = ClusteredLowRankSolver

const libclrs = Ref{String}(get(ENV, "CLRS_HIP_LIB", "libclrs_hip.so"))

# struct clrs_sdp_desc (include/clrs_hip.h) -- field order and types must match the header
struct SdpDesc
    n_clusters::Int32
    n_free::Int32
    cluster_P::Ptr{Int32}
    B::Ptr{Float64}
    n_blocks::Int32
    block_cluster::Ptr{Int32}
    block_m::Ptr{Int32}
    block_delta::Ptr{Int32}
    block_kind::Ptr{Int32}
    term_ptr::Ptr{Int64}
    term_p::Ptr{Int32}
    term_r::Ptr{Int32}
    term_s::Ptr{Int32}
    term_rank::Ptr{Int32}
    term_lambda::Ptr{Float64}
    term_vec_ptr::Ptr{Int64}
    term_vs::Ptr{Float64}
    term_ws::Ptr{Float64}
    dense_ptr::Ptr{Int64}
    dense_p::Ptr{Int32}
    dense_A_ptr::Ptr{Int64}
    dense_A::Ptr{Float64}
end

# Limb planes of the problem data handed to the library: the reference holds the sampled problem at `prec` bits (convert_to_prec, src/interface.jl:1078-1112),
# so a solve at `limbs` words per number passes its data with `limbs` planes (clrs_mw_create_opts: data_limbs = 1, 2 or limbs); the fp64 entry points take one.
data_limbs_for(limbs::Integer) = limbs == 1 ? 1 : Int(limbs)

"""Device context + the host arrays that back the description (kept alive for the lifetime of the context)."""
mutable struct HipContext
    handle::Ptr{Cvoid}
    limbs::Int                  # 1: fp64 entry points (clrs_*); 2..6, 8, 10: multi-word entry points (clrs_mw_*)
    keep::Vector{Any}
    block_off::Vector{Int}      # offsets of the blocks (j,l) in the xy layout
    block_n::Vector{Int}
    jl::Vector{Tuple{Int,Int}}  # (j,l) of every block in description order
    cluster_P::Vector{Int}
    cluster_off::Vector{Int}
    S_off::Vector{Int}
    term_map::Vector{NTuple{5,Int}}   # (j,l,r,s,idx-in-A_Y[j][l][r,s]) of every term, in term order
    n_free::Int
end

check(code::Integer) = code < 0 ? error("clrs-hip: " * unsafe_string(ccall((:clrs_strerror, libclrs[]), Cstring, (Cint,), code)) *
                                        ": " * unsafe_string(ccall((:clrs_last_error, libclrs[]), Cstring, ()))) : Int(code)

f64(x) = Float64(Arblib.midref(x))

"""Limbs of the midpoint of `x`: successive roundings to Float64 (the subtraction is exact at the working precision)."""
function limbs_of!(out::AbstractMatrix{Float64}, i::Int, x, K::Int)
    r = Arb(x; prec=max(precision(x), 64 * K + 64))
    Arblib.get_mid!(r, r)
    for l in 1:K
        h = Float64(Arblib.midref(r))
        out[i, l] = h                      # column l of a (len x K) Julia matrix = limb plane l of the planar C array
        h == 0 && break
        Arblib.sub!(r, r, Arb(h; prec=precision(r)))
    end
    return out
end

"""Sum of the limbs of element `i` of a planar array as an Arb midpoint at precision `prec`."""
function arb_of(a::AbstractMatrix{Float64}, i::Int, prec::Int)
    r = Arb(0; prec=max(prec, 64 * size(a, 2) + 64))
    for l in size(a, 2):-1:1
        Arblib.add!(r, r, Arb(a[i, l]; prec=precision(r)))
    end
    out = Arb(r; prec)
    Arblib.get_mid!(out, out)
    return out
end

# struct clrs_mw_options (include/clrs_hip.h): a field < 0 = the library's process-wide default; matmul_limbs 0 = the context's limbs
struct MwOptions
    exact_products::Int32
    refine::Int32
    pipeline::Int32
    refine_predictor::Int32
    factor_limbs::Int32
    matmul_limbs::Int32
    reserved1::Int32
    reserved2::Int32
end

"""
    HipContext(sdp, cs_map; device=0, limbs=5, matmul_limbs=0)

Replaces `precompute_matrices_bilinear_pairings` (src/solver.jl:985-1059) and the preallocation block
(src/solver.jl:298-317): flattens `sdp.A[j][l][r,s][p]` (cluster-local constraint indices through `cs_map[j]`,
0-based) and `sdp.B[j]` into `clrs_sdp_desc` and creates the device context.  `limbs = limbs_for(prec)`; `matmul_limbs = limbs_for(matmul_prec)`
(the reference's keyword, src/solver.jl:125: the products that form the pairing matrices in fewer bits; 0 = `limbs`).
"""
function HipContext(sdp::CLRS.ClusteredLowRankSDP, cs_map; device::Integer=0, limbs::Integer=5, matmul_limbs::Integer=0)
    J = length(sdp.A)
    DL = data_limbs_for(limbs)
    cluster_P = Int32[size(sdp.c[j], 1) for j in 1:J]
    N = size(sdp.B[1], 2)
    # data arrays are collected as Arb and split into DL limb planes at the end
    Bv = Any[]
    for j in 1:J, k in 1:N, p in 1:cluster_P[j]
        push!(Bv, sdp.B[j][p, k])
    end
    bc = Int32[]; bm = Int32[]; bd = Int32[]; bk = Int32[]
    term_ptr = Int64[0]; tp = Int32[]; tr = Int32[]; ts = Int32[]; tk = Int32[]; tl = Any[]
    tvp = Int64[0]; tvs = Any[]; tws = Any[]
    dense_ptr = Int64[0]; dp = Int32[]; dAp = Int64[0]; dA = Any[]
    jl = Tuple{Int,Int}[]; block_n = Int[]; term_map = NTuple{5,Int}[]
    for j in 1:J, l in 1:length(sdp.A[j])
        Ajl = sdp.A[j][l]
        m = size(Ajl, 1)
        highrank = any(!(v isa CLRS.LowRankMat) for r in 1:m for s in 1:m for v in values(Ajl[r, s]))
        delta = 0
        push!(jl, (j, l)); push!(bc, j - 1); push!(bk, highrank ? 1 : 0)
        if highrank                                   # src/interface.jl:1001-1007: dense blocks have m == 1
            for p in sort(collect(keys(Ajl[1, 1])))
                M = Ajl[1, 1][p]
                delta = size(M, 1)
                push!(dp, cs_map[j][p] - 1)
                append!(dA, [M[a, b] for b in 1:delta for a in 1:delta])
                push!(dAp, length(dA))
            end
            m = 1
        else
            items = NTuple{4,Int}[]
            for r in 1:m, s in 1:m, p in keys(Ajl[r, s]), k in 1:length(Ajl[r, s][p].lambda)
                push!(items, (cs_map[j][p] - 1, r - 1, s - 1, k - 1))
            end
            sort!(items)
            inv_cs = Dict(v => k for (k, v) in cs_map[j])
            # position of a term's pairing in A_Y[j][l][r,s] (src/solver.jl:1152-1170): A_Y is filled in the order
            # `for p in keys(A[r,s]) for rnk`, so the index is the rank of (p, rnk) in that iteration order
            ay_pos = Dict{NTuple{4,Int},Int}()
            for r in 1:m, s in 1:m
                idx = 0
                for p in keys(Ajl[r, s]), k in 1:length(Ajl[r, s][p].lambda)
                    idx += 1
                    ay_pos[(r, s, cs_map[j][p], k)] = idx
                end
            end
            for (p0, r0, s0, k0) in items
                A = Ajl[r0+1, s0+1][inv_cs[p0+1]]
                delta = length(A.vs[k0+1])
                push!(tp, p0); push!(tr, r0); push!(ts, s0); push!(tk, k0); push!(tl, A.lambda[k0+1])
                append!(tvs, A.vs[k0+1]); append!(tws, A.ws[k0+1])     # Matrix(::LowRankMat) = sum lam * vs * ws' (src/interface.jl:798-800)
                push!(tvp, length(tvs))
                push!(term_map, (j, l, r0 + 1, s0 + 1, ay_pos[(r0 + 1, s0 + 1, p0 + 1, k0 + 1)]))
            end
        end
        push!(bm, m); push!(bd, delta); push!(block_n, m * delta)
        push!(term_ptr, length(tp)); push!(dense_ptr, length(dp))
    end
    planar(v) = (a = zeros(Float64, max(length(v), 1), DL); foreach(i -> limbs_of!(a, i, v[i], DL), eachindex(v)); a)
    Bflat, tlf, tvsf, twsf, dAf = planar(Bv), planar(tl), planar(tvs), planar(tws), planar(dA)
    keep = Any[cluster_P, Bflat, bc, bm, bd, bk, term_ptr, tp, tr, ts, tk, tlf, tvp, tvsf, twsf, dense_ptr, dp, dAp, dAf]
    desc = Ref(SdpDesc(J, N, pointer(cluster_P), pointer(Bflat), length(bc), pointer(bc), pointer(bm), pointer(bd), pointer(bk),
                       pointer(term_ptr), pointer(tp), pointer(tr), pointer(ts), pointer(tk), pointer(tlf), pointer(tvp),
                       pointer(tvsf), pointer(twsf), pointer(dense_ptr), pointer(dp), pointer(dAp), pointer(dAf)))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep begin
        if limbs == 1
            check(ccall((:clrs_ctx_create, libclrs[]), Cint, (Ref{SdpDesc}, Cint, Ref{Ptr{Cvoid}}), desc, device, h))
        else
            opts = Ref(MwOptions(-1, -1, -1, -1, -1, Int32(matmul_limbs), 0, 0))
            check(ccall((:clrs_mw_create_opts, libclrs[]), Cint, (Ref{SdpDesc}, Cint, Cint, Cint, Ref{MwOptions}, Ref{Ptr{Cvoid}}), desc, DL, device, limbs, opts, h))
        end
    end
    ctx = HipContext(h[], limbs, keep, cumsum([0; block_n .^ 2]), block_n, jl, Int.(cluster_P), cumsum([0; Int.(cluster_P)]),
                     cumsum([0; Int.(cluster_P) .^ 2]), term_map, N)
    finalizer(c -> ccall((c.limbs == 1 ? :clrs_ctx_destroy : :clrs_mw_destroy, libclrs[]), Cvoid, (Ptr{Cvoid},), c.handle), ctx)
    return ctx
end

"""Smallest limb count whose operations carry `prec` bits (about 53 K - K bits for K limbs)."""
limbs_for(prec::Integer) = prec <= 53 ? 1 : prec <= 104 ? 2 : prec <= 157 ? 3 : prec <= 209 ? 4 : prec <= 262 ? 5 : prec <= 315 ? 6 : prec <= 420 ? 8 : prec <= 525 ? 10 :
                           error("prec = $prec needs more than 10 limbs")

"""Pack a BlockDiagonal of BlockDiagonals of ArbRefMatrix into the planar xy layout (len x limbs, column-major per block)."""
function pack_xy(ctx::HipContext, M)
    out = zeros(Float64, ctx.block_off[end], ctx.limbs)
    for (b, (j, l)) in enumerate(ctx.jl)
        blk = M.blocks[j].blocks[l]
        n = ctx.block_n[b]
        for c in 1:n, r in 1:n
            limbs_of!(out, ctx.block_off[b] + r + (c - 1) * n, blk[r, c], ctx.limbs)
        end
    end
    return out
end

sym(ctx::HipContext, fp64::Symbol, mw::Symbol) = ctx.limbs == 1 ? fp64 : mw

"""
Drop-in for `compute_T_decomposition!` (src/solver.jl:1229-1287).  Same arguments; the Arb scratch arguments
(`bilinear_pairings_*`, `tempX`, `leftvecs`, ..., `part_r`) are accepted and ignored.  Writes `A_Y`, and -- so that a caller
who keeps the reference's own `compute_search_direction!` finds what it reads there (src/solver.jl:1537-1571) -- copies the
factors back into `S` (-> L_j), `LinvB` and `Q` (-> L_Q).  Callers that use `solve_system!` below can pass
`copy_factors=false` and leave the factors on the device.  Throws the reference's `SolverFailure`s.
"""
function compute_T_decomposition!(ctx::HipContext, sdp, S, A_Y, X_inv, Y, bilinear_pairings_Y=nothing, bilinear_pairings_Xinv=nothing,
                                  LinvB=nothing, Q=nothing, args...; prec=precision(S[1]), copy_factors::Bool=true)
    K = ctx.limbs
    Xc, Yf = pack_xy(ctx, X_inv), pack_xy(ctx, Y)
    T = length(ctx.term_map)
    AY = zeros(Float64, max(T, 1), K)
    lib = libclrs[]
    check(ccall((sym(ctx, :clrs_set_timing, :clrs_mw_set_timing), lib), Cint, (Ptr{Cvoid}, Cint), ctx.handle, 1))
    check(ccall((sym(ctx, :clrs_schur_assemble, :clrs_mw_schur_assemble), lib), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.handle, Xc, Yf, C_NULL, AY))
    for (t, (j, l, r, s, idx)) in enumerate(ctx.term_map)
        A_Y[j][l][r, s][idx, 1] = arb_of(AY, t, prec)
    end
    st = check(ccall((sym(ctx, :clrs_schur_factor, :clrs_mw_schur_factor), lib), Cint, (Ptr{Cvoid},), ctx.handle))
    J = length(S)
    if 0 < st <= J
        throw(CLRS.SolverFailure("S was not decomposed succesfully in block $st, try again with higher precision. If this occurred in the first iteration, remove linear dependencies in the PSD part of the constraints or turn preprocessing on."))
    elseif st == J + 1
        throw(CLRS.SolverFailure("Q was not decomposed correctly. Try restarting with a higher precision. If this occurred in the first iteration, remove linear dependencies between free variables or turn preprocessing on."))
    end
    if copy_factors
        N = ctx.n_free
        Lf = zeros(Float64, ctx.S_off[end], K)
        LBf = zeros(Float64, max(ctx.cluster_off[end] * N, 1), K)
        LQf = zeros(Float64, max(N * N, 1), K)
        check(ccall((sym(ctx, :clrs_get_factor, :clrs_mw_get_factor), lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    ctx.handle, Lf, N > 0 ? pointer(LBf) : C_NULL, N > 0 ? pointer(LQf) : C_NULL))
        lb_off = 0
        for j in 1:J
            P = ctx.cluster_P[j]
            for q in 1:P, p in 1:P
                S[j][p, q] = arb_of(Lf, ctx.S_off[j] + p + (q - 1) * P, prec)
            end
            if LinvB !== nothing
                for k in 1:N, p in 1:P
                    LinvB[j][p, k] = arb_of(LBf, lb_off + p + (k - 1) * P, prec)
                end
            end
            lb_off += P * N
        end
        if Q !== nothing
            for b in 1:N, a in 1:N
                Q[a, b] = arb_of(LQf, a + (b - 1) * N, prec)
            end
        end
    end
    t = zeros(Float64, 6)
    check(ccall((sym(ctx, :clrs_get_timings, :clrs_mw_get_timings), lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.handle, t))
    return t[1], t[2], t[3], t[4], t[5]
end

"""
Drop-in for the "solve system" stage of `compute_search_direction!` (src/solver.jl:1527-1582): `dx` (the flat
`ArbRefMatrix(sum P_j, 1)` of src/solver.jl:187,310) and `dy` (`N x 1`) are overwritten; `rhs_x` is the vector
`-d - <A_*, Z>` (`:1518-1523`, length sum P_j), `rhs_y` is `p` -- both Arb column matrices.
"""
function solve_system!(ctx::HipContext, dx, dy, rhs_x, rhs_y; prec=precision(dx))
    K, N, nx = ctx.limbs, ctx.n_free, ctx.cluster_off[end]
    rx = zeros(Float64, nx, K); ry = zeros(Float64, max(N, 1), K)
    for i in 1:nx
        limbs_of!(rx, i, rhs_x[i, 1], K)
    end
    for k in 1:N
        limbs_of!(ry, k, rhs_y[k, 1], K)
    end
    dxf = zeros(Float64, nx, K); dyf = zeros(Float64, max(N, 1), K)
    check(ccall((sym(ctx, :clrs_schur_solve, :clrs_mw_schur_solve), libclrs[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                ctx.handle, rx, ry, dxf, dyf))
    for i in 1:nx
        dx[i, 1] = arb_of(dxf, i, prec)
    end
    for k in 1:N
        dy[k, 1] = arb_of(dyf, k, prec)
    end
    return nothing
end


# =====================================================================================================================
# Drop-in front end: `solvesdp` with the reference's signature and 5-tuple return, no patch to the reference needed.
#
# The reference's `solvesdp(problem; prec, kwargs...)` (src/solver.jl:71-99) builds the ClusteredLowRankSDP, converts it to
# `prec`, and `solvesdp(sdp; ...)` (:100-744) preprocesses, runs the loop and post-processes.  Here the same steps run with the
# reference's own functions for everything outside the loop (ClusteredLowRankSDP, convert_to_prec, preprocess!, postprocess,
# solution_to_bigfloat) and with the device-resident loop of the library (clrs_mw_ipm_*) in place of :348-589.
# =====================================================================================================================

# struct clrs_ipm_data / clrs_ipm_params / clrs_ipm_record (include/clrs_hip.h) -- field order and types must match the header
struct IpmData
    C::Ptr{Float64}
    c::Ptr{Float64}
    b::Ptr{Float64}
    maximize::Int32
    reserved::Int32
    constant::Float64
end
struct IpmParams
    beta_infeasible::Float64
    beta_feasible::Float64
    gamma::Float64
    dual_error_threshold::Float64
    primal_error_threshold::Float64
    max_complementary_gap::Float64
    step_length_threshold::Float64
    safe_step::Int32
    corrector_only::Int32
end
struct IpmRecord
    iter::Int32
    pd_feas::Int32
    error_code::Int32
    factor_status::Int32
    cholesky_status::Int32
    refine_bits::Int32
    mu::Float64
    d_obj::Float64
    p_obj::Float64
    gap::Float64
    dual_error::Float64
    primal_error::Float64
    alpha_d::Float64
    alpha_p::Float64
    beta_c::Float64
    max_P::Float64
    max_p::Float64
    max_d::Float64
end
struct IpmStop
    duality_gap_threshold::Float64
    need_dual_feasible::Int32
    need_primal_feasible::Int32
    max_iterations::Int32
    reserved::Int32
end

# What the per-record callback of clrs_mw_ipm_solve_cb needs between two rows of the iteration table: the reference prints, in the row of an
# iteration, the objectives and the gap of the iterate the iteration STARTED from (src/solver.jl:566-582)
mutable struct TableState
    iter::Int
    t0::Float64
    d_obj::Float64
    p_obj::Float64
    gap::Float64
end
function print_row(recp::Ptr{IpmRecord}, user::Ptr{Cvoid})::Cvoid
    st = unsafe_pointer_to_objref(user)::TableState
    r = unsafe_load(recp)
    CLRS.@printf("%5d %8.1f %11.3e %11.3e %11.3e %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e\n", st.iter, time() - st.t0,
                 r.mu, st.d_obj, st.p_obj, st.gap, r.max_P, r.max_p, r.max_d, r.alpha_d, r.alpha_p, r.beta_c)
    if r.error_code == 0
        st.d_obj, st.p_obj, st.gap = r.d_obj, r.p_obj, r.gap
    end
    st.iter += 1
    return nothing
end

"""Cluster-local renumbering of the constraints preprocessing kept: `original row => position among the kept rows` (what `cs_map[j]` is)."""
function renumber_kept(nrows::Integer, removed)
    gone = Set{Int}(removed)
    out = Dict{Int,Int}()
    for p in 1:nrows
        p in gone || (out[p] = length(out) + 1)
    end
    return out
end

"""
Limb planes (len x K) of the warm-start iterate: x and X from `dualsol`, y and Y from `primalsol` (the meaning of src/solver.jl:202-239), in the
layouts of the device loop (x: constraints stacked by cluster; X, Y: blocks in description order, column-major).
"""
function warm_start_planes(sdp, ctx::HipContext, dualsol, primalsol, K::Int)
    nxy, nx, N = ctx.block_off[end], ctx.cluster_off[end], ctx.n_free
    xw = zeros(Float64, max(nx, 1), K); yw = zeros(Float64, max(N, 1), K)
    Xw = zeros(Float64, max(nxy, 1), K); Yw = zeros(Float64, max(nxy, 1), K)
    for ((con, smp), row) in sdp.order_c                             # (constraint of the Problem, sample) -> row of x
        limbs_of!(xw, row, dualsol.x[con][smp], K)
    end
    for (k, name) in enumerate(sdp.free_coeff_names)
        limbs_of!(yw, k, primalsol.freevars[name], K)
    end
    for (b, (j, l)) in enumerate(ctx.jl)
        name = sdp.matrix_coeff_names[j][l]
        m = size(sdp.A[j][l], 1)
        n = ctx.block_n[b]
        dl = div(n, m)
        whole = !(CLRS.Block(name, 1, 1) in sdp.matrix_coeff_blocks)  # a variable without sub-blocks is stored under its bare name
        for r in 1:m, s in 1:r
            key = (whole && r == 1 && s == 1) ? name : CLRS.Block(name, r, s)
            for (sol, W) in ((dualsol, Xw), (primalsol, Yw))
                M = sol.matrixvars[key]
                for cc in 1:dl, rr in 1:dl
                    limbs_of!(W, ctx.block_off[b] + (r - 1) * dl + rr + ((s - 1) * dl + cc - 1) * n, M[rr, cc], K)
                    r == s || limbs_of!(W, ctx.block_off[b] + (s - 1) * dl + cc + ((r - 1) * dl + rr - 1) * n, M[rr, cc], K)   # the mirrored sub-block: the iterate is symmetric
                end
            end
        end
    end
    return xw, yw, Xw, Yw
end

"""
    solvesdp(problem::Problem; prec=precision(BigFloat), device=0, kwargs...)
    solvesdp(sdp::ClusteredLowRankSDP; prec=precision(BigFloat), device=0, kwargs...)

The reference's `solvesdp` (src/solver.jl:42-127: same keywords, same defaults, same return
`status, dualsol, primalsol, solve_time, errorcode`) with the interior-point loop on the GPU at `limbs_for(prec)` words per number.
`dualsol` / `primalsol` warm-start the device loop (`clrs_mw_ipm_set`).  `matmul_prec` selects the limbs of the pairing products (`clrs_mw_options.matmul_limbs`), `correctoronly` is `clrs_ipm_params.corrector_only`.  Keywords without a
device counterpart (`save_settings`, `testing`) are accepted; a non-default value raises an `ArgumentError`, so that a caller never silently gets something else than it asked for.
"""
function solvesdp(problem::CLRS.Problem; prec=precision(BigFloat), kwargs...)
    sdp = CLRS.ClusteredLowRankSDP(problem, prec=prec)          # src/solver.jl:96-98
    sdp = CLRS.convert_to_prec(sdp, prec)
    return solvesdp(sdp; prec=prec, kwargs...)
end

function solvesdp(sdp::CLRS.ClusteredLowRankSDP;
        prec=precision(BigFloat), device::Integer=0,
        maxiterations=500, beta_infeasible=3//10, beta_feasible=1//10, gamma=9//10,
        omega_p=big(10)^10, omega_d=big(10)^10,
        duality_gap_threshold=1e-15, dual_error_threshold=1e-30, primal_error_threshold=1e-30,
        max_complementary_gap=big(10)^100, need_dual_feasible=false, need_primal_feasible=false,
        verbose=true, step_length_threshold=1e-7,
        dualsol::Union{Nothing,CLRS.DualSolution}=nothing, primalsol::Union{Nothing,CLRS.PrimalSolution}=nothing,
        safe_step::Bool=true, correctoronly=false, save_settings=nothing, preprocess=true, matmul_prec=prec, testing=false)
    (save_settings === nothing || (save_settings.iter_interval === nothing && save_settings.time_interval === nothing && save_settings.callback === nothing)) ||
        throw(ArgumentError("save_settings is not available with the HIP backend"))
    matmul_prec <= prec || throw(ArgumentError("matmul_prec must not exceed prec"))
    warm = dualsol !== nothing && primalsol !== nothing               # src/solver.jl:202: only both together are used
    lib = libclrs[]
    K = limbs_for(prec)
    K >= 2 || throw(ArgumentError("the device-resident loop runs at 2 or more limbs (prec > 53)"))
    # preprocessing with the reference's own code (CLRS.preprocess!, src/pre_postprocessing.jl); the constraints it leaves are renumbered per cluster
    rows_before = [size(sdp.B[j], 1) for j in eachindex(sdp.B)]
    cs, var_rels = preprocess ? CLRS.preprocess!(sdp) : ((), nothing)
    cs_map = [renumber_kept(rows_before[j], (t[3] for t in cs if t[2] == j)) for j in eachindex(sdp.B)]
    ctx = HipContext(sdp, cs_map; device=device, limbs=K, matmul_limbs=(matmul_prec == prec ? 0 : min(K, limbs_for(matmul_prec))))
    DL = data_limbs_for(K)
    nxy, nx, N = ctx.block_off[end], ctx.cluster_off[end], ctx.n_free
    # objective data as DL limb planes: C in the xy layout, c in the x layout, b
    Cf = zeros(Float64, max(nxy, 1), DL); cf = zeros(Float64, max(nx, 1), DL); bf = zeros(Float64, max(N, 1), DL)
    for (b, (j, l)) in enumerate(ctx.jl)
        blk = sdp.C.blocks[j].blocks[l]
        n = ctx.block_n[b]
        for cc in 1:n, r in 1:n
            limbs_of!(Cf, ctx.block_off[b] + r + (cc - 1) * n, blk[r, cc], DL)
        end
    end
    for j in eachindex(sdp.c), p in 1:ctx.cluster_P[j]
        limbs_of!(cf, ctx.cluster_off[j] + p, sdp.c[j][p, 1], DL)
    end
    for k in 1:N
        limbs_of!(bf, k, sdp.b[k, 1], DL)
    end
    data = Ref(IpmData(pointer(Cf), pointer(cf), pointer(bf), sdp.maximize ? 1 : 0, 0, f64(sdp.constant)))
    prm = Ref(IpmParams(Float64(beta_infeasible), Float64(beta_feasible), Float64(gamma), Float64(dual_error_threshold),
                        Float64(primal_error_threshold), Float64(max_complementary_gap), Float64(step_length_threshold), safe_step ? 1 : 0, correctoronly ? 1 : 0))
    GC.@preserve Cf cf bf begin
        check(ccall((:clrs_mw_ipm_create_ex, lib), Cint, (Ptr{Cvoid}, Ref{IpmData}, Cint), ctx.handle, data, DL))
    end
    check(ccall((:clrs_mw_ipm_set_params, lib), Cint, (Ptr{Cvoid}, Ref{IpmParams}), ctx.handle, prm))
    check(ccall((:clrs_mw_ipm_init, lib), Cint, (Ptr{Cvoid}, Cdouble, Cdouble), ctx.handle, Float64(omega_p), Float64(omega_d)))
    d_obj0, p_obj0, gap0 = f64(sdp.constant), f64(sdp.constant), 0.0
    if warm
        # the iterate of a previous solve (src/solver.jl:202-239) as limb planes through clrs_mw_ipm_set.  The reference leaves the case of
        # constraints removed by preprocessing open (its TODO at :203: x is indexed by the ORIGINAL constraints); refused here instead of guessed
        isempty(cs) || throw(ArgumentError("warm start of a problem from which preprocessing removed constraints: pass preprocess=false"))
        xw, yw, Xw, Yw = warm_start_planes(sdp, ctx, dualsol, primalsol, K)
        GC.@preserve xw yw Xw Yw begin
            check(ccall((:clrs_mw_ipm_set, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.handle, xw, N > 0 ? pointer(yw) : Ptr{Float64}(C_NULL), Xw, Yw))
        end
        obj3 = zeros(Float64, 3 * K)                               # objectives of the starting iterate (src/solver.jl:319-321)
        check(ccall((:clrs_mw_ipm_objectives, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.handle, obj3))
        d_obj0, p_obj0, gap0 = obj3[1], obj3[K + 1], obj3[2 * K + 1]
    end
    if verbose
        CLRS.@printf("%5s %8s %11s %11s %11s %10s %10s %10s %10s %10s %10s %10s\n", "iter", "time(s)", "μ", "D-obj", "P-obj", "gap",
                     "D-error", "d-error", "p-error", "α_d", "α_p", "beta")
    end
    time_start = time()
    iter, error_code = 1, 0
    dual_error = primal_error = Inf
    gap, d_obj, p_obj, pd_feas = gap0, d_obj0, p_obj0, false
    # The whole loop in ONE call (clrs_mw_ipm_solve_cb): the library enqueues iterations one ahead of the record it waits for and the device evaluates the
    # termination test of src/solver.jl:921-950 itself -- the path bench.py measures.  The rows of the iteration table (:566-582) are printed by a callback as
    # the host reads each record; the records come back as well.
    table = TableState(1, time_start, d_obj0, p_obj0, gap0)
    row_cb = @cfunction(print_row, Cvoid, (Ptr{IpmRecord}, Ptr{Cvoid}))
    nrec = max(Int(maxiterations), 1)
    recs = Vector{IpmRecord}(undef, nrec)
    n_it, err = Ref{Cint}(0), Ref{Cint}(0)
    stop = Ref(IpmStop(Float64(duality_gap_threshold), need_dual_feasible ? 1 : 0, need_primal_feasible ? 1 : 0, Int32(maxiterations), 0))
    GC.@preserve table recs begin
        check(ccall((:clrs_mw_ipm_solve_cb, lib), Cint, (Ptr{Cvoid}, Ref{IpmStop}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{IpmRecord}, Cint, Ref{Cint}, Ref{Cint}),
                    ctx.handle, stop, verbose ? row_cb : C_NULL, pointer_from_objref(table), recs, nrec, n_it, err))
    end
    error_code = Int(err[])
    for i in 1:min(Int(n_it[]), nrec)
        r = recs[i]
        dual_error, primal_error, pd_feas = r.dual_error, r.primal_error, r.pd_feas != 0
        if r.error_code != 0                                       # 1 SolverFailure, 3 mu too large, 4 step too short (docs/src/solving.md:64-70); 5: clrs_hip.h
            if verbose && r.error_code == 1
                J = length(sdp.A)
                if r.cholesky_status > 0
                    j, l = ctx.jl[r.cholesky_status]
                    println("The cholesky decomposition of X was not computed correctly in block ($j,$l). Try again with higher precision")
                elseif 0 < r.factor_status <= J
                    println("S was not decomposed succesfully in block $(r.factor_status), try again with higher precision. If this occurred in the first iteration, remove linear dependencies in the PSD part of the constraints or turn preprocessing on.")
                elseif r.factor_status == J + 1
                    println("Q was not decomposed correctly. Try restarting with a higher precision. If this occurred in the first iteration, remove linear dependencies between free variables or turn preprocessing on.")
                end
                println("We return the current solution and optimality status.")
            end
            break
        end
        d_obj, p_obj, gap = r.d_obj, r.p_obj, r.gap
        iter += 1
    end
    if verbose
        if error_code == 2                                         # src/solver.jl:362-366
            println("The maximum number of iterations has been reached.")
        elseif error_code == 0 && !correctoronly && dual_error < dual_error_threshold && primal_error < primal_error_threshold && gap < duality_gap_threshold
            println("Optimal solution found")
        end
    end
    time_total = time() - time_start
    # the iterate back as Arb midpoints in the reference's containers
    xf = zeros(Float64, max(nx, 1), K); yf = zeros(Float64, max(N, 1), K); Xf = zeros(Float64, max(nxy, 1), K); Yf = zeros(Float64, max(nxy, 1), K)
    check(ccall((:clrs_mw_ipm_get, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.handle, xf, yf, Xf, Yf))
    x = Arblib.ArbRefMatrix(nx, 1; prec=prec); y = Arblib.ArbRefMatrix(N, 1; prec=prec)
    for i in 1:nx
        x[i, 1] = arb_of(xf, i, prec)
    end
    for k in 1:N
        y[k, 1] = arb_of(yf, k, prec)
    end
    unpack(Mf) = CLRS.BlockDiagonal([CLRS.BlockDiagonal([begin
                b = findfirst(==((j, l)), ctx.jl); n = ctx.block_n[b]
                M = Arblib.ArbRefMatrix(n, n; prec=prec)
                for cc in 1:n, r in 1:n
                    M[r, cc] = arb_of(Mf, ctx.block_off[b] + r + (cc - 1) * n, prec)
                end
                M
            end for l in eachindex(sdp.A[j])]) for j in eachindex(sdp.A)])
    X, Y = unpack(Xf), unpack(Yf)
    if preprocess
        x, y = CLRS.postprocess(x, y, cs, var_rels)                # src/solver.jl:630-632
    end
    dsol, psol = CLRS.solution_to_bigfloat(X, x, Y, y, sdp)
    status = if pd_feas && gap < duality_gap_threshold              # src/solver.jl:727-741
        CLRS.Optimal()
    elseif (pd_feas && gap < 1e-8) || (dual_error < 1e-15 && primal_error < 1e-15 && gap < 1e-8)
        CLRS.NearOptimal()
    elseif pd_feas
        CLRS.Feasible()
    elseif primal_error < primal_error_threshold
        CLRS.PrimalFeasible()
    elseif dual_error < dual_error_threshold
        CLRS.DualFeasible()
    else
        CLRS.NotConverged()
    end
    return status, dsol, psol, time_total, error_code
end

"""
    ClusteredLowRankHIP.optimize!(opt)

`MOI.optimize!` for the reference's `ClusteredLowRankSolver.Optimizer` (ext/MOIExt.jl:395-407) with this package's `solvesdp`: reads
`opt.problem` and `opt.options`, fills `opt.result_data` under the keys the reference's result getters read (`:primalsol`, `:dualsol`,
`:status`, `:errorcode`; ext/MOIExt.jl:417-566).  `ext/ClusteredLowRankHIPMOIExt.jl` wraps it in an `Optimizer` for JuMP.
"""
function optimize!(opt; device::Integer=0)
    opts = Dict{Symbol,Any}(k => v for (k, v) in opt.options)      # (save_settings included: solvesdp raises for what the device loop cannot do)
    status, dualsol, primalsol, t, e = solvesdp(opt.problem; device=device, opts...)
    opt.optimized = true
    opt.result_data[:primalsol] = primalsol
    opt.result_data[:dualsol] = dualsol
    opt.result_data[:status] = status
    opt.result_data[:errorcode] = e
    opt.result_data[:solve_time] = t
    return status, dualsol, primalsol, t, e
end

"""
    kernel_vectors(dualblocks, primalblocks; prec=precision(BigFloat), device=0, kernel_errbound=1e-10, kernel_round_errbound=1e-15, kernel_use_dual=true)
    kernel_vectors(result; kwargs...)

Step 1 of the reference's `exact_solution` ("Finding the kernel": `detecteigenvectors`, src/rounding.jl:575-642, before the entries are rounded to a
field) for all blocks in one device call (`clrs_mw_kernel_vectors`, DESIGN.md section 12) at `limbs_for(prec)` words per number.  `dualblocks[b]` /
`primalblocks[b]`: the square matrices of block `b` (anything `BigFloat(::eltype)` accepts).  Returns, per block, the kernel vectors of the primal
block as `Vector{Vector{BigFloat}}`, each of length `n_b`, in the reference's row convention (`vecs[i] = Rp[i, pinv]`); the keywords are the kernel
fields of `RoundingSettings` with its defaults.  Raises, like the reference, when `maximum(abs.(primalblock * v))` of some vector is not below
`kernel_errbound`.  Where the reference takes an SVD of the primal block (`kernel_use_dual = false`, or a dual block with entries beyond
`1 / sqrt(kernel_round_errbound)`), the primal block itself is eliminated: the same subspace, in echelon form over other pivot columns.
`result`: the tuple `solvesdp` returns (`status, dualsol, primalsol, ...`); the blocks are then the `matrixvars` of both solutions and the value is a
`Dict` from their keys to the vectors.

`rationalize=true`: the entries are also rounded to the field QQ on the device (`clrs_mw_kernel_vectors_rational`, DESIGN.md section 13: what `roundx` ->
`clindep` does per entry, src/rounding.jl:623-628 -- the first continued-fraction convergent `p // q` with `|q v - p| < kernel_round_errbound`) and the rounded
vectors are tested against the primal block again (src/rounding.jl:630-639); the value is then `Vector{Vector{Rational{BigInt}}}` per block.  Raises
"clindep failed to find a relation" where an entry has none with `p, q < 2^53`, and "wrong vector detected" where `maximum(abs.(primalblock * v))` of a
rounded vector is above `kernel_errbound`.
"""
function kernel_vectors(dualblocks::AbstractVector, primalblocks::AbstractVector; prec::Integer=precision(BigFloat), device::Integer=0,
                        kernel_errbound::Real=1e-10, kernel_round_errbound::Real=1e-15, kernel_use_dual::Bool=true, rationalize::Bool=false)
    length(dualblocks) == length(primalblocks) || error("kernel_vectors: one dual block per primal block")
    K = limbs_for(prec)
    K >= 4 || error("kernel_vectors: prec = $prec selects $K limbs; the multi-word kernels need at least 4 (prec >= 158)")
    nb = length(dualblocks)
    n = Int32[size(M, 1) for M in primalblocks]
    all(size(dualblocks[b]) == (n[b], n[b]) && size(primalblocks[b]) == (n[b], n[b]) for b in 1:nb) || error("kernel_vectors: blocks must be square and of equal size")
    off = cumsum(vcat(0, [Int(v)^2 for v in n])); xoff = cumsum(vcat(0, [Int(v) for v in n]))
    plane, xlen = off[end], xoff[end]
    Xw = zeros(Float64, max(plane, 1), K); Yw = zeros(Float64, max(plane, 1), K); Vw = zeros(Float64, max(plane, 1), K)
    for b in 1:nb, cc in 1:n[b], rr in 1:n[b]
        limbs_of!(Xw, off[b] + rr + (cc - 1) * n[b], BigFloat(dualblocks[b][rr, cc]), K)
        limbs_of!(Yw, off[b] + rr + (cc - 1) * n[b], BigFloat(primalblocks[b][rr, cc]), K)
    end
    branch = zeros(Int32, max(nb, 1)); rank = zeros(Int32, max(nb, 1)); count = zeros(Int32, max(nb, 1)); perm = zeros(Int32, max(xlen, 1))
    rmax = zeros(Float64, max(xlen, 1)); vmax = zeros(Float64, max(xlen, 1)); piv = zeros(Float64, max(xlen, 1), K)
    if rationalize
        num = zeros(Float64, max(plane, 1)); den = zeros(Float64, max(plane, 1)); rstat = zeros(Int32, max(plane, 1))
        Vq = zeros(Float64, max(plane, 1), K); rmax2 = zeros(Float64, max(xlen, 1))
        check(ccall((:clrs_mw_kernel_vectors_rational, libclrs[]), Cint,
                    (Cint, Cint, Cint, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Cint, Cdouble, Cdouble, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                    device, K, nb, n, Xw, Yw, plane, Float64(kernel_errbound), kernel_use_dual ? 1 : 0, 1 / sqrt(Float64(kernel_round_errbound)),
                    Float64(kernel_round_errbound), branch, perm, rank, count, Vw, rmax, vmax, piv, num, den, rstat, Vq, rmax2))
        outq = Vector{Vector{Vector{Rational{BigInt}}}}(undef, nb)
        for b in 1:nb
            vecs = Vector{Vector{Rational{BigInt}}}()
            for v in 1:count[b]
                res = rmax[xoff[b] + v]
                res < kernel_errbound || error("Warning: wrong vector detected! (error = $res, block $b, maximum(abs.(v)) = $(vmax[xoff[b] + v]))")
                for i in 1:n[b]
                    st = rstat[off[b] + i + (v - 1) * n[b]]
                    st == 0 || error("clindep failed to find a relation: block $b, vector $v, entry $i (status $st)")
                end
                res2 = rmax2[xoff[b] + v]
                res2 > kernel_errbound && error("Warning: wrong vector detected! (error = $res2 after rounding, block $b)")
                push!(vecs, [BigInt(num[off[b] + i + (v - 1) * n[b]]) // BigInt(den[off[b] + i + (v - 1) * n[b]]) for i in 1:n[b]])
            end
            outq[b] = vecs
        end
        return outq
    end
    check(ccall((:clrs_mw_kernel_vectors, libclrs[]), Cint,
                (Cint, Cint, Cint, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Cint, Cdouble, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, K, nb, n, Xw, Yw, plane, Float64(kernel_errbound), kernel_use_dual ? 1 : 0, 1 / sqrt(Float64(kernel_round_errbound)),
                branch, perm, rank, count, Vw, rmax, vmax, piv))
    out = Vector{Vector{Vector{BigFloat}}}(undef, nb)
    setprecision(BigFloat, max(prec, 64 * K + 64)) do
        for b in 1:nb
            vecs = Vector{Vector{BigFloat}}()
            for v in 1:count[b]
                res = rmax[xoff[b] + v]
                res < kernel_errbound || error("Warning: wrong vector detected! (error = $res, block $b, maximum(abs.(v)) = $(vmax[xoff[b] + v]))")
                push!(vecs, [BigFloat(sum(BigFloat(Vw[off[b] + i + (v - 1) * n[b], l]) for l in K:-1:1); precision=prec) for i in 1:n[b]])
            end
            out[b] = vecs
        end
    end
    return out
end

function kernel_vectors(result::Tuple; kwargs...)
    dualsol, primalsol = result[2], result[3]
    keys_ = collect(keys(primalsol.matrixvars))
    vecs = kernel_vectors([dualsol.matrixvars[k] for k in keys_], [primalsol.matrixvars[k] for k in keys_]; kwargs...)
    return Dict(k => vecs[i] for (i, k) in enumerate(keys_))
end

"""
    rationalize(v::AbstractVector{BigFloat}; prec=precision(BigFloat), errbound=1e-15, device=0)

Round numbers to rationals on the device (`clrs_mw_rationalize`, DESIGN.md section 13) at `limbs_for(prec)` words per number: per number the first
continued-fraction convergent `p // q` of `|v|` with `|q |v| - p| < errbound`, the sign restored.  Returns `(rationals, status)`: `status[i]` is 0 where a
relation was found, 1 where none with `p, q < 2^53` exists within 96 steps, 2 where `v[i]` is not finite; `rationals[i]` is `0 // 1` unless `status[i] == 0`.
"""
function rationalize(v::AbstractVector{BigFloat}; prec::Integer=precision(BigFloat), errbound::Real=1e-15, device::Integer=0)
    K = limbs_for(prec)
    K >= 4 || error("rationalize: prec = $prec selects $K limbs; the multi-word kernels need at least 4 (prec >= 158)")
    cnt = length(v)
    vw = zeros(Float64, max(cnt, 1), K); vq = zeros(Float64, max(cnt, 1), K)
    for i in 1:cnt
        isfinite(v[i]) ? limbs_of!(vw, i, v[i], K) : (vw[i, 1] = Float64(v[i]))
    end
    num = zeros(Float64, max(cnt, 1)); den = zeros(Float64, max(cnt, 1)); status = zeros(Int32, max(cnt, 1))
    check(ccall((:clrs_mw_rationalize, libclrs[]), Cint,
                (Cint, Cint, Cint, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                device, K, cnt, vw, max(cnt, 1), Float64(errbound), num, den, status, vq))
    return [status[i] == 0 ? BigInt(num[i]) // BigInt(den[i]) : big(0) // big(1) for i in 1:cnt], status[1:cnt]
end

"""
    posv(A::AbstractMatrix{BigFloat}, B::AbstractVecOrMat{BigFloat}; prec=precision(BigFloat), device=0)

Solve `A X = B` for a dense symmetric positive definite `A` on the device (`clrs_mw_posv`, DESIGN.md section 26) at `limbs_for(prec)` words per number: a
blocked Cholesky whose diagonal blocks are eliminated by one workgroup each and whose other steps are multi-word products.  Only the lower triangle of `A`
is read.  Raises when a pivot is not positive, naming its column.
"""
function posv(A::AbstractMatrix{BigFloat}, B::AbstractVecOrMat{BigFloat}; prec::Integer=precision(BigFloat), device::Integer=0)
    K = limbs_for(prec)
    K >= 4 || error("posv: prec = $prec selects $K limbs; the multi-word kernels need at least 4 (prec >= 158)")
    n = size(A, 1); nrhs = size(B, 2)
    size(A, 2) == n && size(B, 1) == n || error("posv: A must be n x n and B n x nrhs")
    Aw = zeros(Float64, max(n * n, 1), K); Bw = zeros(Float64, max(n * nrhs, 1), K); Xw = zeros(Float64, max(n * nrhs, 1), K)
    for c in 1:n, r in c:n
        limbs_of!(Aw, r + (c - 1) * n, A[r, c], K)
    end
    for c in 1:nrhs, r in 1:n
        limbs_of!(Bw, r + (c - 1) * n, B[r, c], K)
    end
    info = zeros(Int32, 2)
    check(ccall((:clrs_mw_posv, libclrs[]), Cint,
                (Cint, Cint, Cint, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Int32}),
                device, K, n, nrhs, Aw, size(Aw, 1), Bw, size(Bw, 1), Xw, size(Xw, 1), info))
    info[1] == 0 || error("posv: the pivot of column $(info[1] - 1) (counted from 0) is not positive")
    X = [BigFloat(sum(BigFloat(Xw[r + (c - 1) * n, l]) for l in K:-1:1); precision=prec) for r in 1:n, c in 1:nrhs]
    return B isa AbstractVector ? vec(X) : X
end

"""
    round_to_field(v::AbstractVector{BigFloat}, g::BigFloat, deg::Integer; prec=precision(BigFloat), bits=1000, errbound=1e-15, nd=0, device=0)

The reference's `roundx(x, g, deg)` (src/rounding.jl:519-534) for `deg` = 2 .. 4 on the device (`clrs_mw_field_round`, DESIGN.md section 23), at
`limbs_for(prec)` words per number: per number the first rung p = 1, 6, 11, .. <= min(bits, 53 limbs - 16) at which the first row `a` of an LLL-reduced
basis of `[I | floor(2^p (v, 1, g, .., g^(deg-1)))]` has `|a[1] v + a[2] + a[3] g + ..| < errbound`.  Returns `(coeffs, status, rung)`: `coeffs[i]` the
`deg` rationals `-a[k+1] // a[1]` (zeros unless `status[i] == 0`); `status[i]` 0 found, 1 ladder exhausted, 2 not finite, 3 steering failed or a cap was
hit, 4 an entry left its `nd` digits, 5 `a[1] == 0`; `rung[i]` the bits of the rung the number ended at.  `nd = 0` takes the default digit count.
"""
function round_to_field(v::AbstractVector{BigFloat}, g::BigFloat, deg::Integer; prec::Integer=precision(BigFloat), bits::Integer=1000, errbound::Real=1e-15,
                        nd::Integer=0, device::Integer=0)
    K = limbs_for(prec)
    K >= 4 || error("round_to_field: prec = $prec selects $K limbs; the multi-word kernels need at least 4 (prec >= 158)")
    2 <= deg <= 4 || error("round_to_field: the degree must lie in 2:4, got $deg")
    cnt = length(v); plane = max(cnt, 1); D = deg + 1
    top = 1 + 5 * div(min(bits, 53 * K - 16) - 1, 5)
    ndig = nd > 0 ? Int(nd) : min(20, div(top, 48) + 3)
    vw = zeros(Float64, plane, K); vq = zeros(Float64, plane, K); gw = zeros(Float64, deg, K)
    for i in 1:cnt
        isfinite(v[i]) ? limbs_of!(vw, i, v[i], K) : (vw[i, 1] = Float64(v[i]))
    end
    for k in 1:deg
        limbs_of!(gw, k, g^(k - 1), K)
    end
    rel = zeros(Int32, plane, D, ndig); status = zeros(Int32, plane); rung = zeros(Int32, plane); err = zeros(Float64, plane); info = zeros(Int32, plane, 2)
    check(ccall((:clrs_mw_field_round, libclrs[]), Cint,
                (Cint, Cint, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Cdouble, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}),
                device, K, deg, gw, cnt, vw, plane, bits, Float64(errbound), ndig, rel, status, rung, err, vq, info))
    a(i, k) = sum(BigInt(rel[i, k, s]) << (24 * (s - 1)) for s in 1:ndig)
    coeffs = [status[i] == 0 ? [-a(i, k + 1) // a(i, 1) for k in 1:deg] : [big(0) // big(1) for k in 1:deg] for i in 1:cnt]
    return coeffs, status[1:cnt], rung[1:cnt]
end

"""
    minpoly(v::AbstractVector{BigFloat}, d::Integer; prec=precision(BigFloat), bits=100 * d, errbound=1e-15, nd=0, device=0)

The reference's `min_poly(v, d)` (src/find_field.jl:111-113) for `d` = 1 .. 4 on the device (`clrs_mw_minpoly`, DESIGN.md section 27), at `limbs_for(prec)`
words per number: per number the first rung p = 1, 6, 11, .. <= min(bits, 53 limbs - 16) at which the first row `a` of an LLL-reduced basis of
`[I | floor(2^p (1, v, .., v^d))]` has `|a[1] + a[2] v + .. + a[d+1] v^d| < errbound`.  Returns `(coeffs, status, rung)`: `coeffs[i]` the `d + 1` integers
low to high (zeros unless `status[i]` is 0 or 5); `status[i]` 0 found, 1 ladder exhausted, 2 not finite, 3 steering failed or a cap was hit, 4 an entry left
its `nd` digits or a power is 2^22 or more, 5 `a[1] == 0` or `a[d+1] == 0`: nothing at this degree; `rung[i]` the bits of the rung the number ended at.
"""
function minpoly(v::AbstractVector{BigFloat}, d::Integer; prec::Integer=precision(BigFloat), bits::Integer=100 * d, errbound::Real=1e-15, nd::Integer=0,
                 device::Integer=0)
    K = limbs_for(prec)
    K >= 4 || error("minpoly: prec = $prec selects $K limbs; the multi-word kernels need at least 4 (prec >= 158)")
    1 <= d <= 4 || error("minpoly: the degree must lie in 1:4, got $d")
    cnt = length(v); plane = max(cnt, 1); D = d + 1
    top = 1 + 5 * div(min(bits, 53 * K - 16) - 1, 5)
    ndig = nd > 0 ? Int(nd) : min(20, div(top, 48) + 3)
    vw = zeros(Float64, plane, K)
    for i in 1:cnt
        isfinite(v[i]) ? limbs_of!(vw, i, v[i], K) : (vw[i, 1] = Float64(v[i]))
    end
    rel = zeros(Int32, plane, D, ndig); status = zeros(Int32, plane); rung = zeros(Int32, plane); err = zeros(Float64, plane); info = zeros(Int32, plane, 2)
    check(ccall((:clrs_mw_minpoly, libclrs[]), Cint,
                (Cint, Cint, Cint, Cint, Ptr{Float64}, Cint, Cint, Cdouble, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                device, K, d, cnt, vw, plane, bits, Float64(errbound), ndig, rel, status, rung, err, info))
    a(i, k) = sum(BigInt(rel[i, k, s]) << (24 * (s - 1)) for s in 1:ndig)
    coeffs = [[a(i, k) for k in 1:D] for i in 1:cnt]
    return coeffs, status[1:cnt], rung[1:cnt]
end

"""
    find_pivots_modular(A::AbstractMatrix{<:Integer}, p::Integer; device=0)
    find_pivots_modular(A::AbstractMatrix{<:Integer}; maxprimes=3, device=0)

The reference's `find_pivots_modular` (src/rounding.jl:288-333), the first work of `project_to_affine_space`: the pivot columns (1-based, ascending) of the
reduced row-echelon form of `A` over the integers mod the prime `p`, 2 <= p < 2^23, on the device (`clrs_modp_rref`, DESIGN.md section 14).  `A` is reduced
mod `p` on the host, so its entries may be `BigInt`s.  Without `p` the reference's schedule: `p = min(maximum(abs.(A)), 10^4)`, per round `p = next_prime(p)`;
the first list with `size(A, 1)` pivots is returned, after `maxprimes` rounds the first of the longest lists.  An empty matrix gives `Int[]`;
`maxprimes < 1` is an `ArgumentError`.
"""
function find_pivots_modular(A::AbstractMatrix{<:Integer}, p::Integer; device::Integer=0)
    nr, nc = size(A)
    (nr == 0 || nc == 0) && return Int[]
    res = Matrix{Int32}(undef, nc, nr)                      # row-major for the library: the transpose, column-major
    for i in 1:nr, j in 1:nc
        res[j, i] = Int32(mod(A[i, j], p))
    end
    pivots = zeros(Int32, min(nr, nc)); rank = zeros(Int32, 1)
    check(ccall((:clrs_modp_rref, libclrs[]), Cint,
                (Cint, Cint, Cint, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                device, nr, nc, p, res, pivots, rank, Ptr{Int32}(C_NULL)))
    return Int[Int(pivots[t]) + 1 for t in 1:rank[1]]
end

# the smallest prime strictly above x (trial division: the schedule stays near 10^4)
function next_prime_above(x::Integer)
    n = max(x + 1, 2)
    while any(n % d == 0 for d in 2:isqrt(n))
        n += 1
    end
    return n
end

function find_pivots_modular(A::AbstractMatrix{<:Integer}; maxprimes::Integer=3, device::Integer=0)
    maxprimes >= 1 || throw(ArgumentError("find_pivots_modular: maxprimes must be at least 1, got $maxprimes"))
    isempty(A) && return Int[]
    prime = Int(min(maximum(abs, A), 10^4))
    best = nothing                                          # the longest list so far; a later list replaces it only when strictly longer
    for _ in 1:maxprimes
        prime = next_prime_above(prime)
        cols = find_pivots_modular(A, prime; device=device)
        length(cols) == size(A, 1) && return cols           # one pivot per row: nothing longer exists
        if best === nothing || length(cols) > length(best)
            best = cols
        end
    end
    return best
end

# balanced base-2^24 digits, little-endian, every digit in [-2^23, 2^23): digit l of value i at out[i, l] (planar for the library: column-major)
function balanced_digits(values::AbstractVector{BigInt}, count::Integer)
    out = zeros(Int32, max(length(values), 1), count)
    half, base = big(1) << 23, big(1) << 24
    for (i, v0) in enumerate(values)
        v = v0
        for l in 1:count
            d = mod(v + half, base) - half
            out[i, l] = Int32(d)
            v = (v - d) >> 24
        end
        v == 0 || error("balanced_digits: a value does not fit in $count digits")
    end
    return out
end

# digits enough for every value of this magnitude: c digits hold every |v| <= (2^23 - 1) (2^(24 c) - 1) / (2^24 - 1), all digits 2^23 - 1
function digits_needed(maxabs::BigInt)
    c = 1
    while maxabs > (big(2)^23 - 1) * ((big(1) << (24 * c)) - 1) ÷ (big(2)^24 - 1)
        c += 1
    end
    return c
end

# sum_l d[i, l] 2^(24 (l - 1))
from_balanced_digits(d::AbstractMatrix{Int32}, i::Integer) = foldr((l, acc) -> (acc << 24) + d[i, l], 1:size(d, 2); init=big(0))

# num // den with num = a den (mod m), |num| <= N, 0 < den <= D: the half-extended Euclidean algorithm on (m, a mod m), stopped at the first remainder <= N
function rational_reconstruction(a::Nemo.ZZRingElem, m::Nemo.ZZRingElem, N::Nemo.ZZRingElem, D::Nemo.ZZRingElem)
    r0, r1, t0, t1 = m, mod(a, m), Nemo.ZZ(0), Nemo.ZZ(1)
    while r1 > N
        q = div(r0, r1)
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    end
    (t1 == 0 || abs(t1) > D || gcd(r1, abs(t1)) != 1) && return nothing
    return t1 > 0 ? Nemo.QQ(r1, t1) : Nemo.QQ(-r1, -t1)
end

"""
    solve_dixon(A::ZZMatrix, b::ZZMatrix; maxprimes=3, device=0)

The exact solution of the square integer system `A x = b` (`b` one column) as a `QQMatrix`: what the reference asks of `Nemo._solve_dixon`
(src/rounding.jl:274, 351, 360), with the p-adic lifting on the device (`clrs_modp_dixon_lift`, DESIGN.md section 15).  The digits of `A` and `b` are built
from `BigInt`s; the primes are tried downward from 8388593 (at most `maxprimes`) until `A` is invertible mod `p`; the number of steps is the smallest `K`
with `p^(2K) > 4 N2 D2`, `D2 = prod_c max(sum_r A[r, c]^2, 1)`, `N2 = D2 max(sum b^2, 1)`; the entries are reconstructed from `sum_k x_k p^k mod p^K`
with FLINT integers.  Throws an `ErrorException` ("The system is rank-deficient") when `A` is singular mod every prime tried.
"""
function solve_dixon(A::Nemo.ZZMatrix, b::Nemo.ZZMatrix; maxprimes::Integer=3, device::Integer=0)
    n = Nemo.nrows(A)
    (Nemo.ncols(A) == n && Nemo.nrows(b) == n && Nemo.ncols(b) == 1) || throw(ArgumentError("solve_dixon: A must be n x n and b n x 1"))
    maxprimes >= 1 || throw(ArgumentError("solve_dixon: maxprimes must be at least 1, got $maxprimes"))
    n == 0 && return Nemo.zero_matrix(Nemo.QQ, 0, 1)
    Ab = BigInt[BigInt(A[i, j]) for i in 1:n for j in 1:n]              # row-major
    bb = BigInt[BigInt(b[i, 1]) for i in 1:n]
    nd = digits_needed(maximum(abs, Ab)); nbl = digits_needed(maximum(abs, bb))
    Ad = balanced_digits(Ab, nd); bl = balanced_digits(bb, nbl)
    D2 = prod(max(sum(Ab[(i - 1) * n + j]^2 for i in 1:n), big(1)) for j in 1:n)
    N2 = D2 * max(sum(v^2 for v in bb), big(1))
    N = Nemo.ZZ(isqrt(N2) + 1); D = Nemo.ZZ(isqrt(D2) + 1)
    nrl = max(nbl, nd + 1) + 1
    p = 8388594
    for _ in 1:maxprimes
        p -= 1
        while any(p % d == 0 for d in 2:isqrt(p))
            p -= 1
        end
        K = 0; q = big(1)
        while q <= 4 * N2 * D2
            q *= big(p)^2; K += 1
        end
        X = zeros(Int32, n, max(K, 1)); r = zeros(Int32, n, nrl); info = zeros(Int32, 4)
        check(ccall((:clrs_modp_dixon_lift, libclrs[]), Cint,
                    (Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                    device, n, p, nd, Ad, nbl, bl, K, X, r, info))
        info[1] == n || continue                                        # singular mod p: the next prime
        m = Nemo.ZZ(big(p))^K
        x = Nemo.zero_matrix(Nemo.QQ, n, 1)
        for i in 1:n
            v = Nemo.ZZ(0)
            for k in K:-1:1                                             # Horner: sum_k X[i, k] p^(k - 1)
                v = v * p + Int(X[i, k])
            end
            f = rational_reconstruction(v, m, N, D)
            f === nothing && error("solve_dixon: entry $i has no rational reconstruction within the bounds")
            x[i, 1] = f
        end
        return x
    end
    error("The system is rank-deficient")
end

"""
    lll(A::AbstractMatrix{<:Integer}; delta=0.99, eta=0.51, limbs=6, max_swaps=typemax(Int32), device=0)

An LLL-reduced basis of the lattice spanned by the (independent) rows of `A`, at most 128 rows and 256 columns, on the device (`clrs_zz_lll`, DESIGN.md
section 22): what the reference's `reduction_step` (src/rounding.jl:1062-1104) asks of FLINT's `lll`.  Every row operation is exact; the Gram-Schmidt
data that steer them are floating point of `limbs` fp64 words (2, 4 or 6).  Returns a `Matrix{BigInt}`; throws when the reduction ends with a status other
than 0 (1: a cap was reached, 2: the arithmetic gave up -- take more limbs, 3: an entry left its digits).
"""
function lll(A::AbstractMatrix{<:Integer}; delta::Real=0.99, eta::Real=0.51, limbs::Integer=6, max_swaps::Integer=typemax(Int32), device::Integer=0)
    d, c = size(A)
    (d == 0 || c == 0) && return Matrix{BigInt}(undef, d, c)
    vals = BigInt[BigInt(A[i, j]) for i in 1:d for j in 1:c]               # row-major
    nd = digits_needed(maximum(abs, vals) << 40)                            # 40 bits of headroom for the row operations
    digits = balanced_digits(vals, nd)                                      # planar: digit l of entry e at digits[e, l]
    out = zeros(Int32, d * c, nd); info = zeros(Int32, 8)
    check(ccall((:clrs_zz_lll, libclrs[]), Cint,
                (Cint, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}, Cdouble, Cdouble, Cint, Cint, Ptr{Int32}),
                device, 1, Int32[d], Int32[c], Int32[c], nd, digits, out, Float64(delta), Float64(eta), limbs, max_swaps, info))
    info[1] == 0 || error("lll: the reduction ended with status $(info[1]) after $(info[2]) exchanges")
    return BigInt[from_balanced_digits(out, (i - 1) * c + j) for i in 1:d, j in 1:c]
end

# `ClusteredLowRankHIP.Optimizer`: the MOI optimizer type lives in the package extension (ext/ClusteredLowRankHIPMOIExt.jl, loaded with
# MathOptInterface), which registers it here; JuMP takes any callable that returns an optimizer: `GenericModel{BigFloat}(ClusteredLowRankHIP.Optimizer)`
const OPTIMIZER_TYPE = Ref{Any}(nothing)
function Optimizer(; kwargs...)
    OPTIMIZER_TYPE[] === nothing && error("ClusteredLowRankHIP.Optimizer needs MathOptInterface (or JuMP) to be loaded")
    return OPTIMIZER_TYPE[](; kwargs...)
end

end # module

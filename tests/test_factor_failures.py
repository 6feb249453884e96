"""Failed Cholesky factorisations at chosen pivots, chosen blocks and chosen clusters: the reference's SolverFailure (src/solver.jl:395-397 for a block of X,
:1249 for S_j, :1644-1646 for a block of Y in the step length) through every kernel form that can meet it.

In a pipeline of workgroups (csrc/clrs_mw_pipe.hip.h) stage g looks at pivots 0 .. 8 g + 7 only and the W workgroups at all of them: which workgroup writes
a status decides whether a failure is reported at all.  So the failing pivot is placed before, on and after every stage boundary, in blocks and clusters
other than the first, and every status is compared with the 320-bit oracle's.  The fixtures are tests/util.py::ldl_fixture / rank1_flip (checked on the
host by tests/test_failure_fixtures_cpu.py)."""
import re
import time
import types

import numpy as np
import pytest

import clrs_amd
from tests.util import (flat, ldl_fixture, mw_relerr, mw_with_tails, place_block, random_simple_sdp, rank1_flip, spd_iterates)

pytestmark = pytest.mark.gpu

PIVOTS = [0, 1, 7, 8, 9, 15, 16, 24, 31, 32, 33, 40, 47, 48, 63]
BOUND = 0.2          # seconds: a failed factorisation returns at once (no consumer waits out MWP_SPIN_LIMIT)


@pytest.fixture(scope="module")
def oracle_built():
    from oracle import oracle
    oracle.build()


def tol(K, slack):
    return 2.0 ** (-(53 * K - slack - max(0, K - 5)))


def _sym(f, M):
    M = M.copy()
    for b in range(f.n_blocks):
        n = int(f.block_n[b]); sl = slice(int(f.block_off[b]), int(f.block_off[b + 1]))
        for l in range(M.shape[0]):
            A = M[l, sl].reshape(n, n, order="F")
            M[l, sl] = (np.tril(A) + np.tril(A, -1).T).reshape(-1, order="F")
    return M


def _iterates(f, K, seed=1):
    X, Y = spd_iterates(f, seed=seed)
    if K == 0:
        return X, Y
    return _sym(f, mw_with_tails(X, K, seed=seed + 10)), _sym(f, mw_with_tails(Y, K, seed=seed + 20))


def _random(side):
    """two clusters of two low-rank blocks of `side` rows each (plus 1 x 1 blocks)"""
    return clrs_amd.flatten(random_simple_sdp(side, J=2, n_free=2, max_P=8, max_n=side, lr_blocks=2))


def _x_instance(name):
    return _random(int(name[1:])) if name.startswith("r") else flat(name)


def _block_of(f, msg):
    """the 0-based block a SolverFailure of cholesky_blocks names ("block (j,l)": cluster j, l-th block of the cluster, 1-based)"""
    j, l = map(int, re.search(r"block \((\d+),(\d+)\)", str(msg)).groups())
    return int(np.searchsorted(f.block_cluster, j - 1)) + l - 1


def _x_status(ctx, f, X):
    """(status b + 1 of the first failing block or 0, factor or None, seconds)"""
    from clrs_amd.solver import SolverFailure
    t0 = time.perf_counter()
    try:
        Xc = ctx.cholesky_blocks(X)
        st = 0
    except SolverFailure as e:
        Xc, st = None, _block_of(f, e) + 1
    return st, Xc, time.perf_counter() - t0


def _fail_blocks(f):
    """blocks of at least 9 rows to fail in: the last one, and the last of the largest side -- block 0 only where it is the one block"""
    big = [b for b in range(f.n_blocks) if int(f.block_n[b]) >= 9]
    side = max(int(f.block_n[b]) for b in big)
    return sorted({big[-1], [b for b in big if int(f.block_n[b]) == side][-1]}), big


X_CASES = [("ns_8_15_2", K) for K in (4, 5, 6)] + [("delsarte_3_10", 5), ("polyopt40", 4), ("polyopt40", 6), ("ns_8_15_2", 8)] + \
          [("r33", 5), ("r41", 4), ("r41", 6), ("r48", 5), ("r64", 4), ("r80", 5)]


@pytest.mark.parametrize("name,K", X_CASES)
def test_x_block_failure_names_the_oracles_block(name, K, oracle_built):
    """cholesky_blocks of an X whose block b fails at pivot k (k around every stage boundary of the 32- and 64-row pipelines): every form -- one
    workgroup (inverse in LDS, in memory, or columns shared by several workgroups), k_mw_potrf_x_pipe (default choice and forced) -- raises the
    SolverFailure of the oracle's first failing block, at once; a pivot of +2^-30 factors, to the oracle's factor; after a failure the same context factors
    a good X bit for bit as a fresh one (status words and tag epochs recover)."""
    from clrs_amd.mw import MwSchurContext
    from oracle.oracle import Oracle
    f = _x_instance(name)
    X0, _ = _iterates(f, K)
    o = Oracle(f, mp_bits=320 if K <= 5 else 640)
    fresh = MwSchurContext(f, limbs=K, pipeline=False)
    G = fresh.cholesky_blocks(X0)
    fresh.close()
    blocks, big = _fail_blocks(f)
    cases = []
    for b in blocks:
        n = int(f.block_n[b])
        for k in [k for k in PIVOTS if k < n]:
            cases.append((b, k))
    expect = {}
    for b, k in cases:
        n = int(f.block_n[b])
        Xf = place_block(f, X0, b, ldl_fixture(n, k, seed=7 * b + k), K, seed=b)
        Xt = place_block(f, X0, b, ldl_fixture(n, k, seed=7 * b + k, variant="tiny"), K, seed=b)
        st, _ = o.cholesky_blocks_mw(Xf)
        assert st == b + 1, (b, k, st)
        stt, Lt = o.cholesky_blocks_mw(Xt)
        assert stt == 0
        expect[(b, k)] = (Xf, Xt, Lt)
    # two failing blocks (a late pivot in the earlier one, pivot 0 in the later one): the smaller index wins
    two = None
    if len(big) >= 3:
        lo, hi = big[1], big[-1]
        kl = min(int(f.block_n[lo]) - 1, 9)
        two = place_block(f, place_block(f, X0, hi, ldl_fixture(int(f.block_n[hi]), 0, seed=3), K), lo, ldl_fixture(int(f.block_n[lo]), kl, seed=4), K)
        st, _ = o.cholesky_blocks_mw(two)
        assert st == lo + 1
    for pipe in (False, None, True):
        ctx = MwSchurContext(f, limbs=K, pipeline=pipe)
        st, Xc, _ = _x_status(ctx, f, X0)
        assert st == 0 and np.array_equal(Xc, G), pipe
        for (b, k), (Xf, Xt, Lt) in expect.items():
            st, _, dt = _x_status(ctx, f, Xf)
            assert st == b + 1, (pipe, b, k, st)
            assert dt < BOUND, (pipe, b, k, dt)
            st, Xc, dt = _x_status(ctx, f, X0)
            assert st == 0 and np.array_equal(Xc, G), ("no recovery", pipe, b, k)
            st, Xc, dt = _x_status(ctx, f, Xt)
            assert st == 0, ("tiny pivot reported as a failure", pipe, b, k, st)
            assert mw_relerr(Xc, Lt) <= tol(K, 14), (pipe, b, k, np.log2(mw_relerr(Xc, Lt) + 1e-300))
        if two is not None:
            st, _, dt = _x_status(ctx, f, two)
            assert st == lo + 1 and dt < BOUND, (pipe, st, dt)
            st, Xc, _ = _x_status(ctx, f, X0)
            assert st == 0 and np.array_equal(Xc, G)
        ctx.close()


@pytest.mark.parametrize("name", ["ns_8_15_2", "delsarte_3_10", "r41"])
def test_x_block_failure_fp64(name, oracle_built):
    """the same sweep through the fp64 SchurContext, against the fp64 oracle"""
    from clrs_amd.solver import SchurContext
    from oracle.oracle import Oracle
    f = _x_instance(name)
    X0, _ = _iterates(f, 0)
    o = Oracle(f)
    ctx = SchurContext(f)
    st, G, _ = _x_status(ctx, f, X0)
    assert st == 0
    blocks, _ = _fail_blocks(f)
    for b in blocks:
        n = int(f.block_n[b])
        for k in [k for k in PIVOTS if k < n]:
            Xf = place_block(f, X0, b, ldl_fixture(n, k, seed=7 * b + k), 0)
            ost = o.cholesky_blocks(Xf)[0]
            st, _, dt = _x_status(ctx, f, Xf)
            assert st == ost == b + 1 and dt < BOUND, (b, k, st, ost, dt)
            st, Xc, _ = _x_status(ctx, f, X0)
            assert st == 0 and np.array_equal(Xc, G)
            st, _, _ = _x_status(ctx, f, place_block(f, X0, b, ldl_fixture(n, k, seed=7 * b + k, variant="tiny"), 0))
            assert st == 0, (b, k)
    ctx.close()


# ---- S_j per cluster ----------------------------------------------------------------------------------------------------------
def _s_instance(name):
    if name == "p32x5":        # five clusters of at most 32 constraints: k_mw_factor / k_mw_factor_pipe
        return clrs_amd.flatten(random_simple_sdp(4, J=5, n_free=3, max_P=32, max_n=12, definite=True))
    if name == "p40x4":        # four clusters of 40: k_mw_factor_pipe64 (pipeline = True)
        return clrs_amd.flatten(random_simple_sdp(3, J=4, n_free=3, fixed_P=40, max_n=12, definite=True))
    if name == "p56x3":        # three clusters of 56: k_mw_factor_pipe64 by default
        return clrs_amd.flatten(random_simple_sdp(5, J=3, n_free=3, fixed_P=56, max_n=12, definite=True))
    return flat(name)


def _negate(f, Y, clusters):
    Y = Y.copy()
    for b in range(f.n_blocks):
        if int(f.block_cluster[b]) in clusters:
            Y[..., int(f.block_off[b]):int(f.block_off[b + 1])] *= -1.0
    return Y


S_CASES = [("ce_8_15", 5, (1,)), ("p32x5", 5, (3,)), ("p32x5", 4, (2, 4)), ("p40x4", 5, (2,)), ("p40x4", 6, (3, 1)), ("p56x3", 5, (2,)),
           ("threepoint_4", 5, (0,)), ("polyopt40", 4, (0,)), ("ns_8_15_2", 5, (1,)), ("ns_8_15_2", 5, (3,)), ("ns_8_15_2", 5, (4, 1)), ("ns_8_15_2", 6, (2,))]


@pytest.mark.parametrize("name,K,clusters", S_CASES)
def test_cluster_failure_is_the_oracles_code(name, K, clusters, oracle_built):
    """Y negated on the blocks of chosen clusters makes their S_j negative definite: factor() returns min(j) + 1 -- the oracle's code for the GPU's own S --
    in every form: one workgroup, k_mw_factor_pipe (P <= 32), k_mw_factor_pipe64 (33 .. 64), the blocked path with the clusters that ride on its
    launches (ns_8_15_2: the P = 96 cluster failing, or a riding cluster failing beside it), factor_limbs = K - 1.  At once, and the same context then
    factors the good S bit for bit as a fresh one."""
    from clrs_amd.mw import MwSchurContext
    from oracle.oracle import Oracle
    f = _s_instance(name)
    X, Y = _iterates(f, K)
    Yn = _negate(f, Y, set(clusters))
    want = min(clusters) + 1
    o = Oracle(f, mp_bits=320 if K <= 5 else 640)
    forms = [dict(pipeline=False), dict(pipeline=None), dict(pipeline=True)]
    if K in (5, 6):
        forms += [dict(pipeline=False, factor_limbs=K - 1), dict(pipeline=True, factor_limbs=K - 1)]
    ref = None
    for kw in forms:
        fresh = MwSchurContext(f, limbs=K, **kw)
        fresh.compute_S_integrated(fresh.cholesky_blocks(X), Y)
        assert fresh.factor() == 0, kw
        good = fresh.get_factor()
        fresh.close()
        ctx = MwSchurContext(f, limbs=K, **kw)
        Xc = ctx.cholesky_blocks(X)
        for rep in range(2):                      # (the second one is timed: it meets the first one's status words and tags)
            S, _ = ctx.compute_S_integrated(Xc, Yn)
            t0 = time.perf_counter()
            code = ctx.factor()
            dt = time.perf_counter() - t0
            assert code == want, (kw, rep, code, want)
        assert dt < BOUND, (kw, dt)
        if ref is None:
            o.set_S_mw(S)
            ref = o.schur_factor()
            assert ref == want
        ctx.compute_S_integrated(Xc, Y)
        assert ctx.factor() == 0, ("no recovery", kw)
        for a, b in zip(ctx.get_factor(), good):
            assert np.array_equal(a, b), kw
        ctx.close()


@pytest.mark.parametrize("name,clusters", [("p32x5", (3,)), ("p32x5", (4, 2)), ("p40x4", (2,)), ("p56x3", (1,))])
def test_cluster_failure_fp64(name, clusters, oracle_built):
    """the same through the fp64 SchurContext, against the fp64 oracle's own assembly (on instances whose S_j fp64 factors at the good iterate: those of
    cohnelkies(8,15) and Nsphere_packing(8,15) are not positive definite in fp64 -- the reason for the multi-word path)"""
    from clrs_amd.solver import SchurContext
    from oracle.oracle import Oracle
    f = _s_instance(name)
    X, Y = _iterates(f, 0)
    Yn = _negate(f, Y, set(clusters))
    o = Oracle(f)
    ctx = SchurContext(f)
    Xc = ctx.cholesky_blocks(X)
    ctx.compute_S_integrated(Xc, Y)
    assert ctx.factor() == 0
    good = ctx.get_factor()
    for rep in range(2):
        ctx.compute_S_integrated(Xc, Yn)
        t0 = time.perf_counter()
        code = ctx.factor()
        dt = time.perf_counter() - t0
    o.schur_assemble(Xc, Yn)
    assert code == o.schur_factor() == min(clusters) + 1 and dt < BOUND, (code, dt)
    ctx.compute_S_integrated(Xc, Y)
    assert ctx.factor() == 0
    for a, b in zip(ctx.get_factor(), good):
        assert np.array_equal(a, b)
    ctx.close()


# ---- a block of Y in the step length, through the loop -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ns_iterate():
    from clrs_amd.mw import solvesdp_mw
    f = flat("ns_8_15_2")
    r = solvesdp_mw(f, limbs=5, duality_gap_threshold=1e-4, dual_error_threshold=1e-20, primal_error_threshold=1e-20, maxiterations=60)
    assert r.error_code in (0, 2), r.error_code
    return f, r


LOOP_KW = dict(duality_gap_threshold=1e-30, dual_error_threshold=1e-30, primal_error_threshold=1e-30, maxiterations=3)


@pytest.mark.parametrize("k", [0, 7, 8, 20, 31])
def test_y_block_failure_in_the_step_length_ends_the_loop(k, ns_iterate, oracle_built):
    """The iterate of a loose solve of Nsphere_packing(8, 15, [1/2, 1/2]) with its second 32-row block of Y given a pivot -1e-3 D_k at pivot k (rank1_flip):
    X and S_j still factor, the Cholesky of that block of Y in the step length fails (src/solver.jl:1644-1646).  Warm-started there, the loop ends in its
    first iteration with error_code 1 and the failing record's factor and Cholesky statuses 0 -- with the Cholesky of the X and Y blocks through the pipelines
    (k_mw_potrf_x_pipe, the default at these block sides) and without them; the oracle from the same iterate fails at the same place.  (The pipelines took
    the status of a Y block from stage 0, which looks at pivots 0 .. 7 only: from k = 8 on the failure was lost and the loop went on.)"""
    from clrs_amd import _lib
    from clrs_amd.mw import solvesdp_mw
    from oracle.oracle import Oracle
    f, r0 = ns_iterate
    K = 5
    b = [i for i in range(f.n_blocks) if int(f.block_n[i]) == 32][1]
    sl = slice(int(f.block_off[b]), int(f.block_off[b + 1]))
    Y = r0.Y.copy()
    Y[:, sl], _ = rank1_flip(r0.Y[:, sl], k, 1e-3)
    dual = types.SimpleNamespace(x=r0.x, X=r0.X)
    primal = types.SimpleNamespace(y=r0.y, Y=Y)
    o = Oracle(f, mp_bits=320)
    ro = o.solvesdp(start=(r0.x, r0.y if f.n_free else np.zeros((K, 0)), r0.X, Y), **LOOP_KW)
    assert ro["error_code"] == 1 and ro["iterations"] == 0, (ro["error_code"], ro["iterations"])
    assert o.last_failure() == 4, o.last_failure()                    # the Cholesky of a block of Y in the step length
    L = _lib.load()
    try:
        for pipe_x in (1, 0):
            _lib.check(L.clrs_config_set(b"mw_pipeline_x", pipe_x))
            r = solvesdp_mw(f, limbs=K, dualsol=dual, primalsol=primal, **LOOP_KW)
            assert r.error_code == 1 and r.iterations == ro["iterations"], (pipe_x, r.error_code, r.iterations)
            assert r.timings["fail_status"] == (0, 0), (pipe_x, r.timings["fail_status"])
    finally:
        _lib.check(L.clrs_config_set(b"mw_pipeline_x", 1))

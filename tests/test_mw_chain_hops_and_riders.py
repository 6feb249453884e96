"""The main chain of the multi-word interior-point iteration: its in-launch hand-offs and what the Cholesky of the X blocks leaves out.

Three run-time switches, read when a context is created, select between forms that do the SAME floating-point operations in the same order:

* `clrs_config_set("mw_chain_hop", h)`: the three "last workgroup continues" hand-offs of k_mwi_Zi (panels in Zs) and k_mwi_step (panels in Wd;
  eigenvalues in eig and the failure flag) -- 0: release fences (`mwk::wg_last_block`), 1: write-through stores, a drain, a counter and ONE lane's
  acquire in the last arriver, 2: write-through stores and write-through loads, no fence at all (`mwk::wg_last_block_wt`).
* `clrs_config_set("mw_y_riders", r)`: inside the iteration, small contexts form the Y half of the assembly's pairings (T = Y V, GY = V^T T) in extra
  workgroups of the Cholesky launch of the X blocks (k_mw_potrf_x_ride; 1), or in k_mw_zt / k_mw_gram as the stand-alone entry points do (0).
* `clrs_config_set("mw_skip_xfb", s)`: k_mw_potrf_x forms the scaled triangles Xf / Xb (and U^T for them) always (0), or only in contexts where a
  substitution path can read them (1).

Every result must therefore agree BIT FOR BIT between the forms.

The hand-off buffers are reused by every launch, so a last arriver that read a stale L1 or L2 line (the failure the write-through forms could have
and the fence form cannot) would show as a bit difference against the fence form: `test_many_live_contexts_...` runs whole solves in ten live contexts
for that.  These are ordinary solves; nothing is provoked."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import flat

pytestmark = pytest.mark.gpu

SWITCHES = {"mw_chain_hop": (1, (0, 2)), "mw_y_riders": (1, (0,)), "mw_skip_xfb": (1, (0,))}       # name: (default, the other values)
VARIANTS = [("default", {})] + [("%s=%d" % (k, v), {k: v}) for k, (_, others) in SWITCHES.items() for v in others]


def _context(f, cfg, **kw):
    """a context created under the switches `cfg`; the process-wide configuration is back at its defaults afterwards"""
    from clrs_amd import _lib
    from clrs_amd.mw import MwSchurContext
    L = _lib.load()
    try:
        for k, v in cfg.items():
            _lib.check(L.clrs_config_set(k.encode(), v))
        return MwSchurContext(f, **kw)
    finally:
        for k, (default, _) in SWITCHES.items():
            L.clrs_config_set(k.encode(), default)


def _assert_same_solve(a, b, what):
    assert a.error_code == b.error_code and a.status == b.status and a.iterations == b.iterations, (what, a.status, b.status, a.iterations, b.iterations)
    assert np.array_equal(np.asarray(a.history), np.asarray(b.history)), what          # (the table rows carry no wall-clock column)
    for name in ("x", "y", "X", "Y"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)
    assert np.array_equal(a.timings["objectives_limbs"], b.timings["objectives_limbs"]), what


INSTANCES = [
    # (4 limbs, ~209 bits: error thresholds 1e-25 instead of the 256-bit defaults, as test_four_limbs_reach_the_objective_with_thresholds_for_209_bits)
    ("ce_8_15", dict(limbs=4, data_limbs=4), dict(dual_error_threshold=1e-25, primal_error_threshold=1e-25, duality_gap_threshold=1e-12)),
    ("ce_8_15", dict(limbs=5, data_limbs=5), {}),
    ("delsarte_3_10", dict(limbs=5), {}),
    ("polyopt40", dict(limbs=5), {}),                     # PolyOpt 2d = 40: blocks of 21 rows
    # Nsphere_packing(8, 15, [1/2, 1/2, 1/2]) at 6 limbs: the inverse factors of its 48 x 48 blocks do not fit in LDS beside the blocks (MwBlk::inv = 2, formed
    # in memory), so the context keeps the scaled triangles and the one-workgroup congruences -- the fallback, which must be untouched
    ("ns_8_15_3", dict(limbs=6), dict(maxiterations=15)),
]


@pytest.mark.parametrize("name,ckw,skw", INSTANCES, ids=["%s-K%d" % (n, c["limbs"]) for n, c, _ in INSTANCES])
def test_switch_for_switch_bit_identity(name, ckw, skw):
    """whole solves with each switch at each of its values: x, y, X, Y, the objectives' limbs and every table row identical to the default's"""
    from clrs_amd.mw import solvesdp_mw
    f = flat(name)
    res = []
    for label, cfg in VARIANTS:
        ctx = _context(f, cfg, **ckw)
        try:
            res.append((label, solvesdp_mw(f, ctx=ctx, **skw)))
        finally:
            ctx.close()
    ref = res[0][1]
    assert ref.error_code in (0, 2) and ref.iterations >= 10, (ref.status, ref.error_code, ref.iterations)
    if "maxiterations" not in skw:
        assert ref.error_code == 0 and ref.status == "Optimal", (ref.status, ref.error_code)
    for label, r in res[1:]:
        _assert_same_solve(ref, r, (name, label))


def test_substitution_path_of_the_stand_alone_entry_points_is_untouched():
    """a block beyond LDS (101 rows): no inverse factor, the assembly substitutes with the scaled triangles Xf of k_mw_potrf_x -- which such a context
    must go on forming whatever the switch says: factor, S, the factorisation and a solve bit for bit"""
    from tests.util import mw_with_tails, spd_iterates
    K = 5
    f = flat("polyopt_scaled_100")
    X, Y = spd_iterates(f, seed=1)
    X, Y = mw_with_tails(X, K, seed=11), mw_with_tails(Y, K, seed=21)
    rng = np.random.default_rng(11)
    rx, ry = mw_with_tails(rng.standard_normal(f.x_len), K, 1), mw_with_tails(rng.standard_normal(max(f.n_free, 1)), K, 2)[:, :f.n_free]
    out = []
    for skip in (1, 0):
        ctx = _context(f, {"mw_skip_xfb": skip}, limbs=K)
        try:
            Xc = ctx.cholesky_blocks(X)
            S, AY = ctx.compute_S_integrated(Xc, Y)
            assert ctx.factor() == 0
            out.append([Xc, S, AY, *ctx.solve(rx, ry)])
        finally:
            ctx.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_switches_on_a_sharded_solve_on_one_gpu():
    """two ranks on one GPU (contexts of one process, one thread each, in-process exchanges): the hand-offs of k_mwi_Zi and the panels of k_mwi_step are
    the same kernels there (the step lengths themselves travel through the gather and a launch of k_mwi_scalar)"""
    import threading
    import clrs_amd
    from clrs_amd import _lib
    from clrs_amd.mw import LocalGroup, MwSchurContext, shard_problem, solvesdp_mw
    from clrs_amd.problems import cohnelkies_multi
    full = clrs_amd.flatten(cohnelkies_multi(8, 15, [1.0, 1.125, 1.25]))
    world = 2
    L = _lib.load()

    def solve(cfg):
        group = LocalGroup(world)
        out, err = [None] * world, [None] * world
        shards = [shard_problem(full, r, world) for r in range(world)]
        try:                                          # the switches are process-wide and read at creation: create every rank's context here, then let the threads run
            for k, v in cfg.items():
                _lib.check(L.clrs_config_set(k.encode(), v))
            ctxs = [MwSchurContext(s, limbs=5) for s, _ in shards]
        finally:
            for k, (default, _) in SWITCHES.items():
                L.clrs_config_set(k.encode(), default)

        def run(rank):
            try:
                ctxs[rank].comm_init_local(group, rank)
                out[rank] = solvesdp_mw(shards[rank][0], ctx=ctxs[rank], shard_info=shards[rank][1])
            except Exception as e:                  # a failing rank must not leave the others waiting in a collective: nothing to do but report
                err[rank] = e
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        for c in ctxs:
            c.close()
        group.close()
        assert all(e is None for e in err), err
        assert all(o is not None for o in out)
        return out
    ref = solve({})
    assert ref[0].error_code == 0 and ref[0].status == "Optimal"
    for label, cfg in VARIANTS[1:]:
        got = solve(cfg)
        for rank in range(world):
            _assert_same_solve(ref[rank], got[rank], ("sharded", label, rank))


def _one_iteration(f, K, cfg, X, Y):
    """clrs_mw_ipm_set with the iterate (x = 0, y = 0, X, Y), one clrs_mw_ipm_iterate: the record's fields and what clrs_mw_ipm_get returns"""
    from clrs_amd import _lib
    ctx = _context(f, cfg, limbs=K)
    L = ctx.L
    dp = lambda a: a.ctypes.data_as(_lib.p_d)
    try:
        keep = [ctx._data("C"), ctx._data("c"), ctx._data("b") if f.n_free else np.zeros((ctx.data_limbs, 1))]
        data = _lib.IpmData(dp(keep[0]), dp(keep[1]), dp(keep[2]), int(f.maximize), 0, float(f.constant))
        _lib.check(L.clrs_mw_ipm_create_ex(ctx.h, C.byref(data), ctx.data_limbs))
        prm = _lib.IpmParams(0.3, 0.1, 0.9, 1e-30, 1e-30, 1e100, 1e-7, 1, 0)
        _lib.check(L.clrs_mw_ipm_set_params(ctx.h, C.byref(prm)))
        _lib.check(L.clrs_mw_ipm_init(ctx.h, 1e10, 1e10))
        x0, y0 = np.zeros((K, f.x_len)), np.zeros((K, max(f.n_free, 1)))
        Xk, Yk = np.ascontiguousarray(X[:K]), np.ascontiguousarray(Y[:K])
        _lib.check(L.clrs_mw_ipm_set(ctx.h, dp(x0), dp(y0) if f.n_free else None, dp(Xk), dp(Yk)))
        rec = _lib.IpmRecord()
        _lib.check(L.clrs_mw_ipm_iterate(ctx.h, C.byref(rec)))
        fields = tuple(getattr(rec, n) for n, _ in _lib.IpmRecord._fields_)
        out = [np.zeros((K, f.x_len)), np.zeros((K, max(f.n_free, 1))), np.zeros((K, f.xy_len)), np.zeros((K, f.xy_len))]
        _lib.check(L.clrs_mw_ipm_get(ctx.h, dp(out[0]), dp(out[1]) if f.n_free else None, dp(out[2]), dp(out[3])))
        return fields, out
    finally:
        ctx.close()


@pytest.mark.parametrize("K", [4, 5])
def test_one_iteration_from_the_trajectory_fixture(K):
    """tests/golden/ce_8_15_traj.npz: iterates of cohnelkies(8,15) with mu from 1e20 down to 2e-16 and cond(X) up to 2^56.  One whole iteration from
    each of them under every switch: the record and the new iterate agree bit for bit with the default's (an iteration that ends with an error -- the
    last iterate belongs to the 256-bit run and is beyond 4 limbs -- must end with the same error and leave the same iterate)."""
    f = flat("ce_8_15")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ce_8_15_traj.npz"))
    moved = 0
    for s, it in enumerate(g["iters"]):
        ref_rec, ref_out = _one_iteration(f, K, {}, g["X"][s], g["Y"][s])
        assert all(np.all(np.isfinite(a)) for a in ref_out)
        moved += int(not np.array_equal(ref_out[2], np.ascontiguousarray(g["X"][s][:K])))
        for label, cfg in VARIANTS[1:]:
            rec, out = _one_iteration(f, K, cfg, g["X"][s], g["Y"][s])
            assert np.array_equal(np.array(rec, dtype=np.float64), np.array(ref_rec, dtype=np.float64), equal_nan=True), (int(it), label, rec, ref_rec)
            for a, b, name in zip(out, ref_out, "xyXY"):
                assert np.array_equal(a, b), (int(it), label, name)
    assert moved >= 2                                # the comparison is not between iterations that all stopped before their update


def test_many_live_contexts_reuse_the_hand_off_buffers_without_stale_lines():
    """Ten contexts alive at once, two streams each (streams share hardware queues, workgroups of different contexts share compute units and their
    L1s), several whole solves in every context: Zs, Wd and eig are rewritten by every launch, and a last arriver that read a line of an earlier launch
    -- from its compute unit's L1 or its XCD's L2 -- would end with different bits.  Every solve of every context, under both write-through forms, equals
    the fence form's."""
    from clrs_amd.mw import solvesdp_mw
    f = flat("ce_8_3")
    kw = dict(limbs=4, duality_gap_threshold=1e-10, dual_error_threshold=1e-20, primal_error_threshold=1e-20)
    fence = _context(f, {"mw_chain_hop": 0}, limbs=4)
    try:
        ref = solvesdp_mw(f, ctx=fence, **kw)
    finally:
        fence.close()
    assert ref.error_code == 0 and ref.status == "Optimal"
    ctxs = [_context(f, {"mw_chain_hop": 1 + i % 2}, limbs=4) for i in range(10)]
    try:
        for rep in range(3):
            for c in ctxs:
                _assert_same_solve(ref, solvesdp_mw(f, ctx=c, **kw), ("live contexts", rep))
    finally:
        for c in ctxs:
            c.close()

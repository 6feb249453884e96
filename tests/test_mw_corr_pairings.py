"""X^-1 applied as ONE product in k_mwi_Zi: `clrs_config_set("mw_xinv_product", 1)` (default) forms Xv = Xi^T Xi once per iteration on the side
stream (k_mwi_Xv) and every k_mwi_Zi launch of the iteration is M, then Xv M -- two dependent product phases instead of three; 0: Xi^T (Xi M), the
launches and the bits as they were.  The same quantities are summed in another order, so the switch changes last bits, never the trajectory.

(The file is named after the change it came with; the other half of that change, the corrector's right-hand side from pairings with X^-1 V, is not
in the code: DESIGN.md section 5.10.  SWITCHES lists what exists; every test below runs with all of it on against all of it off.)"""
import numpy as np
import pytest

from tests.util import flat, mw_diff, random_simple_sdp

pytestmark = pytest.mark.gpu

SWITCHES = ("mw_xinv_product",)
ON, OFF = {k: 1 for k in SWITCHES}, {k: 0 for k in SWITCHES}
DEFAULTS = {"mw_xinv_product": 1, "mw_stream_words": 1, "mw_affine_corrector": 1}
TOL4 = dict(duality_gap_threshold=1e-10, dual_error_threshold=1e-20, primal_error_threshold=1e-20)      # ce_8_3 at 4 limbs, as test_stream_words_and_events_give_the_same_solve


def _solve(f, cfg, ckw, **skw):
    """a solve in a context of its own under the switches `cfg` (most are read when the context is created, `mw_affine_corrector` when the iteration is:
    they stay set until the solve has returned); the process-wide configuration is back at its defaults afterwards"""
    from clrs_amd import _lib
    from clrs_amd.mw import MwSchurContext, solvesdp_mw
    L = _lib.load()
    ctx = None
    try:
        for k, v in cfg.items():
            _lib.check(L.clrs_config_set(k.encode(), v))
        ctx = MwSchurContext(f, **ckw)
        return solvesdp_mw(f, ctx=ctx, limbs=ckw["limbs"], **skw)
    finally:
        for k, v in DEFAULTS.items():
            L.clrs_config_set(k.encode(), v)
        if ctx is not None:
            ctx.close()


def _assert_same_bits(a, b, what):
    assert a.error_code == b.error_code and a.status == b.status and a.iterations == b.iterations, (what, a.status, b.status, a.iterations, b.iterations)
    assert np.array_equal(np.asarray(a.history), np.asarray(b.history)), what
    for name in ("x", "y", "X", "Y"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


def _assert_same_trajectory(a, b, what):
    """status, error code and iteration count equal; mu, both step lengths and beta_c of every iteration to 1e-8 (the tolerance of
    test_device_loop_follows_the_oracle_on_random_sdps against the oracle)"""
    assert a.error_code == b.error_code and a.status == b.status and a.iterations == b.iterations, (what, a.status, b.status, a.iterations, b.iterations)
    ha, hb = np.asarray(a.history), np.asarray(b.history)
    assert ha.shape == hb.shape and ha.shape[0] >= 1, (what, ha.shape, hb.shape)
    for it in range(hb.shape[0]):
        for col in (1, 8, 9, 10):
            assert abs(ha[it, col] - hb[it, col]) <= 1e-8 * max(abs(hb[it, col]), 1e-300), (what, it, col, ha[it, col], hb[it, col])


def _iterate_distance(a, b):
    """largest |a - b| over x, y, X, Y, limbs summed, each array relative to its largest entry"""
    worst = 0.0
    for name in ("x", "y", "X", "Y"):
        u, v = np.atleast_2d(getattr(a, name)), np.atleast_2d(getattr(b, name))
        scale = float(np.max(np.abs(v[0])))
        if scale == 0.0:
            assert not np.any(u), name
            continue
        worst = max(worst, float(np.max(np.abs(mw_diff(u, v)))) / scale)
    return worst


@pytest.mark.parametrize("cfg", [ON, OFF], ids=["on", "off"])
def test_stream_words_and_events_give_the_same_solve_under_the_switches(cfg):
    """ce_8_3 at 4 limbs: the two streams synchronised by words, then by events only -- same kernels, same order of operations, whatever the value of the
    switch: the new launch and the new buffer are ordered by both forms"""
    f = flat("ce_8_3")
    a = _solve(f, {**cfg, "mw_stream_words": 1}, dict(limbs=4), **TOL4)
    b = _solve(f, {**cfg, "mw_stream_words": 0}, dict(limbs=4), **TOL4)
    assert a.error_code == 0 and a.status == "Optimal"
    _assert_same_bits(a, b, cfg)


def test_switched_off_twice_is_one_solve():
    """the switch at 0 is a deterministic path of its own (what the comparisons below are made against)"""
    f = flat("ce_8_3")
    _assert_same_bits(_solve(f, OFF, dict(limbs=4), **TOL4), _solve(f, OFF, dict(limbs=4), **TOL4), "off, twice")


def _random1():
    import clrs_amd
    return clrs_amd.flatten(random_simple_sdp(seed=1, J=3, n_free=1, definite=True))


@pytest.mark.parametrize("name", ["ce_8_3", "random1"])
def test_same_trajectory(name):
    if name == "ce_8_3":
        f, ckw, skw = flat("ce_8_3"), dict(limbs=4), TOL4
    else:
        f, ckw, skw = _random1(), dict(limbs=5), dict(maxiterations=12)
    on, off = _solve(f, ON, ckw, **skw), _solve(f, OFF, ckw, **skw)
    assert not all(np.array_equal(getattr(on, n), getattr(off, n)) for n in ("x", "y", "X", "Y")), "the switch changed nothing: the new path did not run"
    _assert_same_trajectory(on, off, name)


def test_size_of_the_change_against_the_affine_corrector():
    """x, y, X, Y after 1 and after 10 iterations of cohnelkies(8,15) at 5 limbs, switches on against off, set against a re-association of the same right-hand
    side that the library has had for long: `mw_affine_corrector` 1 against 0 (rhs0 + mu_c tau against the right-hand side formed with mu_c inside), both
    with the new switches off.  Both forms are bounded by the same cond(X)-amplified unit round-off; four bits (a factor 16) are allowed for the different
    number of roundings.  The instance is the workload of bench.py: the affine corrector is on there, and its X is the ill-conditioned one the change is for.
    Measured (MI355X): 8.87e-53 against 5.06e-53 after one iteration, 1.20e-29 against 1.18e-29 after ten (with other instances)."""
    f = flat("ce_8_15")
    ckw = dict(limbs=5, data_limbs=5)
    for its in (1, 10):
        off = _solve(f, OFF, ckw, maxiterations=its)
        on = _solve(f, ON, ckw, maxiterations=its)
        noaff = _solve(f, {**OFF, "mw_affine_corrector": 0}, ckw, maxiterations=its)
        assert on.iterations == off.iterations == noaff.iterations == its
        new, yard = _iterate_distance(on, off), _iterate_distance(noaff, off)
        print("iterations %d: switches on against off %.3e (2^%.1f), affine corrector 0 against 1 %.3e (2^%.1f)" %
              (its, new, np.log2(new) if new else -np.inf, yard, np.log2(yard) if yard else -np.inf))
        assert yard > 0.0, its
        assert new <= 16.0 * yard, (its, new, yard)


def _mixed_sdp(seed, J):
    """every cluster: two low-rank blocks of different sides (5 and 11) and a 1 x 1 dense block, one rank-1 term per constraint and block"""
    from clrs_amd.sdp import Block, ClusteredLowRankSDP, HiLo, LowRankMat
    rng = np.random.default_rng(seed)
    P, blocks, B, c, C = 6, [], [], [], []
    for _ in range(J):
        cl = []
        for n in (5, 11):
            V = rng.standard_normal((P, n))
            lam = rng.uniform(0.5, 1.5, P) * rng.choice([-1.0, 1.0], P)
            cl.append(Block(m=1, delta=n, entries={(0, 0): {p: LowRankMat(np.array([lam[p]]), V[p:p + 1, :], V[p:p + 1, :]) for p in range(P)}}, name="lr"))
        cl.append(Block(m=1, delta=1, entries={(0, 0): {p: HiLo.of(rng.standard_normal((1, 1))) for p in (0, 2, 3, 5)}}, name="dense"))
        blocks.append(cl)
        C.append([np.zeros((5, 5)), np.zeros((11, 11)), np.zeros((1, 1))])
        B.append(rng.standard_normal((P, 1)))
        c.append(rng.standard_normal(P))
    sdp = ClusteredLowRankSDP(maximize=True, constant=0.0, blocks=blocks, B=B, c=c, C=C, b=rng.standard_normal(1), names={})
    sdp.check()
    return sdp


@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("J", [1, 2, 4])
@pytest.mark.parametrize("side", [2, 3, 9, 16, 24, "mixed"])
def test_small_shapes_of_the_lane_maps(side, J, K):
    """one low-rank block per cluster of fewer rows than the eight lanes of an entry (2, 3), of no multiple of them (9), of the workload's side (16) and of
    the last side before the tiled path (24); a cluster of two low-rank blocks of different sides and a 1 x 1 dense block; one, two and four clusters; 4
    limbs and 5 (the reduced-limb dispatch of the predictor's launches).  Six iterations, switches on against off."""
    import clrs_amd
    if side == "mixed":
        sdp = _mixed_sdp(700 + J, J)
    else:
        sdp = random_simple_sdp(500 + 10 * side + J, J=J, n_free=1, fixed_P=min(6, side * (side + 1) // 2 - 1), max_n=side, lr_blocks=1)      # (fewer constraints than independent pairings)
    f = clrs_amd.flatten(sdp)
    ckw = dict(limbs=K)
    on, off = _solve(f, ON, ckw, maxiterations=6), _solve(f, OFF, ckw, maxiterations=6)
    _assert_same_trajectory(on, off, (side, J, K))


def test_the_tiled_path_is_untouched():
    """blocks of 40 rows take the tiled products (k_mwi_bmm), which know nothing of the switch: bit for bit the solve with the switch off"""
    import clrs_amd
    f = clrs_amd.flatten(random_simple_sdp(seed=10, J=2, n_free=5, fixed_P=70, max_n=40, lr_blocks=2))
    ckw = dict(limbs=5)
    _assert_same_bits(_solve(f, ON, ckw, maxiterations=4), _solve(f, OFF, ckw, maxiterations=4), "tiled")


@pytest.mark.parametrize("kw", [dict(seed=21, J=5, n_free=2, definite=True), dict(seed=22, J=2, n_free=0, definite=True)], ids=["J5", "no_free_variables"])
def test_contexts_without_the_affine_corrector(kw):
    """five clusters, and no free variables: the corrector's right-hand side is formed with mu_c inside (k_mwi_Zi which = 0 on the main stream) -- the
    product with Xv serves these launches too"""
    import clrs_amd
    f = clrs_amd.flatten(random_simple_sdp(**kw))
    ckw = dict(limbs=5)
    on, off = _solve(f, ON, ckw, maxiterations=8), _solve(f, OFF, ckw, maxiterations=8)
    _assert_same_trajectory(on, off, kw)

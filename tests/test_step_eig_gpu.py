"""The step length's eigenvalue kernels against exact inertia counts (tests/step_eig_util.py).

Part 1, clrs_test_min_eig: the three fp64 smallest-eigenvalue routines (form 0: wg_min_eig32, form 1: wg_min_eig, form 2: the fp64 loop's ipm_min_eig) on
the case list, at every template switch and loop-tail length, within n 2^-47 ||A||_2.
Part 2, clrs_mw_test_step_eig: the congruence forms of mwi_step_body on M = L L^T, dM = L W0 L^T formed exactly and rounded to K limbs, within
(n + 1) 2^-47 ||W0||_2 of the pencil's smallest eigenvalue.

Forms of mwi_step_body that NO context can reach, whatever the sides of its blocks (so the coverage test at the end of this module does not ask for them):
  * inv_path 0 (substitutions, W in LDS or in global memory; Y factored by wg_potrf inside the step kernel) and inv_path 1 (Y factored inside the kernel beside
    explicit inverse factors).  clrs_mw_ipm_create_ex refuses a context unless `stepd = (step_w_lds ? 2 : 1) * nnK + step_rest <= lim` ("device-resident
    multi-word iteration needs PSD blocks that fit in LDS").  step_rest holds 3 K maxn + maxn^2, so every block passes `one = n^2 K + 3 K n <= lim` of
    clrs_mw.hip mw_stage_lds and carries an inverse factor (`k.inv = ... two <= lim ? 1 : one <= lim ? 2 : 0` is never 0): any_xinv && !any_xsub.  And
    `step_need2 = nnK + maxn^2 + 3 maxn + 2 MW_NT + 8` is below stepd, so `st->y_with_x = st->any_xinv && !st->any_xsub && step_need2 <= lim` always holds
    and mw_ipm_launch_step takes `ip = st->y_with_x ? 2 : st->step_inv ? 1 : 0` = 2.  (The same bound caps the sides: 79 rows at 2 limbs, 61 at 4, 55 at 5.)
  * inv_path 2 in ONE workgroup (gridDim.z == 1, mwi_step_congruence_inv): `st->zs_step = std::max<int>(old_rule, ...)` with old_rule >= MWI_ZS = 4; with one
    workgroup per congruence only the tiled form (inv_path 3, blocks beyond 24 rows) runs.
What runs: inv_path 2 in column panels (SW = 4, and SW = 16 one-column panels), inv_path 3, 1 x 1 blocks, factors in K and in K - 1 limbs, wg_min_eig32 and
(beyond 64 rows) wg_min_eig; Y failures through `yfail` of the Cholesky launch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.step_eig_util import (CONGRUENCE_KINDS, assert_min_eig, assert_min_eig_all, cases_budget, check_min_eig, congruence_pair, easy_pair,      # noqa: E402
                                 eig_cases, eig_tol, limbs_to_mp, scalar_pair)

pytestmark = pytest.mark.gpu

NS_32 = (2, 3, 4, 5, 6, 8, 9, 15, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 63, 64)      # forms 0 and 2
NS_LDS = (1, 2, 3, 17, 64, 65, 80, 100, 128)                                          # form 1
EPS = 2.0 ** -53
WORST = {}                                                                            # form -> (error in n eps ||A||, n, case): printed, recorded in DESIGN.md


# ---- part 1: the eigenvalue routines -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(NS_32) | set(NS_LDS)))
def test_min_eig_routines_against_inertia_counts(n):
    from clrs_amd.mw import min_eig_hook
    cases = eig_cases(n, limit=cases_budget(n))
    A = np.stack([a for _, a in cases])
    forms = ([0, 2] if n in NS_32 else []) + ([1] if n in NS_LDS else [])
    got = {f: min_eig_hook(f, A) for f in forms}                          # one launch per (form, n): every case of this n in it
    for i, (name, a) in enumerate(cases):
        vals = [float(got[f][i]) for f in forms]
        if name == "zero":
            assert all(abs(v) <= 1e-280 for v in vals), (n, forms, vals)
            continue
        ref = float(np.linalg.eigvalsh(a)[0])                             # (for the printed figures only)
        unit = n * EPS * float(np.linalg.norm(a, 2))
        for f, v in zip(forms, vals):
            e = abs(v - ref) / unit
            if e > WORST.get(f, (0.0,))[0]:
                WORST[f] = (e, n, name)
        print(f"n = {n:3d} {name:16s} " + " ".join(f"form {f}: {abs(v - ref) / unit:7.3f}" for f, v in zip(forms, vals)) + "  (n eps ||A||)")
        assert_min_eig_all(vals, a, eig_tol(n, a), what=f"n = {n}, {name}, forms {forms}")
    print("worst so far, form -> (error / (n eps ||A||), n, case):", WORST)


def test_min_eig_hook_refuses_sizes_outside_its_ranges():
    from clrs_amd._lib import ClrsError
    from clrs_amd.mw import min_eig_hook
    for form, n in ((0, 1), (0, 65), (2, 1), (2, 65), (1, 129), (3, 8), (-1, 8)):
        with pytest.raises(ClrsError) as e:
            min_eig_hook(form, np.zeros((1, n, n)))
        assert e.value.code == -1 and "clrs_test_min_eig" in str(e.value)


# ---- part 2: the congruence forms ----------------------------------------------------------------------------------------------------------
# name -> limbs, the SDP (tests.util.random_simple_sdp: `sides` is what it yields, asserted), options of the context, library switches
CONTEXTS = {
    "k2_20_blocks":      dict(K=2, sdp=dict(seed=0, J=7, max_n=9), sides=[6, 1, 3, 6, 1, 8, 8, 3, 9, 9, 7, 5, 1, 6, 2, 3, 4, 1, 5, 1]),
    "k2_20_blocks_xv0":  dict(K=2, sdp=dict(seed=0, J=7, max_n=9), sides=[6, 1, 3, 6, 1, 8, 8, 3, 9, 9, 7, 5, 1, 6, 2, 3, 4, 1, 5, 1], config={"mw_xinv_product": 0}),
    "k4_3_blocks":       dict(K=4, sdp=dict(seed=86, J=1, max_n=17), sides=[16, 11, 17]),
    "k5_mixed_24":       dict(K=5, sdp=dict(seed=0, J=3, max_n=24), sides=[8, 1, 2, 16, 1, 2, 12, 24, 18, 1, 1]),                     # factors in 4 limbs
    "k5_mixed_24_full":  dict(K=5, sdp=dict(seed=0, J=3, max_n=24), sides=[8, 1, 2, 16, 1, 2, 12, 24, 18, 1, 1], factor_limbs=5),
    "k5_mixed_24_nopipe": dict(K=5, sdp=dict(seed=0, J=3, max_n=24), sides=[8, 1, 2, 16, 1, 2, 12, 24, 18, 1, 1], config={"mw_pipeline_x": 0}),
    "k2_one_25":         dict(K=2, sdp=dict(seed=0, J=1, max_n=25, lr_blocks=1), sides=[25, 1]),                                      # beyond 24 rows: tiled products
    "k4_one_32":         dict(K=4, sdp=dict(seed=6, J=1, max_n=32, lr_blocks=1), sides=[32]),
    "k5_one_33":         dict(K=5, sdp=dict(seed=0, J=1, max_n=33, lr_blocks=1), sides=[1, 33]),
    "k2_one_48":         dict(K=2, sdp=dict(seed=1, J=1, max_n=48, lr_blocks=1), sides=[48]),
    "k2_one_64":         dict(K=2, sdp=dict(seed=0, J=1, max_n=64, lr_blocks=1), sides=[64, 1]),
    "k4_one_61":         dict(K=4, sdp=dict(seed=0, J=1, max_n=61, lr_blocks=1), sides=[61]),                                         # the largest side 4 limbs take
    "k5_one_55":         dict(K=5, sdp=dict(seed=2, J=1, max_n=55, lr_blocks=1), sides=[55, 1]),                                      # ... and 5 limbs
    "k2_one_72":         dict(K=2, sdp=dict(seed=6, J=1, max_n=72, lr_blocks=1), sides=[72, 1]),                                      # wg_min_eig inside the step kernel
}
RUNS = {}                                                                              # name -> the record of run_context


def _flat(spec):
    import clrs_amd
    from tests.util import random_simple_sdp
    f = clrs_amd.flatten(random_simple_sdp(n_free=2, fixed_P=3, **spec["sdp"]))
    sides = [int(v) for v in f.block_n]
    assert sides == spec["sides"], sides
    return f, sides


def _pairs(sides, K, diag_bits=16):
    """per block the hard pair (M, dM, ||W0||) and the easy one; 1 x 1 blocks: two scalar pairs with their exact ratios"""
    hard, easy = [], []
    for b, n in enumerate(sides):
        if n == 1:
            hard.append(scalar_pair(K, seed=2 * b))
            easy.append(scalar_pair(K, seed=2 * b + 1))
            continue
        M, dM, W0, _ = congruence_pair(n, K, CONGRUENCE_KINDS[(b + n) % len(CONGRUENCE_KINDS)], seed=b, diag_bits=diag_bits)
        assert np.linalg.cond(M[0].reshape(n, n)) <= 2.0 ** 40
        hard.append((M, dM, float(np.linalg.norm(W0, 2))))
        Me, dMe, We = easy_pair(n, K, seed=b)
        easy.append((Me, dMe, float(np.max(np.abs(We)))))
    return hard, easy


def _place(f, K, blocks):
    """planar (K, xy_len) from one (K, n * n) array per block"""
    out = np.zeros((K, f.xy_len))
    for b, a in enumerate(blocks):
        out[:, int(f.block_off[b]):int(f.block_off[b + 1])] = a
    return out


def check_block(eig, n, pair, what):
    """the assertions of one (block, which): pair = (M, dM, ||W0||) or, 1 x 1, (M, dM, exact ratio)"""
    import mpmath as mp
    M, dM, third = pair
    if n == 1:
        with mp.workprec(400):
            assert abs(mp.mpf(float(eig)) - third) <= mp.ldexp(abs(third), -50), (what, eig, third)      # no 1e-5 on this branch (src/solver.jl:1637-1641)
        return
    assert_min_eig(float(eig) + 1e-5, limbs_to_mp(dM, n), (n + 1) * 2.0 ** -47 * third, B=limbs_to_mp(M, n), what=what)


def run_context(name):
    """both runs of one context (cached): hard pairs in (X, dX) and easy ones in (Y, dY), then the other way round"""
    if name in RUNS:
        return RUNS[name]
    from clrs_amd import _lib
    from clrs_amd.mw import MwSchurContext
    spec = CONTEXTS[name]
    K = spec["K"]
    f, sides = _flat(spec)
    hard, easy = _pairs(sides, K)
    L = _lib.load()
    defaults = {"mw_xinv_product": 1, "mw_pipeline_x": 1}
    try:
        for key, v in spec.get("config", {}).items():
            assert L.clrs_config_set(key.encode(), v) == 0
        ctx = MwSchurContext(f, limbs=K, factor_limbs=spec.get("factor_limbs"))
    finally:
        for key in spec.get("config", {}):
            L.clrs_config_set(key.encode(), defaults[key])
    ctx.ipm_create()
    Mh, dMh = _place(f, K, [p[0] for p in hard]), _place(f, K, [p[1] for p in hard])
    Me, dMe = _place(f, K, [p[0] for p in easy]), _place(f, K, [p[1] for p in easy])
    eig_x, info_x = ctx.test_step_eig(Mh, Me, dMh, dMe)
    eig_y, info_y = ctx.test_step_eig(Me, Mh, dMe, dMh)
    RUNS[name] = dict(f=f, sides=sides, hard=hard, easy=easy, ctx=ctx, K=K, runs=[(eig_x, info_x, (hard, easy)), (eig_y, info_y, (easy, hard))],
                      mats=dict(Mh=Mh, dMh=dMh, Me=Me, dMe=dMe))
    return RUNS[name]


@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_congruence_forms_against_inertia_counts(name):
    r = run_context(name)
    for eig, info, pairs in r["runs"]:
        print(name, info)
        assert info["fail"] == 0, info
        for which in (0, 1):
            for b, n in enumerate(r["sides"]):
                check_block(eig[which, b], n, pairs[which][b], f"{name}: block {b} (n = {n}), which = {which}, plan {info}")
    assert r["runs"][0][1] == r["runs"][1][1]                     # the plan is the context's, not the data's
    if name.endswith("_full"):
        assert r["runs"][0][1]["kf"] == r["K"]
    if name == "k5_mixed_24":
        assert r["runs"][0][1]["kf"] == r["K"] - 1


@pytest.mark.parametrize("K", (4, 5))
def test_cond_2_80_needs_the_multiword_products(K):
    """cond(M) about 2^80: the kernel's K-limb congruence passes the assertion that the same congruence in fp64 (numpy, with the exact factor L) fails"""
    import clrs_amd
    from clrs_amd.mw import MwSchurContext
    from tests.util import random_simple_sdp
    n = 8
    f = clrs_amd.flatten(random_simple_sdp(11, J=1, n_free=2, fixed_P=3, max_n=n, lr_blocks=1))
    sides = [int(v) for v in f.block_n]
    b = sides.index(n)
    M, dM, W0, Lx = congruence_pair(n, K, "random", seed=3, diag_bits=38)
    assert 2.0 ** 72 <= np.linalg.cond(Lx) ** 2 <= 2.0 ** 84
    tol = (n + 1) * 2.0 ** -47 * float(np.linalg.norm(W0, 2))
    Mm, dMm = limbs_to_mp(M, n), limbs_to_mp(dM, n)
    Wf = np.linalg.solve(Lx, np.linalg.solve(Lx, dM[0].reshape(n, n)).T)
    assert check_min_eig(float(np.linalg.eigvalsh(0.5 * (Wf + Wf.T))[0]), dMm, tol, B=Mm) != (True, True)
    blocks_M, blocks_dM = [], []
    for bb, nn in enumerate(sides):
        if bb == b:
            blocks_M.append(M); blocks_dM.append(dM)
        else:
            s = scalar_pair(K, seed=bb)
            blocks_M.append(s[0]); blocks_dM.append(s[1])
    ctx = MwSchurContext(f, limbs=K)
    ctx.ipm_create()
    XM, XdM = _place(f, K, blocks_M), _place(f, K, blocks_dM)
    eig, info = ctx.test_step_eig(XM, XM, XdM, XdM)
    ctx.close()
    assert info["fail"] == 0
    for which in (0, 1):
        assert_min_eig(float(eig[which, b]) + 1e-5, dMm, tol, B=Mm, what=f"K = {K}, which = {which}, {info}")


@pytest.mark.parametrize("name,n_bad,pivot", (("k2_20_blocks", 8, 5), ("k4_3_blocks", 17, 12), ("k2_one_25", 25, 12)))
def test_an_indefinite_Y_block_fails_alone(name, n_bad, pivot):
    """Y of one block fails its Cholesky at a chosen pivot: the failure flag is set, that block's eigenvalue is 0, every other value is still right
    (the factorisation of Y that rides on the Cholesky launch reports it, `yfail`; panels -- the workgroups beyond the first return early -- and the tiled form)."""
    from tests.util import ldl_fixture, mw_from_double
    r = run_context(name)
    f, K, sides, m = r["f"], r["K"], r["sides"], r["mats"]
    b = sides.index(n_bad)
    Y = m["Mh"].copy()
    Y[:, int(f.block_off[b]):int(f.block_off[b + 1])] = mw_from_double(ldl_fixture(n_bad, pivot, seed=b, variant="fail").reshape(-1, order="F"), K)
    eig, info = r["ctx"].test_step_eig(m["Me"], Y, m["dMe"], m["dMh"])
    assert info["fail"] != 0 and eig[1, b] == 0.0, (info, eig[1, b])
    assert {k: v for k, v in info.items() if k != "fail"} == {k: v for k, v in r["runs"][0][1].items() if k != "fail"}
    for which, pairs in ((0, r["easy"]), (1, r["hard"])):
        for bb, n in enumerate(sides):
            if (which, bb) != (1, b):
                check_block(eig[which, bb], n, pairs[bb], f"{name} with Y block {b} indefinite: block {bb} (n = {n}), which = {which}")
    # and without it the flag is clear again
    eig2, info2 = r["ctx"].test_step_eig(m["Me"], m["Mh"], m["dMe"], m["dMh"])
    assert info2["fail"] == 0 and np.array_equal(eig2, r["runs"][1][0])


def test_a_solve_after_the_hook_is_the_solve_of_a_fresh_context():
    from clrs_amd.mw import MwSchurContext, solvesdp_mw
    r = run_context("k5_mixed_24")
    f, K, m = r["f"], r["K"], r["mats"]
    r["ctx"].test_step_eig(m["Mh"], m["Me"], m["dMh"], m["dMe"])
    kw = dict(maxiterations=6, omega_p=10.0, omega_d=10.0)
    a = solvesdp_mw(f, ctx=r["ctx"], **kw)
    fresh = MwSchurContext(f, limbs=K)
    b = solvesdp_mw(f, ctx=fresh, **kw)
    fresh.close()
    assert a.iterations == b.iterations > 0 and a.error_code == b.error_code
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history)
    for name in ("x", "y", "X", "Y"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_every_reachable_form_of_the_step_kernel_ran():
    """over the plans the contexts of this module chose (those not run yet in this session are run now): see the module docstring for the forms no context reaches"""
    recs = []
    for name in sorted(CONTEXTS):
        r = run_context(name)
        recs.append((name, r["K"], r["sides"], r["runs"][0][1]))
    for rec in recs:
        print(rec[0], rec[3])
    ip = lambda v: [r for r in recs if r[3]["ip"] == v]
    assert not ip(0) and not ip(1), "a form the module docstring calls unreachable ran: extend the tests to check it"
    panels = ip(2)
    assert panels and all(r[3]["zs_step"] >= 4 and r[3]["z_tiled"] == 0 for r in panels)
    wide = lambda r, n: r[3]["zs_step"] >= n and n <= 16                       # mwi_step_panels: one column per workgroup, SW = 16
    assert any(n > 1 and wide(r, n) for r in panels for n in r[2]), "inverse factors, one-column panels (SW = 16)"
    assert any(n > 1 and not wide(r, n) for r in panels for n in r[2]), "inverse factors, panels of several columns (SW = 4)"
    assert any(r[3]["zs_step"] > min(n for n in r[2] if n > 1) for r in panels), "gridDim.z beyond a block's side"
    assert ip(3) and all(r[3]["z_tiled"] == 1 for r in ip(3)), "tiled products"
    assert any(1 in r[2] for r in recs), "1 x 1 blocks"
    assert any(r[3]["kf"] < r[1] for r in recs) and any(r[3]["kf"] == r[1] == 5 for r in recs), "reduced and full factor limbs at K = 5"
    assert any(max(r[2]) > 64 for r in recs) and {len(r[2]) for r in recs} >= {1, 3, 20}
    assert {r[1] for r in recs} == {2, 4, 5}
    assert {n for r in recs for n in r[2]} >= {1, 2, 3, 8, 9, 16, 17, 24, 25, 32, 33, 48, 64}
    for r in RUNS.values():
        r["ctx"].close()
    RUNS.clear()

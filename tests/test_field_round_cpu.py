"""Rounding to a number field by integer relations, without a GPU: csrc/clrs_mw_field_round_arith.h compiled for the host against planted
elements, against an independent restatement of the reference's clindep, on the edge cases and on its own invariants; the binding; the refusals of the C entry;
and `kernel_vectors(field=...)` with host stand-ins on a rank-one pair and on the 320-bit oracle's solutions of the two Delsarte problems over QQ(sqrt 5)."""
import ctypes as C
import functools
import json
import os
import re
from fractions import Fraction as F

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd.mw import to_limbs
from clrs_amd.rounding import KernelVectorError, NumberField, RoundingSettings
from tests import field_round_util as fu
from tests import kernel_vectors_util as ku
from tests import lll_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "delsarte_field_kernel.json")
COUNT = 6


@functools.lru_cache(maxsize=None)
def _planted_run(name, h):
    f = fu.field(name)
    limbs, eb = fu.planted_limbs(f.degree, h), fu.planted_errbound(f.degree, h)
    elems, vals = fu.planted(name, h, COUNT)
    return f, limbs, eb, elems, vals, fu.host_round(vals, f, limbs, errbound=eb)


# ---- the number field ----------------------------------------------------------------------------------------------------------------------------------------
def test_number_field_checks_its_generator():
    f = fu.field("x4-x-1")
    assert f.degree == 4 and f.powers(6).shape == (6, 4) and f.powers(10).shape == (10, 4)
    assert f.powers(4)[0, 0] == 1.0 and not f.powers(4)[1:, 0].any()
    with mp.workprec(400):
        with pytest.raises(ValueError, match="no root"):
            NumberField([-5, 0, 1], mp.mpf("2.2360679"))
        g = NumberField([-5, 0, 1], mp.sqrt(5))
        assert g.powers(6).shape == (6, 2)
        with pytest.raises(ValueError, match="limbs need"):
            g.powers(10)                                                        # a root to 400 bits does not carry the 514 of ten limbs
    limbs = to_limbs([fu.field("x2-2").g], 5)[:, 0]
    assert NumberField([-2, 0, 1], limbs).prec == 265
    with pytest.raises(ValueError):
        NumberField([1], 1.0)
    with pytest.raises(ValueError, match="degree 1"):
        rounding.round_to_field(np.zeros(1), NumberField([-1, 2], mp.mpf(1) / 2), 4)


# ---- planted elements ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h", fu.PLANTED)
def test_planted_elements_come_back(name, h):
    f, limbs, eb, elems, vals, r = _planted_run(name, h)
    assert 53 * limbs - 16 >= (f.degree + 1) * (h + 8) + 16
    print(name, h, "limbs", limbs, "rungs", list(r.rung), "exchanges", list(r.exchanges), "max err", r.err.max(), "errbound", eb)
    assert (r.status == 0).all() and (r.path == 0).all()
    assert [tuple(c) for c in r.coeffs] == elems                                # every one, none skipped
    assert (r.err < eb).all() and (r.rung % 5 == 1).all() and (r.rungs == (r.rung + 4) // 5).all()
    # vq = -(sum a_k g^(k-1)) / a_0: one sum of deg products and one division in K limbs, a few units of 2^(-53 K + K) each, against the size of the terms
    with mp.workprec(fu.MP_PREC):
        gp = f.power_values(prec=fu.MP_PREC)
        size = max(mp.fsum(abs(x) * abs(g) for x, g in zip(e, gp)) for e in elems) + 1
        bound = size * mp.ldexp(1, -53 * limbs + limbs + 6)
        assert fu.vq_error(r.vq, elems, f) * 1 <= bound
    # the relation itself: primitive, and the planted one up to sign
    for a, e in zip(r.rel, elems):
        assert functools.reduce(np.gcd, [abs(int(x)) for x in a]) == 1 and int(a[0]) != 0
        assert all(F(-int(a[k + 1]), int(a[0])) == e[k] for k in range(f.degree))


@pytest.mark.parametrize("name,h", fu.PLANTED)
def test_planted_elements_agree_with_the_restated_clindep(name, h):
    f, limbs, eb, elems, vals, r = _planted_run(name, h)
    n = 3 if h < 40 else 2                                                       # (the Fraction LLL from scratch at every rung is slow at 120 bits)
    ref = fu.restated(vals[:, :n], f, limbs, eb)
    print(name, h, "restated rungs", [p for _, p in ref], "ours", list(r.rung[:n]))
    assert [e for e, _ in ref] == elems[:n] == [tuple(c) for c in r.coeffs[:n]]


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------------------------------
def _vals(xs, limbs):
    with mp.workprec(fu.MP_PREC):
        return to_limbs([mp.mpf(x) if not callable(x) else x() for x in xs], limbs)


def test_zero_rationals_and_the_generator():
    f, limbs = fu.field("x2-5"), 4
    vals = _vals([0, 3, mp.mpf(-7) / 3, lambda: f.g, lambda: -f.g / 2, lambda: mp.mpf(1) / 3 + f.g], limbs)
    r = fu.host_round(vals, f, limbs, errbound=2.0 ** -40)
    assert (r.status == 0).all()
    assert [tuple(c) for c in r.coeffs] == [(0, 0), (3, 0), (F(-7, 3), 0), (0, 1), (0, F(-1, 2)), (F(1, 3), 1)]
    assert r.rung[0] == 1 and r.err[0] == 0.0 and not r.vq[:, 0].any()          # v = 0: the zero element at the first rung
    for name in ("x3-2", "x4-x-1"):                                              # rationals have zero higher coefficients in every degree
        g = fu.field(name)
        r = fu.host_round(_vals([0, 5, mp.mpf(22) / 7, lambda: g.g], 4), g, 4, errbound=2.0 ** -50)
        z = (0,) * (g.degree - 2)
        assert (r.status == 0).all() and [tuple(c) for c in r.coeffs] == [(0, 0) + z, (5, 0) + z, (F(22, 7), 0) + z, (0, 1) + z] and r.rung[0] == 1


@pytest.mark.parametrize("name,h", [("x2-5", 4), ("x2-2", 4), ("x3-2", 4), ("x4-x-1", 4)])
def test_noise_below_the_bound_changes_nothing(name, h):
    """noise of errbound / 2^10 on v moves the residual of the planted relation by |a_0| errbound / 2^10 <= 2^(h - 10) errbound: below the bound for h < 10
    only, so the sets of height 4 (at height 16 the planted relation itself no longer passes, and must not)"""
    f, limbs, eb, elems, vals, r = _planted_run(name, h)
    with mp.workprec(fu.MP_PREC):
        noisy = to_limbs([x + (-1) ** i * mp.mpf(eb) / 1024 for i, x in enumerate(clrs_amd.mw.from_limbs(vals))], limbs)
    assert np.any(noisy != vals)
    rn = fu.host_round(noisy, f, limbs, errbound=eb)
    assert (rn.status == 0).all() and [tuple(c) for c in rn.coeffs] == elems and (rn.err < eb).all() and (rn.err > 0).all()


def test_statuses_1_2_4_and_5():
    f, limbs = fu.field("x2-5"), 4
    pi = _vals([lambda: mp.pi], limbs)
    r = fu.host_round(pi, f, limbs, errbound=1e-15, bits=40)
    assert list(r.status) == [1] and r.rung[0] == 36 and r.coeffs[0, 0] is None and not r.rel.any() and r.err[0] >= 1e-15 and r.rungs[0] == 8
    bad = np.zeros((limbs, 3))
    bad[0] = [np.nan, np.inf, -np.inf]
    r = fu.host_round(bad, f, limbs)
    assert list(r.status) == [2, 2, 2] and not r.rung.any() and not r.rel.any() and not r.vq.any()
    r = fu.host_round(pi, fu.field("3/2"), limbs, errbound=1e-15)               # 3 - 2 g = 0: a relation among the powers of g alone
    assert list(r.status) == [5] and int(r.rel[0, 0]) == 0 and [abs(int(x)) for x in r.rel[0, 1:]] == [3, 2] and r.coeffs[0, 0] is None and not r.vq.any()
    # an nd one digit too small for the planted relation: h = 40 needs two digits of 24 bits
    _, limbs, eb, elems, vals, full = _planted_run("x2-5", 40)
    assert max(abs(int(x)) for x in full.rel.flat) >= 2 ** 24
    r = fu.host_round(vals, fu.field("x2-5"), limbs, errbound=eb, nd=1)
    assert (r.status == 4).all() and not r.rel.any()
    for nd, every in ((2, False), (3, True)):                                    # the other rows of a basis at 120 bits have entries near 60 bits: three digits
        r = fu.host_round(vals, fu.field("x2-5"), limbs, errbound=eb, nd=nd)
        assert set(r.status) <= {0, 4} and (not every or (r.status == 0).all())
        assert all((r.rel[i] == full.rel[i]).all() and r.rung[i] == full.rung[i] for i in range(COUNT) if r.status[i] == 0)
    big = fu.host_round(np.array([2.0 ** 22, -2.0 ** 30]), fu.field("x2-5"), 4)
    assert list(big.status) == [4, 4] and not big.rung.any()


# ---- the incremental state ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,limbs", [("x2-5", 16, 4), ("x3-2", 16, 5), ("x4-x-1", 4, 6)])
def test_state_after_every_rung_is_unimodular_and_consistent(name, h, limbs):
    """launches of one rung: after each, for every lane still running, U is integral with |det U| = 1, c == U s_p with s_p = floor(W / 2^(P - p)), and
    W_i = floor(2^P u_i) recomputed here in mpmath; the rows are (0.98, 0.52)-reduced exactly"""
    f = fu.field(name)
    D, eb, nd = f.degree + 1, fu.planted_errbound(f.degree, h), 4
    elems, vals = fu.planted(name, h, 4, limbs=limbs)
    with mp.workprec(fu.MP_PREC):
        us = [[x] + f.power_values(prec=fu.MP_PREC) for x in clrs_amd.mw.from_limbs(vals)]
    seen = []

    def trace(ws, gw, plan):
        P, nw, hdr = plan["P"], plan["nw"], plan["hdr"]
        for i in range(ws.shape[1]):
            if ws[0, i] != -1:
                continue
            p = 1 + 5 * (int(ws[1, i]) - 1)
            Wd = [ws[hdr:hdr + nw, i]] + [gw[k] for k in range(D - 1)]
            W = [sum(int(d) << (24 * s) for s, d in enumerate(w)) for w in Wd]
            W = [w - (1 << (24 * nw)) if w >> (24 * nw - 1) else w for w in W]
            with mp.workprec(fu.MP_PREC):
                assert W == [int(mp.floor(mp.ldexp(u, P))) for u in us[i]]
            L = rounding.planes_to_ints(ws[hdr + nw:, i].reshape(nd, D, D + 1))
            U, c = L[:, :D], L[:, D]
            assert abs(lu.det_fraction(U)) == 1
            assert list(c) == [sum(int(U[r, j]) * (W[j] >> (P - p)) for j in range(D)) for r in range(D)]
            assert lu.is_lll_reduced(L)
            seen.append(p)

    fu.host_call(limbs, f.degree, f.powers(limbs), 4, vals, 4, 1000, eb, nd, launch_rungs=1, trace=trace)
    assert len(seen) > 4 * 3 and min(seen) == 1


@pytest.mark.parametrize("name,h", [("x2-2", 40), ("x4-x-1", 16)])
def test_result_does_not_depend_on_the_launch_cut(name, h):
    f, limbs, eb, elems, vals, r = _planted_run(name, h)
    mixed = np.concatenate([vals, _vals([0, lambda: mp.pi, 1], limbs), np.full((limbs, 2), 0.5)], axis=1)      # (two numbers behind count)
    runs = [fu.host_call(limbs, f.degree, f.powers(limbs), mixed.shape[1] - 2, mixed, mixed.shape[1], 1000, eb, 4, launch_rungs=n) for n in (1, 7, fu.LAUNCH_RUNGS)]
    assert fu.host_plan(1000, limbs, f.degree, 4)["launch_rungs"] == fu.LAUNCH_RUNGS
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()
    rel, status = runs[0][0], runs[0][1]
    assert (status[-2:] == fu.SENTINEL).all() and (rel[:, :, -2:] == fu.SENTINEL).all() and (status[:COUNT] == 0).all()      # nothing behind count


# ---- the binding and the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "double": C.c_double, "const double *": _lib.p_d, "double *": _lib.p_d, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    names = {"clrs_mw_field_round": ["device", "limbs", "deg", "gpow", "count", "v", "plane", "bits", "errbound", "nd", "rel", "status", "rung", "err", "vq", "info"],
             "clrs_mw_field_round_times": ["kernel_ms", "whole_ms"],
             "clrs_mw_kernel_vectors_field": ["device", "limbs", "nblk", "n", "X", "Y", "plane", "tau", "use_dual", "dual_max", "round_errbound", "deg", "gpow", "bits", "nd",
                                              "branch", "perm", "rank", "count", "V", "resid_max", "v_max", "pivot_resid", "rel", "status", "rung", "err", "Vq", "info",
                                              "round_resid_max"]}
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    for sym, want_names in names.items():
        ret, args = re.search(r"^\s*(\w+)\s+" + sym + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")] == want_names
        want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
        assert ret == "int" and _lib.SYMBOLS[sym] == (C.c_int, want)
        assert sym == "clrs_mw_kernel_vectors_field" or ":" + sym in jl or sym.endswith("_times")
    assert ":clrs_mw_field_round" in jl and "function round_to_field(" in jl
    # the shared part of the kernel-vector prototypes is the same list
    assert [n for n in names["clrs_mw_kernel_vectors_field"] if n not in ("round_errbound", "deg", "gpow", "bits", "nd", "rel", "status", "rung", "err", "Vq", "info",
                                                                         "round_resid_max")] == \
        ["device", "limbs", "nblk", "n", "X", "Y", "plane", "tau", "use_dual", "dual_max", "branch", "perm", "rank", "count", "V", "resid_max", "v_max", "pivot_resid"]
    assert any(u[1] == "clrs_mw_field_round.hip" and "-ffp-contract=off" in u[2] for u in _lib._UNITS)
    assert RoundingSettings().kernel_bits == 1000


def test_refusals_come_before_any_device_work():
    """no GPU here: a call that reached hipSetDevice would return CLRS_ERR_HIP or CLRS_ERR_NO_DEVICE, not CLRS_ERR_INVALID"""
    L = _lib.load()
    limbs, deg, n, nd = 4, 2, 3, 2
    g, v = fu.field("x2-5").powers(limbs), np.zeros((limbs, n))
    rel, status, rung, err, vq, info = fu._pools(limbs, deg, n, nd)
    pi, pd = fu._pi, fu._pd
    null_d, null_i = _lib.p_d(), _lib.p_i32()

    def call(limbs=limbs, deg=deg, g=pd(g), count=n, v=pd(v), plane=n, bits=100, eb=1e-15, nd=nd, rel=pi(rel), status=pi(status), err=pd(err), info=pi(info)):
        return L.clrs_mw_field_round(0, limbs, deg, g, count, v, plane, bits, eb, nd, rel, status, pi(rung), err, pd(vq), info)

    bad_g = g.copy()
    bad_g[0, 1] = np.inf
    for kw in (dict(limbs=3), dict(limbs=7), dict(deg=1), dict(deg=5), dict(count=-1), dict(plane=n - 1), dict(eb=0.0), dict(eb=-1.0), dict(eb=float("nan")),
               dict(bits=0), dict(nd=0), dict(nd=21), dict(g=null_d), dict(v=null_d), dict(rel=null_i), dict(status=null_i), dict(err=null_d), dict(info=null_i),
               dict(g=pd(bad_g))):
        assert call(**kw) == -1, kw
        assert b"field_round" in L.clrs_last_error()
    assert call(count=0, v=null_d, rel=null_i) == 0                              # nothing to do, nothing touched
    assert (status == fu.SENTINEL).all() and (rel == fu.SENTINEL).all() and (vq == fu.SENTINEL).all()
    a, b = C.c_double(-1), C.c_double(-1)
    assert L.clrs_mw_field_round_times(C.byref(a), C.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0
    # the kernel vectors with the rounding behind them: the refusals of clrs_mw_kernel_vectors and those of the rounding
    nblk = np.array([2], np.int32)
    XY, V4, i4, x2 = np.zeros((limbs, 4)), np.zeros((limbs, 4)), np.zeros(4, np.int32), np.zeros(2)
    rel4, info4, piv = np.zeros((nd, 3, 4), np.int32), np.zeros((2, 4), np.int32), np.zeros((limbs, 2))

    def kv(limbs=limbs, tau=1e-10, eb=1e-15, deg=2, g=pd(g), bits=100, nd=nd, rel=pi(rel4), Vq=pd(V4), plane=4):
        return L.clrs_mw_kernel_vectors_field(0, limbs, 1, pi(nblk), pd(XY), pd(XY), plane, tau, 1, 1e7, eb, deg, g, bits, nd, pi(i4), pi(i4), pi(i4), pi(i4), pd(V4), pd(x2),
                                              pd(x2), pd(piv), rel, pi(i4), pi(i4), pd(x2), Vq, pi(info4), pd(x2))

    for kw in (dict(limbs=3), dict(tau=0.0), dict(eb=0.0), dict(deg=1), dict(deg=5), dict(bits=0), dict(nd=0), dict(nd=21), dict(g=null_d), dict(rel=null_i),
               dict(Vq=null_d), dict(plane=3)):
        assert kv(**kw) == -1, kw
        assert b"kernel vectors" in L.clrs_last_error()
    assert L.clrs_mw_field_round_times(None, C.byref(b)) == -1
    assert L.clrs_config_set(b"field_round_launch_rungs", 7) == 0 and L.clrs_config_set(b"field_round_launch_rungs", 0) == 0


# ---- kernel_vectors(field=...) with host stand-ins -----------------------------------------------------------------------------------------------------------------
ROUND = fu.host_field_batch(ku.host_batch)


def test_rank_one_pair_over_q_sqrt5():
    """Y = 1 - w w^T / |w|^2 has the kernel vector w = (1/sqrt 5, (1 + sqrt 5)/4, 1); X = w w^T"""
    f, limbs = fu.field("x2-5"), 6
    with mp.workprec(fu.MP_PREC):
        w = [1 / f.g, (1 + f.g) / 4, mp.mpf(1)]
        nn = mp.fsum(x * x for x in w)
        X = to_limbs([[a * b for b in w] for a in w], limbs)
        Y = to_limbs([[(1 if i == j else 0) - a * b / nn for j, b in enumerate(w)] for i, a in enumerate(w)], limbs)
    out = rounding.kernel_vectors([3], fu.Sol(X, Y), limbs=limbs, rationalize=True, field=f, round_batch=ROUND)
    assert len(out) == 1 and out[0].count == 1 and out[0].num is None and out[0].den is None
    vec = rounding.vectors_to_field(out[0])[0]
    lead = next(i for i, x in enumerate(vec) if x != (0, 0))

    def mul(a, b):                                                               # in QQ(sqrt 5)
        return (a[0] * b[0] + 5 * a[1] * b[1], a[0] * b[1] + a[1] * b[0])

    want = [(F(0), F(1, 5)), (F(1, 4), F(1, 4)), (F(1), F(0))]
    assert all(mul(vec[i], want[lead]) == mul(want[i], vec[lead]) for i in range(3))          # proportional to w, exactly
    assert out[0].coeffs.shape == (3, 1, 2) and out[0].round_status.shape == (3, 1) and out[0].vectors_rounded.shape == (limbs, 3, 1)
    assert out[0].round_resid_max[0] < 1e-10
    with pytest.raises(NotImplementedError, match="degree above 1"):
        rounding.basis_transformations({0: (3, rounding.vectors_to_field(out[0]))}, RoundingSettings(reduce_kernelvectors=False))
    # field=None and a field of degree 1 take the path over QQ: the call of `round_batch` is today's, without `field` or `bits`
    calls = []

    def spy(*args, **kw):
        calls.append((len(args), sorted(kw)))
        raise StopIteration

    for fld in (None, NumberField([-1, 2], mp.mpf(1) / 2)):
        with pytest.raises(StopIteration):
            rounding.kernel_vectors([3], fu.Sol(X, Y), limbs=limbs, rationalize=True, field=fld, round_batch=spy)
    with pytest.raises(StopIteration):
        rounding.kernel_vectors([3], fu.Sol(X, Y), limbs=limbs, rationalize=True, field=f, round_batch=spy)
    assert calls == [(8, ["device"]), (8, ["device"]), (8, ["bits", "device", "field"])]


def _tuples(out):
    return {str(b): [[[str(x) for x in e] for e in vec] for vec in rounding.vectors_to_field(k)] for b, k in enumerate(out) if k.count}


@pytest.mark.parametrize("name", list(fu.DELSARTE))
def test_oracle_solutions_of_the_delsarte_problems_round_to_q_sqrt5(name, oracle_built):
    n, d, cos, objective, blocks, counts, height = fu.DELSARTE[name]
    f = fu.delsarte_flat(name)
    assert [int(x) for x in f.block_n] == blocks
    sol, sol64 = fu.oracle_iterate(name, 1e-60)
    field = fu.field("x2-5")
    out = rounding.kernel_vectors(f, sol, limbs=6, rationalize=True, field=field, round_batch=ROUND)
    assert {b: k.count for b, k in enumerate(out) if k.count} == counts
    worst = max(float(k.round_resid_max.max()) for k in out if k.count)
    print(name, "rungs", sorted({int(p) for k in out if k.count for p in k.round_rung.flat}), "max |Y vq| =", worst)
    assert worst < RoundingSettings().kernel_errbound
    got = _tuples(out)
    # |rel| <= height: a coefficient -a_k / a_0 in lowest terms has numerator and denominator of the primitive relation's size at most
    assert max(max(abs(c.numerator), c.denominator) for k in out if k.count for c in k.coeffs.flat) <= height
    sol40, _ = fu.oracle_iterate(name, 1e-40)
    assert _tuples(rounding.kernel_vectors(f, sol40, limbs=6, rationalize=True, field=field, round_batch=ROUND)) == got
    assert json.load(open(GOLDEN))[name]["blocks"] == got
    # The fp64 X, Y of the same solve sit 1e-16 off the field.  Three generic reals have a relation of residual about 2^(-2 p / 3) at p bits, so at
    # kernel_round_errbound = 1e-25 a spurious one appears near p = 125 whatever the number is (measured: the fp64 iterates are "rounded" at rungs 116 .. 126
    # with coefficients up to 4.8e12 when the ladder goes that far, as the reference's clindep would).  The ladder must end below that for a number off the
    # field to be refused: kernel_bits = 100, the default of the reference's roundx.
    with pytest.raises(KernelVectorError, match=rounding.CLINDEP_MESSAGE + "|" + rounding.WRONG_VECTOR_MESSAGE):
        rounding.kernel_vectors(f, sol64, limbs=6, rationalize=True, field=field, settings=RoundingSettings(kernel_round_errbound=1e-25, kernel_bits=100),
                                round_batch=ROUND)


# ---- the path through lll_batch, on the host build of clrs_zz_lll ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h", [("x2-5", 16), ("x3-2", 4), ("x5-x-1", 4)])
def test_relations_by_lll_batch_on_the_host_build(name, h):
    f = fu.field(name)
    limbs, eb = fu.planted_limbs(f.degree, h), fu.planted_errbound(f.degree, h)
    elems, vals = fu.planted(name, h, 3)
    vals = np.concatenate([vals, _vals([0, lambda: mp.pi], limbs)], axis=1)
    vals[0, -1] = np.nan
    r = rounding.field_relations_lll(vals, f, limbs, errbound=eb, bits=(f.degree + 1) * (h + 8) - 6, lll=lu.host_lll_batch)
    assert list(r.status) == [0, 0, 0, 0, 2] and (r.path == 1).all() and [tuple(c) for c in r.coeffs[:3]] == elems and r.rung[3] == 1
    assert (r.err[:4] < eb).all() and fu.vq_error(r.vq[:, :3], elems, f) <= mp.ldexp(1, -53 * limbs + limbs + 6) * 2 ** (h + 2)
    if f.degree <= 4:                                                            # the rescue: what the kernel ends with status 4 goes through lll_batch
        relations = functools.partial(rounding.field_relations_lll, lll=lu.host_lll_batch)
        stuck = rounding.round_to_field(vals[:, :3], f, limbs, errbound=eb, nd=1, relations=False, call=fu.host_call)
        back = rounding.round_to_field(vals[:, :3], f, limbs, errbound=eb, nd=1, relations=relations, call=fu.host_call)
        assert [tuple(c) for c in back.coeffs] == elems and (back.status == 0).all()
        assert all(back.path[i] == (stuck.status[i] == 4) for i in range(3)) and set(stuck.status) <= {0, 4}
    else:
        through = rounding.round_to_field(vals[:, :3], f, limbs, errbound=eb, relations=functools.partial(rounding.field_relations_lll, lll=lu.host_lll_batch))
        assert [tuple(c) for c in through.coeffs] == elems and (through.path == 1).all()

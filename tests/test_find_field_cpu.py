"""CPU side of find_field (csrc/clrs_minpoly_arith.h, clrs_amd.rounding.minimal_polynomials / select_vals / find_common_minpoly / find_field / to_field;
DESIGN.md section 27): the header compiled for the host against planted numbers and an independent restatement of the reference's min_poly -> clindep, every
status, the launch cuts, the Python layer with host stand-ins for the device calls, and the 320-bit oracle's solutions of the Delsarte problems."""
import ctypes as C
import functools
import os
import re
from fractions import Fraction as F

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd.mw import to_limbs
from clrs_amd.rounding import NumberField
from tests import field_round_util as fu
from tests import kernel_vectors_util as ku
from tests import lll_util as lu
from tests import minpoly_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4                                                     # the planted polynomials have coefficients below 2^4
BITS = mu.generic_bits(4, H)                              # 54: below the 62 bits at which five generic reals have a relation under 1e-15
RELATIONS = functools.partial(rounding.minpoly_relations_lll, lll=lu.host_lll_batch)


def _search(xs, limbs, **kw):
    kw.setdefault("relations", False)
    return rounding.minimal_polynomials(mu.planes(xs, limbs), limbs, call=mu.host_call, **kw)


# ---- planted numbers ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limbs", (4, 5, 10))
@pytest.mark.parametrize("name", list(mu.PLANTED))
def test_planted_numbers_give_their_minimal_polynomial(name, limbs):
    x, poly = mu.PLANTED[name]
    deg = len(poly) - 1
    s = _search([x], limbs, max_degree=4, bits=BITS)
    print(name, limbs, "status", s.status[0].tolist(), "rung", s.rung[0].tolist(), "relations", s.rel[0])
    assert s.degree[0] == deg and s.minpoly[0] == poly
    for d in range(1, deg):                               # nothing below its own degree: no relation, a degenerate one, or one refused for its size
        assert s.status[0, d - 1] in (1, 5) or max(abs(a) for a in s.rel[0][d - 1]) > 10 ** 5, d
    assert s.status[0, deg - 1] == 0 and (s.status[0, deg:] == -1).all() and (s.path[0, :deg] == 0).all()
    assert mu.up_to_sign(s.rel[0][deg - 1]) == poly
    # the accepted rung and relation against the restatement on the same powers, every rung from scratch
    (a, p), = mu.restated(mu.planes([x], limbs), deg, limbs, 1e-15, BITS)
    assert mu.up_to_sign(a) == mu.up_to_sign(s.rel[0][deg - 1]) == poly and p == s.rung[0, deg - 1]       # (a lattice vector and its negative are one relation)


def test_zero_and_one_close_at_degree_one():
    s = _search([0, 1, -3, mp.mpf(5) / 2], 5, bits=BITS)
    assert list(s.degree) == [1, 1, 1, 1] and s.minpoly == [[0, 1], [-1, 1], [3, 1], [-5, 2]]
    assert list(s.status[:, 0]) == [5, 0, 0, 0] and (s.status[:, 1:] == -1).all()


# ---- every status ------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_status_in_one_batch():
    limbs, deg = 5, 4
    bits = mu.generic_bits(deg, H)
    xs = [lambda: mp.pi, lambda: mp.e, mu.PLANTED["sqrt2+sqrt3"][0], 50.0, 0.0, 0.0, 0.0]
    v = mu.planes(xs, limbs)
    v[0, 4], v[0, 5], v[0, 6] = np.nan, np.inf, -np.inf
    rel, status, rung, err, info = mu.host_call(limbs, deg, 7, v, 7, bits, 1e-15, mu.ND)
    assert list(status) == [1, 1, 0, 4, 2, 2, 2]
    assert rung[0] == rung[1] == rounding.field_top_bits(bits, limbs) and err[0] >= 1e-15 and err[2] < 1e-15
    assert (rel[:, :, [0, 1, 3, 4, 5, 6]] == 0).all() and list(info[1, 3:]) == [0, 0, 0, 0]      # 50^4 > 2^22 and the non-finite end before any rung
    assert mu.relation_of((rel,), 2) == [1, 0, -10, 0, 1] or mu.relation_of((rel,), 2) == [-1, 0, 10, 0, -1]
    for d in (1, 2, 3):                                   # pi and e at every degree, the cut of each degree
        st = mu.host_call(limbs, d, 2, v, 7, mu.generic_bits(d, H), 1e-15, mu.ND)[1]
        assert list(st[:2]) == [1, 1], d
    assert mu.host_call(limbs, 3, 4, v, 7, bits, 1e-15, mu.ND)[1][3] == 5        # 50^3 < 2^22: the first row is x - 50 padded with zeros
    assert mu.host_call(limbs, 1, 4, v, 7, bits, 1e-15, mu.ND)[1][3] == 0


def test_one_digit_is_status_4_and_the_rescue_finds_it():
    """a tall rational: numerator and denominator near 2^40 do not fit one base-2^24 digit"""
    limbs, num, den = 4, 1099511627689, 1099511627791
    v = mu.planes([lambda: mp.mpf(num) / den], limbs)
    stuck = rounding.minimal_polynomials(v, limbs, max_degree=1, bits=120, errbound=2.0 ** -100, max_coeff=2 ** 41, nd=1, call=mu.host_call, relations=False)
    assert stuck.status[0, 0] == 4 and stuck.degree[0] == 0 and stuck.minpoly[0] is None
    back = rounding.minimal_polynomials(v, limbs, max_degree=1, bits=120, errbound=2.0 ** -100, max_coeff=2 ** 41, nd=1, call=mu.host_call, relations=RELATIONS)
    assert back.status[0, 0] == 0 and back.path[0, 0] == 1 and back.minpoly[0] == [-num, den]
    wide = rounding.minimal_polynomials(v, limbs, max_degree=1, bits=120, errbound=2.0 ** -100, max_coeff=2 ** 41, call=mu.host_call, relations=False)
    assert wide.status[0, 0] == 0 and wide.path[0, 0] == 0 and wide.minpoly[0] == [-num, den]
    with pytest.raises(ValueError, match="degrees"):
        rounding.minimal_polynomials(v, limbs, max_degree=5, relations=False, call=mu.host_call)


def test_sqrt2_at_degree_3_is_status_5():
    """The relations of (1, s, s^2, s^3), s = sqrt 2, are spanned by (-2, 0, 1, 0) = x^2 - 2 padded with a zero and (0, -2, 0, 1) = x (x^2 - 2), orthogonal and
    both of norm sqrt 5; their sum and difference (x^2 - 2)(1 +- x) have norm sqrt 10.  In the lattice of a rung each of the two carries a last column
    floor(2^p s^2) - 2^(p+1) or floor(2^p s^3) - 2 floor(2^p s), a number in {-1, 0, 1} the floors decide, so the two are as good as equally short and the
    first row of a reduced basis is one of them, never a true cubic: a_3 = 0 or a_0 = 0, status 5 either way.  Which of the two depends on the road the
    reduction took: the host build, which carries the basis of rung 1 on to rung 6, ends with x (x^2 - 2); the restatement, which reduces the lattice of rung 6
    from scratch, with x^2 - 2.  Both accept at p = 6, the first rung at which 2^p times the residual of any shorter row exceeds 1."""
    limbs = 5
    v = mu.planes([mu.PLANTED["sqrt2"][0]], limbs)
    rel, status, rung, err, info = mu.host_call(limbs, 3, 1, v, 1, 200, 1e-15, mu.ND)
    a = mu.relation_of((rel,), 0)
    print("sqrt 2 at degree 3:", a, "rung", rung[0])
    assert status[0] == 5 and err[0] < 1e-15 and rung[0] == 6 and mu.up_to_sign(a) == [0, -2, 0, 1]
    (b, p), = mu.restated(v, 3, limbs, 1e-15, 200)
    assert p == 6 and mu.up_to_sign(b) == [-2, 0, 1, 0]
    s = _search([mu.PLANTED["sqrt2"][0]], limbs, max_degree=3, min_degree=3, bits=200)
    assert s.degree[0] == 0 and s.minpoly[0] is None and s.rel[0][2] == a          # the host layer: nothing at this degree


# ---- launch cuts --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", (1, 2, 3, 4))
def test_result_does_not_depend_on_the_launch_cut(deg):
    limbs = 6
    vals, bits, eb = mu.mixed(deg, limbs)
    whole = mu.mixed_host(deg, limbs)
    assert {0, 1, 2, 4} <= set(int(s) for s in whole[1][:64])
    for cut in (1, 7):
        got = mu.host_call(limbs, deg, mu.TOTAL, vals, mu.TOTAL + mu.PAD, bits, eb, mu.ND, launch_rungs=cut)
        for a, b in zip(got, whole):
            assert a.tobytes() == b.tobytes()


# ---- the path through lll_batch, and the refactored field_relations_lll -----------------------------------------------------------------------------------------------
def test_minpoly_relations_lll_on_the_host_build():
    limbs = 5
    for name in ("sqrt2", "cbrt2", "sqrt2+sqrt3", "3/7"):
        x, poly = mu.PLANTED[name]
        rel, status, rung, err = rounding.minpoly_relations_lll(mu.planes([x, lambda: mp.pi], limbs), len(poly) - 1, limbs, bits=BITS, lll=lu.host_lll_batch)
        assert list(status) == [0, 1] and mu.up_to_sign(rel[0]) == poly and err[0] < 1e-15, name
    v = mu.planes([0, 50.0, 0], limbs)
    v[0, 2] = np.nan
    assert list(rounding.minpoly_relations_lll(v, 4, limbs, bits=BITS, lll=lu.host_lll_batch)[1]) == [5, 4, 2]
    x5 = fu.field("x5-x-1").g                                                   # degree 5: no kernel, all through `relations`
    s = rounding.minimal_polynomials(mu.planes([x5], limbs), limbs, max_degree=5, bits=BITS, call=mu.host_call, relations=RELATIONS)
    assert s.degree[0] == 5 and s.minpoly[0] == [-1, -1, 0, 0, 0, 1] and s.path[0, 4] == 1 and (s.path[0, :4] == 0).all()


@pytest.mark.parametrize("name,h", [("x2-5", 16), ("x3-2", 4)])
def test_field_relations_lll_is_what_it_was(name, h):
    """the inputs of tests/test_field_round_cpu.test_relations_by_lll_batch_on_the_host_build after the rung loop moved into a helper"""
    f = fu.field(name)
    limbs, eb = fu.planted_limbs(f.degree, h), fu.planted_errbound(f.degree, h)
    elems, vals = fu.planted(name, h, 3)
    vals = np.concatenate([vals, mu.planes([0, lambda: mp.pi], limbs)], axis=1)
    vals[0, -1] = np.nan
    r = rounding.field_relations_lll(vals, f, limbs, errbound=eb, bits=(f.degree + 1) * (h + 8) - 6, lll=lu.host_lll_batch)
    assert list(r.status) == [0, 0, 0, 0, 2] and (r.path == 1).all() and [tuple(c) for c in r.coeffs[:3]] == elems and r.rung[3] == 1
    assert r.coeffs[4, 0] is None and tuple(r.coeffs[3]) == (F(0),) * f.degree and (r.err[:4] < eb).all()
    no_field = rounding.field_relations_lll(mu.planes([mp.sqrt(7)], 5), fu.field("3/2"), 5, lll=lu.host_lll_batch)
    assert list(no_field.status) == [5] and no_field.coeffs[0, 0] is None


# ---- find_common_minpoly, to_field -------------------------------------------------------------------------------------------------------------------------------
def _common(xs, limbs=5, **kw):
    s = _search(xs, limbs, max_degree=4, bits=BITS)
    v = mu.planes(xs, limbs)
    gens = [(v[:, i], int(s.degree[i]), s.minpoly[i]) for i in range(len(xs))]
    return rounding.find_common_minpoly(gens, limbs, bits=BITS, call=mu.host_call, relations=False, round_call=fu.host_call, round_relations=False, **kw), v


def _embed(coeffs, field):
    with mp.workprec(mu.MP_PREC):
        return mp.fsum(mp.mpf(c.numerator) / c.denominator * field.g ** k for k, c in enumerate(coeffs))


def test_common_field_of_generators_of_one_quadratic_field():
    with mp.workprec(mu.MP_PREC):
        xs = [mp.sqrt(5), (1 + mp.sqrt(5)) / 2, 3 * mp.sqrt(5) - 2]
    field, v = _common(xs)
    assert field.degree == 2 and field.minpoly == [-1, -1, 1] and field.prec == 64 * 5 + 128        # the largest degree, the smallest sum |coeffs|
    back = rounding.to_field(v, field, limbs=5, bits=BITS, call=fu.host_call, relations=False)
    assert back == [(F(-1), F(2)), (F(0), F(1)), (F(-5), F(6))]
    assert rounding.find_common_minpoly([], 5).minpoly == [-1, 1]


def test_two_quadratic_fields_extend_to_their_compositum():
    with mp.workprec(mu.MP_PREC):
        xs = [mp.sqrt(2), mp.sqrt(3)]
        field, v = _common(xs)
        assert field.degree == 4 and field.minpoly == [1, 0, -10, 0, 1] and abs(field.g - (xs[0] + xs[1])) < mp.ldexp(1, -400)
        back = rounding.to_field(v, field, limbs=5, bits=BITS, call=fu.host_call, relations=False)
        for x, c in zip(xs, back):
            assert abs(_embed(c, field) - x) < mp.mpf(10) ** -30
    assert back[0] == (F(0), F(-9, 2), F(0), F(1, 2)) and back[1] == (F(0), F(11, 2), F(0), F(-1, 2))


def test_a_common_field_above_max_degree_is_refused():
    with mp.workprec(mu.MP_PREC):
        xs = [mp.sqrt(2), mp.cbrt(2)]
    with pytest.raises(ArithmeticError, match="find_field: the common field has degree above max_degree"):
        _common(xs)


def test_to_field_refuses_a_number_outside_the_field():
    with pytest.raises(ValueError, match=rounding.CLINDEP_MESSAGE):
        rounding.to_field(mu.planes([mp.sqrt(5), lambda: mp.pi], 5), fu.field("x2-5"), limbs=5, bits=mu.generic_bits(2, H), call=fu.host_call, relations=False)


# ---- find_field on the oracle's solutions ----------------------------------------------------------------------------------------------------------------------------
HOOKS = dict(batch=ku.host_batch, call=mu.host_call, relations=RELATIONS, round_call=fu.host_call, round_relations=False)
ROUND = fu.host_field_batch(ku.host_batch)


@pytest.mark.parametrize("name", list(fu.DELSARTE))
def test_find_field_on_the_oracles_solutions_over_q_sqrt5(name, oracle_built):
    f = fu.delsarte_flat(name)
    sol, _ = fu.oracle_iterate(name, 1e-60)
    values, origins = rounding.select_vals(f, sol, limbs=6, batch=ku.host_batch)
    print(name, len(origins), "selected values, blocks", sorted({o[0] for o in origins}))
    assert values.shape == (6, len(origins)) and len(origins) >= 1 and (np.abs(values[0]) > 1e-15).all()
    found = rounding.find_field(f, sol, limbs=6, **HOOKS)
    print(name, "minpoly", found.minpoly, "g", mp.nstr(found.g, 20))
    assert found.degree == 2
    with mp.workprec(mu.MP_PREC):
        c, = rounding.to_field([mp.sqrt(5)], found, limbs=6, call=fu.host_call, relations=False)
        assert abs(_embed(c, found) - mp.sqrt(5)) < 1e-10
    out = rounding.kernel_vectors(f, sol, limbs=6, rationalize=True, field=found, round_batch=ROUND)
    assert {b: k.count for b, k in enumerate(out) if k.count} == fu.DELSARTE[name][5]


def test_find_field_on_a_rational_solution_has_degree_one(oracle_built):
    from oracle.oracle import Oracle
    from clrs_amd import problems
    f = clrs_amd.flatten(problems.delsarte_exact(8, 3, 0.5))
    r = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=1e-60)
    assert r["error_code"] == 0 and abs(r["p_obj"] - 240) <= 1e-9
    r2 = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=1e-60, snapshots=[r["iterations"]], snapshot_limbs=6)
    sol = fu.Sol(r2["snap"]["X"][0], r2["snap"]["Y"][0])
    found = rounding.find_field(f, sol, limbs=6, **HOOKS)
    assert found.degree == 1 and found.minpoly == [-1, 1] and found.g == 1


# ---- the binding and the refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "double": C.c_double, "const double *": _lib.p_d, "double *": _lib.p_d, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    names = {"clrs_mw_minpoly": ["device", "limbs", "deg", "count", "v", "plane", "bits", "errbound", "nd", "rel", "status", "rung", "err", "info"],
             "clrs_mw_minpoly_times": ["kernel_ms", "whole_ms"]}
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    for sym, want_names in names.items():
        ret, args = re.search(r"^\s*(\w+)\s+" + sym + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")] == want_names
        want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
        assert ret == "int" and _lib.SYMBOLS[sym] == (C.c_int, want)
    assert ":clrs_mw_minpoly," in jl and "function minpoly(" in jl
    assert any(u[1] == "clrs_minpoly.hip" and "-ffp-contract=off" in u[2] for u in _lib._UNITS)
    mw_units = [u for u in _lib._UNITS if u[0].startswith("clrs_mw")]
    assert mw_units and not any(u[3]("clrs_minpoly.hip") or u[3]("clrs_minpoly_arith.h") for u in mw_units)      # an edit rebuilds its own unit only
    for name in ("MinPolySearch", "minimal_polynomials", "minpoly_relations_lll", "select_vals", "find_common_minpoly", "find_field", "to_field"):
        assert name in rounding.__all__ and hasattr(rounding, name)


def test_refusals_come_before_any_device_work():
    """no GPU here: a call that reached hipSetDevice would return CLRS_ERR_HIP or CLRS_ERR_NO_DEVICE, not CLRS_ERR_INVALID"""
    L = _lib.load()
    limbs, deg, n, nd = 4, 2, 3, 2
    v = np.zeros((limbs, n))
    rel, status, rung, err, info = mu._pools(deg, n, nd)
    pi, pd = mu._pi, mu._pd
    null_d, null_i = _lib.p_d(), _lib.p_i32()

    def call(limbs=limbs, deg=deg, count=n, v=pd(v), plane=n, bits=100, eb=1e-15, nd=nd, rel=pi(rel), status=pi(status), err=pd(err), info=pi(info)):
        return L.clrs_mw_minpoly(0, limbs, deg, count, v, plane, bits, eb, nd, rel, status, pi(rung), err, info)

    for kw in (dict(limbs=3), dict(limbs=7), dict(deg=0), dict(deg=5), dict(count=-1), dict(count=n + 1), dict(plane=n - 1), dict(eb=0.0), dict(eb=-1.0),
               dict(eb=float("nan")), dict(bits=0), dict(nd=0), dict(nd=rounding.LLL_MAX_DIGITS + 1), dict(v=null_d), dict(rel=null_i), dict(status=null_i),
               dict(err=null_d), dict(info=null_i)):
        assert call(**kw) == -1, kw
        assert b"minpoly" in L.clrs_last_error()
    assert call(count=0, v=null_d, rel=null_i) == 0                              # nothing to do, nothing touched
    assert (status == mu.SENTINEL).all() and (rel == mu.SENTINEL).all()
    a, b = C.c_double(-1), C.c_double(-1)
    assert L.clrs_mw_minpoly_times(C.byref(a), C.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0
    assert L.clrs_mw_minpoly_times(None, C.byref(b)) == -1

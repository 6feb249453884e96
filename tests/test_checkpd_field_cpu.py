"""CPU side of the exact positive-definiteness check over a number field (rounding.checkpd_field, split_primes, field_minor_bounds, clrs_modp_minors_field,
clrs_modp_field_frobenius): the arithmetic header through its g++ build against Python integers, the host layer through the
`minors=` stand-in (tests/pd_field_util.py) against Bareiss' minors in Z[g] and their signs in mpmath with `==`, the coefficient bound, the prime scan against
root counts by trial, the binding and the refusals of the C functions, which happen before any device call."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import mpmath as mp
import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import pd_field_util as fu
from tests import pd_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pi, _pd = fu._pi, fu._pd
PRIMES = (pu.PMAX, 8388587, 10007, 7, 3, 2)
POLYS = {2: ([-5, 0, 1], [-5, 0, 2], [1, 1, 1]), 3: ([-2, 0, 0, 1], [3, -1, 4, 7]), 4: ([-1, -1, 0, 0, 1], [6, 0, -5, 0, 1], [2, 3, 5, 7, 11])}


# ---- the arithmetic header ----------------------------------------------------------------------------------------------------------------------------------------
def polymulmod(a, b, f, p):
    """a b mod (f, p) on Python integers: the plain product, then the top term cleared with f, downwards"""
    d, inv = len(f) - 1, pow(f[-1], -1, p)
    t = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            t[i + j] += x * y
    for k in range(len(t) - 1, d - 1, -1):
        c = t[k] * inv
        for j in range(d + 1):
            t[k - d + j] -= c * f[j]
    return [v % p for v in (t + [0] * d)[:d]]


def test_digit_horner_of_the_residue_kernel():
    L, top = fu.host_lib(), 1 << 23
    rng = np.random.default_rng(1)
    for p in PRIMES:
        for digits in ([top], [-top], [top] * 5, [-top] * 5, [0, 0, top], [top - 1, -top + 1, 12345, -top], [int(v) for v in rng.integers(-top, top + 1, size=70)]):
            d = np.array(digits, np.int32)
            want = sum(int(v) << (24 * l) for l, v in enumerate(digits)) % p
            assert L.ff_digits_host(p, d.size, _pi(d)) == float(want), (p, digits[:4])


@pytest.mark.parametrize("deg", (2, 3, 4))
def test_residue_by_horner(deg):
    L = fu.host_lib()
    rng = np.random.default_rng(deg)
    for p in PRIMES:
        c = rng.integers(0, p, size=(40, deg)).astype(np.float64)
        r = rng.integers(0, p, size=40).astype(np.float64)
        c[0], r[0] = p - 1, p - 1                                     # the extremes: every product (p - 1)^2
        c[1], r[1] = p - 1, 0
        c[2], r[2] = 0, p - 1
        out = np.full(40, -1.0)
        assert L.ff_residue_host(deg, p, 40, _pd(np.ascontiguousarray(c)), _pd(r), _pd(out)) == 0
        want = [sum(int(c[i, j]) * pow(int(r[i]), j, p) for j in range(deg)) % p for i in range(40)]
        assert out.tolist() == [float(v) for v in want]
    assert L.ff_residue_host(5, 7, 0, None, None, None) == -1 and L.ff_residue_host(1, 7, 0, None, None, None) == -1


@pytest.mark.parametrize("deg", (2, 3, 4))
def test_fold_table_product_step_and_frobenius(deg):
    L = fu.host_lib()
    rng = np.random.default_rng(10 + deg)
    cases = [(f, p) for f in POLYS[deg] for p in PRIMES if f[-1] % p]
    cases += [([p - 1] * (deg + 1), p) for p in PRIMES[:3]]            # every coefficient at its largest
    for f, p in cases:
        fm = [c % p for c in f]
        for trial in range(4):
            a, b = [int(v) for v in rng.integers(0, p, size=deg)], [int(v) for v in rng.integers(0, p, size=deg)]
            if trial == 0:
                a, b = [p - 1] * deg, [p - 1] * deg
            bit = trial & 1
            table, prod, step, frob = np.full((deg - 1) * deg, -1.0), np.full(deg, -1.0), np.full(deg, -1.0), np.full(deg, -1.0)
            arr = lambda v: np.array(v, np.float64)
            assert L.ff_field_host(deg, p, _pd(arr(fm)), _pd(arr(a)), _pd(arr(b)), bit, _pd(table), _pd(prod), _pd(step), _pd(frob)) == 0
            x = [0, 1] + [0] * (deg - 2)
            xpow, want_table = polymulmod([1], [1], fm, p), []
            for k in range(2 * deg - 1):
                if k >= deg:
                    want_table += xpow
                xpow = polymulmod(xpow, x, fm, p)
            assert table.tolist() == [float(v) for v in want_table], (f, p)
            assert prod.tolist() == [float(v) for v in polymulmod(a, b, fm, p)], (f, p)
            sq = polymulmod(a, a, fm, p)
            assert step.tolist() == [float(v) for v in (polymulmod(sq, x, fm, p) if bit else sq)], (f, p)
            assert frob.tolist() == [float(v) for v in fu.host_frobenius(f, p)], (f, p)
    assert L.ff_field_host(2, 5, _pd(np.array([1.0, 0.0, 0.0])), None, None, 0, None, None, None, None) == -2      # the leading coefficient is 0 mod p


def test_host_frobenius_formulations_agree_and_detect_splitting():
    for polys in POLYS.values():
        for f in polys:
            for p in (2, 3, 5, 7, 11, 13, 101, 10007, pu.PMAX):
                assert rounding._frobenius_host(f, p) == fu.host_frobenius(f, p)
                d = len(f) - 1
                if f[-1] % p:
                    splits = len(fu.roots_by_trial(f, p)) == d if p < 200 else None
                    if splits is not None:
                        disc_ok = len(rounding._pmod_gcd(f, [j * c for j, c in enumerate(f)][1:], p)) == 1
                        assert (fu.host_frobenius(f, p) == [0, 1] + [0] * (d - 2) and disc_ok) == splits, (f, p)


def test_the_batched_host_frobenius_is_the_scalar_one():
    primes = [int(p) for p in rounding._primes_descending()[:60]] + [2, 3, 5, 7, 11, 10007]
    for name in fu.FIELDS:
        f = fu.field(name).minpoly
        assert fu.host_frobenius_many(f, primes).tolist() == [fu.host_frobenius(f, p) for p in primes]


# ---- split_primes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fu.FIELDS)
def test_split_primes_against_root_counts_by_trial(name):
    fld = fu.field(name)
    f, d = fld.minpoly, fld.degree
    small = [int(p) for p in rounding._primes_descending() if p < 1500]
    want = [(p, fu.roots_by_trial(f, p)) for p in small if f[-1] % p]
    want = [(p, r) for p, r in want if len(r) == d]
    assert len(want) >= 3
    primes, roots = rounding.split_primes(fld, len(want), start=1500)
    assert list(zip(primes, roots)) == want
    assert rounding.split_primes(f, 2, start=want[1][0]) == ([w[0] for w in want[2:4]], [w[1] for w in want[2:4]])   # strictly below `start`; a coefficient list
    with pytest.raises(ArithmeticError):
        rounding.split_primes(fld, len(want) + 1, start=1500)        # the primes run out
    top, top_roots = rounding.split_primes(fld, 2)
    assert top[0] > top[1] > (1 << 22) and all(sum(c * pow(r, j, p) for j, c in enumerate(f)) % p == 0 for p, rr in zip(top, top_roots) for r in rr)
    assert all(len(set(rr)) == d and rr == sorted(rr) for rr in top_roots)


def test_split_primes_takes_a_batch_test():
    """`frobenius=`: the scan in batches, here the host Frobenius behind the interface of the device function"""
    seen = []

    def batch(minpoly, primes):
        seen.append(len(primes))
        return np.array([fu.host_frobenius(minpoly, int(p)) for p in primes], np.int32)
    fld = fu.field("x3-2")
    assert rounding.split_primes(fld, 3, start=3000, frobenius=batch) == rounding.split_primes(fld, 3, start=3000) and seen and max(seen) <= 4096
    with pytest.raises(ValueError):
        rounding.split_primes([1, 1], 1)


# ---- checkpd_field through the stand-ins -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fu.PLANTED)
def test_planted_matrices(name):
    fld, A, pd, order = fu.planted(name)
    scale, minors, exact_pd, exact_order = fu.planted_exact(name)
    assert exact_pd == pd and (order is None or exact_order == order)
    assert all(fu.sign_at(fld, A[i][i]) > 0 for i in range(len(A)))   # nothing here is decided by the diagonal
    cert, calls = fu.planted_host_certificate(name)
    assert cert.scale == scale and cert.pd == pd == bool(cert) and cert.failed_order == exact_order and cert.minors == minors and len(calls) >= 1
    assert all(isinstance(v, int) for m in cert.minors for v in m)
    h, lc = cert.minpoly, cert.generator_scale
    assert h[-1] == 1 and lc == abs(fld.minpoly[-1]) and [c * lc ** j for j, c in enumerate(h)] == [c * lc ** (fld.degree - 1) * (1 if fld.minpoly[-1] > 0 else -1) for c in fld.minpoly]
    want_primes, want_roots = rounding.split_primes(fld, len(cert.primes))
    assert cert.primes == want_primes and cert.roots == [[r * lc % p for r in rr] for p, rr in zip(want_primes, want_roots)]
    assert all(sum(c * pow(r, j, p) for j, c in enumerate(h)) % p == 0 for p, rr in zip(cert.primes, cert.roots) for r in rr)
    lo, hi = cert.interval
    with mp.workprec(fu.MP_PREC):
        assert isinstance(lo, F) and isinstance(hi, F) and mp.mpf(lo.numerator) / lo.denominator < fld.g < mp.mpf(hi.numerator) / hi.denominator
    for p, r, k in cert.discarded:                                   # a discarded pair: the image of that minor at the pair is zero, and of none before it
        assert p in cert.primes and r in cert.roots[cert.primes.index(p)]
        images = [sum(c * pow(r, j, p) for j, c in enumerate(m)) % p for m in minors[:k]]
        assert images[-1] == 0 and all(images[:-1])
    if name == "one pair breaks down at 5 of 8":
        p, roots = fu.first_split_prime("x2-5")
        assert cert.discarded == [(p, roots[0], 5)] and cert.primes[0] == p and len(cert.minors) == 8
    if name in ("zero minor 17 of 33", "singular psd gram"):
        assert cert.minors[-1] == [0] * fld.degree and len(cert.discarded) == fld.degree * len(cert.primes)          # every pair breaks down, the zero is proven


def test_one_matrix_two_embeddings_opposite_answers():
    (f1, A1, _, _), (f2, A2, _, _) = fu.planted("g-2 at 5 of 8"), fu.planted("g-2 at 5 of 8, negative root")
    with mp.workprec(fu.MP_PREC):
        assert A1 == A2 and f1.minpoly == f2.minpoly and f1.g + f2.g == 0 and f1.g > 2
    a, b = fu.planted_host_certificate("g-2 at 5 of 8")[0], fu.planted_host_certificate("g-2 at 5 of 8, negative root")[0]
    assert a.pd and not b.pd and b.failed_order == 5 and a.minors[:5] == b.minors and a.interval[0] > 0 > b.interval[1]


def test_the_tiny_minor_needs_refinement():
    fld, A, _, _ = fu.planted("(g-2)^20 at 5 of 8")
    cert = fu.planted_host_certificate("(g-2)^20 at 5 of 8")[0]
    with mp.workprec(fu.MP_PREC):
        v = fu.value(fld, tuple(F(c) for c in cert.minors[4]))
        assert 0 < v < mp.mpf(10) ** -12 and max(abs(c) for c in cert.minors[4]) > 10 ** 12
    assert cert.pd and cert.interval[1] - cert.interval[0] < F(1, 1 << 64)       # fp64 cannot see this sign: c_0 + c_1 sqrt 5 cancels to 1e-13 of its terms


@pytest.mark.parametrize("name", fu.PLANTED)
def test_bound_holds_for_every_exact_coefficient(name):
    fld, A, _, _ = fu.planted(name)
    scale, lc, M = fu.normal_form(fld, A)
    d, n = fld.degree, len(A)
    coeff = [[[fu.to_h_coordinates(lc, M[i][j])[c] for j in range(n)] for i in range(n)] for c in range(d)]
    bounds = rounding.field_minor_bounds(coeff, fld)
    minors = [fu.to_h_coordinates(lc, m) for m in fu.bareiss_minors_field(fld.minpoly, M)]       # (up to the first zero minor: beyond it Bareiss has no pivot)
    assert len(bounds) == n and all(isinstance(b, int) for b in bounds)
    assert all(abs(c) <= bounds[k] for k, m in enumerate(minors) for c in m)


@pytest.mark.parametrize("name", [n for n in fu.PLANTED if n not in ("zero minor 17 of 33", "singular psd gram")])       # (those two have the eigenvalue 0)
def test_decisions_against_the_smallest_eigenvalue(name):
    fld, A, _, _ = fu.planted(name)
    with mp.workprec(400):
        E = mp.matrix([[fu.value(fld, e) for e in row] for row in A])
        lam = min(mp.eigsy(E, eigvals_only=True))
        assert abs(lam) > mp.ldexp(1, -200)                           # well separated: the eigenvalues of entries near 2^10 are good to about 2^-380 here
        assert fu.planted_host_certificate(name)[0].pd == (lam > 0)


def test_breakdowns_that_leave_too_few_primes_draw_more():
    """both pairs of the first split prime break down at order 2, so order 3 needs a further call"""
    fld = fu.field("x2-5")
    p, _ = fu.first_split_prime("x2-5")
    e = lambda v: (F(v), F(0))
    A = [[e(1), e(0), e(0)], [e(0), e(p), e(0)], [e(0), e(0), e(1)]]
    fu.host_field_minors.calls.clear()
    cert = rounding.checkpd_field(A, fld, minors=fu.host_field_minors)
    assert cert.pd and cert.minors == [[1, 0], [p, 0], [p, 0]] and len(fu.host_field_minors.calls) == 2 and len(cert.primes) >= 2
    assert sorted(cert.discarded) == sorted((p, r, 2) for r in cert.roots[0])


def test_small_and_degenerate_inputs():
    fld = fu.field("x2-5")
    calls = fu.host_field_minors.calls
    c = rounding.checkpd_field([], fld, minors=fu.host_field_minors)
    assert c.pd and c.minors == [] and c.failed_order is None and c.scale == 1 and c.primes == [] and c.interval[0] < c.interval[1]
    calls.clear()
    c = rounding.checkpd_field([[(F(1, 2), 0), (0, 0)], [(0, 0), (2, -1)]], fld, minors=fu.host_field_minors)        # 2 - sqrt 5 < 0: the host answers
    assert not c.pd and c.failed_order == 2 and c.minors == [] and c.scale == 2 and calls == []
    assert not rounding.checkpd_field([[(0, 0)]], fld, minors=fu.host_field_minors).pd and calls == []
    c = rounding.checkpd_field([[(-2, 1)]], fld, minors=fu.host_field_minors)
    assert c.pd and c.minors == [[-2, 1]] and c.scale == 1
    assert not rounding.checkpd_field([[(-2, 1)]], fu.field("x2-5 negative root"), minors=fu.host_field_minors).pd
    c = rounding.checkpd_field([[(F(1, 3), 0), (0, F(1, 2))], [(0, F(1, 2)), (1, 0)]], fld, minors=fu.host_field_minors)   # det = 1/3 - 5/4 < 0
    assert not c.pd and c.failed_order == 2 and c.scale == 6 and c.minors == [[2, 0], [12 - 45, 0]]
    half = fu.field("2x2-5")                                         # g^2 = 5/2: [[1, g], [g, 3]] has determinant 1/2; in h = 2 g, scaled by 2: [[2, h], [h, 6]]
    c = rounding.checkpd_field([[(1, 0), (0, 1)], [(0, 1), (3, 0)]], half, minors=fu.host_field_minors)
    assert c.pd and c.scale == 2 and c.generator_scale == 2 and c.minpoly == [-10, 0, 1] and c.minors == [[2, 0], [2, 0]]
    c = rounding.checkpd_field([[(1, 0), (0, 1)], [(0, 1), (2, 0)]], half, minors=fu.host_field_minors)      # determinant 2 - 5/2 < 0
    assert not c.pd and c.minors == [[2, 0], [-2, 0]]


def test_refused_inputs():
    fld = fu.field("x2-5")
    one, g = (1, 0), (0, 1)
    for bad in ([[one, g], [one, one]], [[one, g, g], [g, one, g]], [[(1, 0, 0)]], [[1]], 5):
        with pytest.raises(ValueError):
            rounding.checkpd_field(bad, fld, minors=fu.host_field_minors)
    big = [[(int(i == j), 0) for j in range(129)] for i in range(129)]
    with pytest.raises(ValueError, match="128"):
        rounding.checkpd_field(big, fld, minors=fu.host_field_minors)
    with pytest.raises(ValueError):
        rounding.field_minor_bounds([[[1]]], fld)
    with pytest.raises(ValueError):
        rounding.field_minor_bounds([[[1, 2], [3, 4]], [[0, 0], [0, 0]]], fld)
    with pytest.raises(ValueError):
        rounding.is_valid_solution([[[one]]], [[1]], [1], [1], field=fld, minors=fu.host_field_minors)           # the slack check over a field is not built


def test_a_reducible_polynomial_is_reported_not_guessed():
    """(x^2 - 2)(x^2 - 3) at sqrt 2: the element 2 - g^2 has non-zero coefficients and the value zero.  No precision decides its sign; the cap does"""
    with mp.workprec(fu.MP_PREC):
        fld = rounding.NumberField([6, 0, -5, 0, 1], mp.sqrt(2))
    z = (0, 0, 0, 0)
    with pytest.raises(ArithmeticError, match="order 2"):
        rounding.checkpd_field([[(2, 0, 0, 0), (0, 1, 0, 0)], [(0, 1, 0, 0), (1, 0, 0, 0)]], fld, minors=fu.host_field_minors)
    with pytest.raises(ArithmeticError, match="diagonal entry 2"):
        rounding.checkpd_field([[(1, 0, 0, 0), z], [z, (-2, 0, 1, 0)]], fld, minors=fu.host_field_minors)
    with mp.workprec(fu.MP_PREC):
        with pytest.raises(ArithmeticError, match="reducible"):
            rounding.checkpd_field([[(-2, 1)]], rounding.NumberField([-4, 0, 1], mp.mpf(2)), minors=fu.host_field_minors)      # g - 2 at the root 2 of x^2 - 4


def test_is_valid_solution_over_a_field_and_unchanged_without_one():
    fld, good, _, _ = fu.planted("gram x2-5")
    bad = fu.planted("negative minor 9 of 20")[1]
    kw = dict(check_slacks=False, field=fld, minors=fu.host_field_minors)
    assert rounding.is_valid_solution([good, good], **kw) == (True, [])
    assert rounding.is_valid_solution([good, bad, [[(-1, 0)]]], **kw) == (False, [("block", 1, 9), ("block", 2, 1)])
    # field=None: the inputs of tests/test_checkpd_cpu.py::test_is_valid_solution, the same answers with and without the keyword
    ok, nok = [[2, 1], [1, 2]], [[1, 2], [2, 1]]
    A, x, b = [[1, F(1, 2), 0], [0, 1, 1]], [F(1, 3), 2, -1], [F(4, 3), 1]
    for extra in ({}, {"field": None}, {"field": None, "primes": None}):
        assert rounding.is_valid_solution([ok, pu.hilbert(5)], A, b, x, minors=pu.host_minors, **extra) == (True, [])
        got = rounding.is_valid_solution([ok, nok, ok, [[-1]]], A, [F(4, 3), 2], x, minors=pu.host_minors, **extra)
        assert got == (False, [("constraint", 1, F(-1)), ("block", 1, 2), ("block", 3, 1)])
        assert rounding.is_valid_solution([ok], check_slacks=False, minors=pu.host_minors, **extra) == (True, [])
        assert rounding.is_valid_solution([], A, b, x, minors=pu.host_minors, **extra) == (True, [])
        with pytest.raises(ValueError):
            rounding.is_valid_solution([ok], minors=pu.host_minors, **extra)


# ---- the binding and the refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32, "double *": _lib.p_d, "const int64_t *": _lib.p_i64}
    names = {"clrs_modp_minors_field": ["device", "n", "deg", "nd", "digits", "nprimes", "primes", "roots", "minors", "breakdown", "info"],
             "clrs_modp_minors_field_times": ["residues_ms", "ldl_ms", "total_ms"],
             "clrs_modp_field_frobenius": ["device", "deg", "minpoly", "nprimes", "primes", "out"]}
    L = _lib.load()
    for fn, want in names.items():
        ret, args = re.search(r"^\s*(\w+)\s+%s\s*\(([^;{]*?)\)\s*;" % fn, hdr, flags=re.M).groups()
        args = [" ".join(a.split()) for a in args.split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == want
        assert ret == "int" and _lib.SYMBOLS[fn] == (C.c_int, [table[re.sub(r"\w+$", "", a).strip()] for a in args]) and hasattr(L, fn)
    for name in ("split_primes", "field_frobenius", "leading_minors_field_mod", "field_minor_bounds", "FieldPDCertificate", "checkpd_field"):
        assert name in rounding.__all__ and hasattr(rounding, name)
    assert rounding.FIELD_MINORS_DEGREES == (2, 3, 4)


def test_refusals_need_no_device():
    """what the two C functions refuse, they refuse before they touch a device, and they write nothing"""
    L = _lib.load()
    D = np.array([[[[2, 1], [1, 3]], [[0, -1], [-1, 0]]], [[[1, 0], [0, 1]], [[0, 2], [2, 0]]]], np.int32)          # deg = 2, nd = 2, n = 2
    P = np.array([pu.PMAX, 10007, 2], np.int32)
    R = np.array([[5, 9], [0, 10006], [0, 1]], np.int32)
    minors, brk, info = np.full((3, 2, 2), fu.SENTINEL, np.int32), np.full((3, 2), fu.SENTINEL, np.int32), np.full(4, fu.SENTINEL, np.int32)

    def call(n=2, deg=2, nd=2, D=D, nprimes=3, P=P, R=R, minors=minors, brk=brk, info=info):
        return L.clrs_modp_minors_field(0, n, deg, nd, _pi(D), nprimes, _pi(P), _pi(R), _pi(minors), _pi(brk), _pi(info))
    assert call(deg=1) == -1 and call(deg=0) == -1 and call(deg=5) == -1 and b"deg" in L.clrs_last_error()
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=129) == -1 and b"128" in L.clrs_last_error()
    assert call(nd=0) == -1 and call(nd=32768) == -1 and call(nprimes=0) == -1 and call(nprimes=65536) == -1
    for name in ("D", "P", "R", "minors", "brk", "info"):
        assert call(**{name: None}) == -1 and b"null" in L.clrs_last_error()
    for v in ((1 << 23) + 1, -(1 << 23) - 1):
        bad = D.copy()
        bad[1, 1, 0, 0] = v
        assert call(D=bad) == -1 and b"digit" in L.clrs_last_error()
    bad = D.copy()
    bad[1, 0, 0, 1] = 5                                               # the second coefficient's first plane
    assert call(D=bad) == -1 and b"symmetric" in L.clrs_last_error()
    for p in (1, 0, -7, 4, 10005, 1 << 23, (1 << 23) + 9):
        assert call(P=np.array([pu.PMAX, p, 2], np.int32)) == -1 and b"prime" in L.clrs_last_error()
    assert call(P=np.array([10007, 2, 10007], np.int32)) == -1 and b"repeated" in L.clrs_last_error()
    for q, v in ((0, -1), (0, pu.PMAX), (1, 10007), (2, 2)):
        bad = R.copy()
        bad[q, 1] = v
        assert call(R=bad) == -1 and b"root" in L.clrs_last_error()
    bad = R.copy()
    bad[1, 1] = 0
    assert call(R=bad) == -1 and b"equal roots" in L.clrs_last_error()
    assert all(int(v) == fu.SENTINEL for a in (minors, brk, info) for v in a.flat)
    assert L.clrs_modp_minors_field_times(None, None, None) == -1

    out = np.full((3, 2), fu.SENTINEL, np.int32)
    f = np.array([-5, 0, 1], np.int64)

    def frob(deg=2, f=f, nprimes=3, P=P, out=out):
        return L.clrs_modp_field_frobenius(0, deg, None if f is None else f.ctypes.data_as(_lib.p_i64), nprimes, _pi(P), _pi(out))
    assert frob(deg=1) == -1 and frob(deg=5) == -1 and frob(nprimes=0) == -1 and frob(nprimes=(1 << 20) + 1) == -1
    assert frob(f=None) == -1 and frob(P=None) == -1 and frob(out=None) == -1 and b"null" in L.clrs_last_error()
    assert frob(f=np.array([1, 1, 0], np.int64)) == -1 and b"leading" in L.clrs_last_error()
    for p in (1, 0, -7, 4, 10005, 1 << 23):
        assert frob(P=np.array([pu.PMAX, p, 2], np.int32)) == -1 and b"prime" in L.clrs_last_error()
    assert all(int(v) == fu.SENTINEL for v in out.flat)

    sym = [[[2, 1], [1, 3]], [[0, 1], [1, 0]]]
    for args in ((sym[:1], [7], [[1]]), ([[[1, 2], [3, 4]], sym[1]], [7], [[1, 2]]), (sym, [], []), (sym, [1 << 23], [[1, 2]]), (sym, [7], [[1, 7]]), (sym, [7], [[1]]),
                 ([np.eye(129, dtype=np.int64)] * 2, [7], [[1, 2]]), (sym * 3, [7], [[1, 2, 3, 4, 5, 6]])):
        with pytest.raises(ValueError):
            rounding.leading_minors_field_mod(*args)
    for args in (([1, 1], [7]), ([1, 0, 0, 0, 0, 1], [7]), ([1, 0, 1], []), ([1, 0, 1], [1 << 23]), ([1, 0, 1 << 63], [7])):
        with pytest.raises(ValueError):
            rounding.field_frobenius(*args)


def test_no_cpu_fallback_without_a_device():
    """without a device the calls raise; with one they compute (this test never skips)"""
    import torch
    sym = [[[2, 1], [1, 2]], [[0, 0], [0, 0]]]
    if torch.cuda.is_available():
        m, b = rounding.leading_minors_field_mod(sym, [7], [[1, 2]])
        assert m.tolist() == [[[2, 3], [2, 3]]] and b.tolist() == [[0, 0]]
        assert rounding.field_frobenius([-5, 0, 1], [11, 7]).tolist() == [[0, 1], [0, 6]]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.leading_minors_field_mod(sym, [7], [[1, 2]])
        with pytest.raises(_lib.ClrsError):
            rounding.field_frobenius([-5, 0, 1], [11, 7])
        with pytest.raises(_lib.ClrsError):
            rounding.checkpd_field([[(2, 0)]], fu.field("x2-5"))

"""CPU tests of the exact integer matrix product (clrs_zz_gemm): the arithmetic of csrc/clrs_modp_zz_arith.h compiled for the host, a whole
host product built from it the way the kernels are, the linear digit conversions, the `matmul=` hooks of the four front ends of clrs_amd.rounding, the binding,
and the refusals of the C function, which happen before any device call.  Every comparison is `==`; the oracle is Python integer arithmetic."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import zz_util as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF, BASE = zu.HALF, zu.BASE


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------------------------
def test_flush_period_of_the_kernel_is_within_the_bound():
    most, taken, steps, bits = zu.host_constants()
    assert (most, bits) == (31, 24) and 1 <= taken <= most and steps * 4 == taken
    # the bound itself: a remainder of 2^23 plus 4 F products of 2^46 stays below 2^53 iff F <= 31
    assert HALF + 4 * 31 * 2 ** 46 < 2 ** 53 <= HALF + 4 * 32 * 2 ** 46
    csrc = os.path.join(ROOT, "clusteredlowranksolver.jl_amd", "csrc")
    src, tile = open(os.path.join(csrc, "clrs_modp_zz_gemm.hip.h")).read(), open(os.path.join(csrc, "clrs_modp_tile.hip.h")).read()
    assert re.search(r"^#define ZZ_BK 16\b", tile, flags=re.M) and "ZZ_FLUSH_MFMAS / (ZZ_BK / 4)" in src and "static_assert(ZZ_FLUSH_STEPS" in src
    assert "zz_tile_loop<ZZ_FLUSH_STEPS>" in src                    # the period the kernel hands to the shared loop is the one asserted


def test_split_at_the_ends_at_ties_and_at_zero():
    values = [0, 2 ** 53 - 1, -(2 ** 53 - 1), 1, -1, HALF, -HALF, HALF - 1, HALF + 1, -HALF - 1]
    for c in (0, 1, 2, 3, -1, -2, 12345, -12346, 2 ** 28, 2 ** 28 + 1, -(2 ** 28) - 1):
        values += [c * BASE + HALF, c * BASE - HALF, c * BASE, c * BASE + HALF - 1, c * BASE - HALF + 1]
    lo, c, bad = zu.host_split(values)
    for v, l, q, b in zip(values, lo, c, bad):
        assert b == 0 and l == int(l) and q == int(q)
        assert int(q) * BASE + int(l) == v and abs(int(l)) <= HALF, v
        if abs(v % BASE - HALF) != 0:                               # away from a tie the remainder is the balanced digit
            assert int(l) == ((v + HALF) % BASE) - HALF, v
    # ties go to the even multiple: 2^23 = 0 * 2^24 + 2^23, 3 * 2^23 = 2 * 2^24 - 2^23
    lo, c, _ = zu.host_split([HALF, 3 * HALF, -HALF, -3 * HALF])
    assert [int(v) for v in c] == [0, 2, 0, -2] and [int(v) for v in lo] == [HALF, -HALF, -HALF, HALF]
    # what is no flushed accumulator is seen: a fraction, a value of 2^53 and beyond, a NaN
    _, _, bad = zu.host_split([0.5, float(2 ** 77), float("nan")])
    assert bad[0] == 1 and bad[2] == 1
    assert zu.host_flush_cycle([0] * 4, [0] * 4, rem=0.0, hi0=float(2 ** 53))[0] == 1


@pytest.mark.parametrize("nmfma", [1, 7, 28, 31])
def test_flush_cycle_of_extreme_products_is_exact(nmfma):
    rng = np.random.default_rng(nmfma)
    count = 4 * nmfma
    operands = {
        "all-positive-max-1": (np.full(count, HALF - 1), np.full(count, HALF - 1)),
        "all-negative-products": (np.full(count, HALF - 1), np.full(count, 1 - HALF)),
        "random-signs": ((HALF - 1) * rng.choice([-1, 1], size=count), (HALF - 1) * rng.choice([-1, 1], size=count)),
        "all-2^23": (np.full(count, HALF), np.full(count, HALF)),
        "all-minus-2^23": (np.full(count, -HALF), np.full(count, HALF)),
        "mix": (np.where(rng.integers(0, 2, size=count) == 0, HALF, HALF - 1) * rng.choice([-1, 1], size=count),
                np.where(rng.integers(0, 2, size=count) == 0, -HALF, HALF - 1)),
    }
    for name, (a, b) in operands.items():
        for rem in (0, HALF, -HALF, HALF - 1):
            exact = rem + sum(int(x) * int(y) for x, y in zip(a, b))
            assert abs(exact) < 2 ** 53
            bad, acc, lo, hi = zu.host_flush_cycle(a, b, rem=rem, hi0=5.0)
            assert bad == 0 and acc == exact and int(acc) == exact, (name, rem)
            assert int(lo) + (int(hi) - 5) * BASE == exact and abs(int(lo)) <= HALF, (name, rem)


def test_flush_cycle_past_the_bound_is_what_the_bound_forbids():
    """without a flush: 32 MFMAs of products (2^23 - 1)^2, a little below 2^46, still sum below 2^53 and exactly; 40 of them do not, and fp64 then loses the
    sum -- the reason for the period"""
    a, b = np.full(4 * 32, HALF - 1), np.full(4 * 32, HALF - 1)
    exact = (HALF - 1) + sum(int(x) * int(y) for x, y in zip(a, b))
    _, acc, _, _ = zu.host_flush_cycle(a, b, rem=HALF - 1)
    assert exact < 2 ** 53                                          # (products of 2^23 - 1 are a little below 2^46: still inside)
    assert int(acc) == exact
    a, b = np.full(4 * 40, HALF - 1), np.full(4 * 40, HALF - 1)
    exact = 1 + sum(int(x) * int(y) for x, y in zip(a, b))
    _, acc, _, _ = zu.host_flush_cycle(a, b, rem=1)
    assert exact > 2 ** 53 and int(acc) != exact


def test_carry_walk():
    rng = np.random.default_rng(3)
    ns = 5
    S = rng.integers(-2 ** 60, 2 ** 60, size=(64, ns))
    S[0] = 0
    S[1] = [-1, 0, 0, 0, 0]
    S[2] = [HALF, HALF, HALF, HALF, HALF - 1]                     # digits at the upper end: each 2^23 becomes -2^23 and a carry
    S[3] = [-HALF, -HALF, -HALF, -HALF, -HALF]                     # the lower end stays as it is
    S[4] = [HALF - 1, HALF - 1, HALF - 1, HALF - 1, HALF - 1]
    S[5] = [-HALF - 1, 0, 0, 0, 0]
    S[6] = [2 ** 61, -2 ** 61, 2 ** 61, -2 ** 61, 2 ** 61]
    values = [sum(int(v) << (24 * s) for s, v in enumerate(row)) for row in S]
    need = [rounding.to_balanced_digits(np.array([v], dtype=object)).shape[0] for v in values]
    for ndc in (1, 2, ns, ns + 1, ns + 2, ns + 3, ns + 6):
        digits, over = zu.host_carry(S, ndc)
        assert over == sum(1 for c in need if c > ndc)
        for row, v, c in zip(digits, values, need):
            if c <= ndc:                                            # sign extension included: the planes above are what the carry leaves
                assert row.tolist() == rounding.to_balanced_digits(np.array([v], dtype=object), count=ndc)[:, 0].tolist()
            else:                                                   # (the low digits were still walked: they are the low digits of the value)
                assert all(-HALF <= int(d) < HALF for d in row)
    assert max(need) <= ns + 3


# ---- a whole host product, built the way the kernels are --------------------------------------------------------------------------------------------------------
def _check_host_product(name, Ad, Bd, dcs=(None,)):
    exact = zu.exact_product(Ad, Bd)
    ndc = zu.digits_needed(exact)
    want = zu.expected_planes(exact, ndc)
    for dc in dcs:
        code, Cd, info = zu.host_gemm(Ad, Bd, ndc, dc=dc)
        assert code == 0 and info[0] == 0 and info[3] == 0, name
        assert info[1] == (1 if dc is None else -(-Bd.shape[0] // dc))
        assert np.array_equal(Cd, want), name


def test_host_product_on_the_tile_edge_shapes():
    for name, Ad, Bd in zu.shape_cases():
        _check_host_product(name, Ad, Bd)


@pytest.mark.parametrize("name,Ad,Bd", zu.k_cases(), ids=[c[0] for c in zu.k_cases()])
def test_host_product_across_the_flush_boundary(name, Ad, Bd):
    _check_host_product(name, Ad[:, :5], Bd[:, :, :5])


def test_host_product_digit_counts_ranges_and_the_check_shape():
    for name, Ad, Bd in zu.digit_cases():
        _check_host_product(name, Ad, Bd, dcs=(None, 1, 2))
    name, Ad, Bd = zu.vector_case()
    _check_host_product(name, Ad, Bd, dcs=(None, 7))


def test_host_product_refuses_too_few_digits_and_extends_signs():
    Ad, Bd = zu.random_digits(1, 2, 6, 9), zu.random_digits(2, 2, 9, 4)
    exact = zu.exact_product(Ad, Bd)
    assert any(v < 0 for v in exact.flat)
    ndc = zu.digits_needed(exact)
    code, Cd, info = zu.host_gemm(Ad, Bd, ndc + 3)
    assert code == 0 and np.array_equal(Cd, zu.expected_planes(exact, ndc + 3))
    too_long = sum(1 for v in exact.flat if rounding.to_balanced_digits(np.array([v], dtype=object)).shape[0] > ndc - 1)
    code, Cd, info = zu.host_gemm(Ad, Bd, ndc - 1)
    assert code == -1 and info[0] == too_long > 0 and (Cd == zu.SENTINEL).all()


def test_sanitizer_program_ends_clean():
    """the stand-alone program over zz_host.cpp, built with -fsanitize=address,undefined, run as a process of its own"""
    r = subprocess.run([zu.sanitizer_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "zz_host: ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)


# ---- the digit conversions -------------------------------------------------------------------------------------------------------------------------------------
def _boundary_values():
    out = [0, 1, -1, HALF, -HALF, HALF - 1, 1 - HALF, HALF + 1, -HALF - 1]
    out += [s << (24 * c - 1) for c in (1, 2, 3) for s in (1, -1)]   # +-2^(24 c - 1): one digit more on the positive side than on the negative
    for l in (1, 2, 3, 10, 100, 417):
        for base in (1 << (24 * l), (1 << (24 * l)) // 2, zu.rounding._balanced_offset(l), (1 << (24 * l)) - 1 - zu.rounding._balanced_offset(l)):
            out += [s * (base + d) for s in (1, -1) for d in (-1, 0, 1)]
    return out


TO_PLANES = (rounding.ints_to_planes, rounding.to_balanced_digits)
FROM_PLANES = (rounding.planes_to_ints, rounding.from_balanced_digits)


def test_ints_to_planes_and_back_against_the_oracles():
    """both names of either direction against tests/zz_util.py's plain restatement of the definition (which shares no code with them)"""
    rng = np.random.default_rng(11)
    values = _boundary_values()
    for bits in (1, 23, 24, 25, 47, 48, 62, 63, 64, 65, 1000, 5000, 24 * 300, 100000):
        for _ in range(3):
            v = int.from_bytes(rng.bytes((bits + 7) // 8), "little") >> ((-bits) % 8)
            values += [v, -v]
    assert any(abs(v).bit_length() == 5000 for v in values)
    for v in values:                                                # one by one: the count of each
        a = np.array([v], dtype=object)
        for to_planes, from_planes in zip(TO_PLANES, FROM_PLANES):
            planes = to_planes(a)
            if abs(v).bit_length() <= 24 * 300:
                want = zu.digits_restated(a)
                assert planes.dtype == want.dtype and planes.shape == want.shape and np.array_equal(planes, want), v
                assert zu.values_of(planes)[0] == v
            else:                                                   # (the restatement is quadratic: at 10^5 bits only the properties)
                assert planes.dtype == np.int32 and planes.min() >= -HALF and planes.max() < HALF and planes[-1, 0] != 0
            assert from_planes(planes)[0] == v and type(from_planes(planes)[0]) is int
            assert rounding._balanced_need(v) == planes.shape[0]
    assert zu.digits_restated([HALF - 1]).tolist() == [[HALF - 1]] and zu.digits_restated([HALF]).shape[0] == 2 and zu.digits_restated([-HALF]).shape[0] == 1
    short = [v for v in values if abs(v).bit_length() <= 24 * 100]
    mixed = np.array(short + [0] * (-len(short) % 4), dtype=object).reshape(4, -1)        # together: one count for all, shapes kept
    small = np.array([[1, -2 ** 40], [HALF, -HALF]], dtype=np.int64)
    loose = np.array([[[HALF, -HALF]], [[HALF, 5]]], np.int32)      # digits that include 2^23 (what clrs_zz_gemm accepts as input) still give the value
    for to_planes, from_planes in zip(TO_PLANES, FROM_PLANES):
        planes = to_planes(mixed)
        assert planes.shape[1:] == mixed.shape and np.array_equal(planes, zu.digits_restated(mixed))
        assert np.array_equal(to_planes(mixed, count=planes.shape[0] + 5), zu.digits_restated(mixed, count=planes.shape[0] + 5))
        back = from_planes(planes)
        assert back.shape == mixed.shape and back.dtype == object and all(type(v) is int for v in back.flat) and (back == mixed).all()
        assert np.array_equal(to_planes(small), zu.digits_restated(small))
        assert np.array_equal(to_planes([[3, 4]], count=3), zu.digits_restated([[3, 4]], count=3))
        empty = to_planes(np.zeros((0, 3), np.int64))
        assert empty.shape == (1, 0, 3) and empty.dtype == np.int32 and to_planes(np.zeros((0, 3), np.int64), count=4).shape == (4, 0, 3)
        assert (from_planes(loose) == zu.values_of(loose)).all() and from_planes(loose).tolist() == [[HALF + HALF * BASE, -HALF + 5 * BASE]]


def test_ints_to_planes_refuses_a_count_too_small():
    for v in (HALF, -HALF - 1, 1 << 24 * 5, -(1 << 24 * 5), 10 ** 400):
        need = rounding._balanced_need(v)
        assert rounding.ints_to_planes(np.array([v], dtype=object), count=need).shape[0] == need
        with pytest.raises(ValueError):
            rounding.ints_to_planes(np.array([v], dtype=object), count=need - 1)
        with pytest.raises(ValueError):
            rounding.ints_to_planes(np.array([0, v], dtype=object), count=need - 1)
    with pytest.raises(ValueError):
        rounding.ints_to_planes(np.array([10 ** 400], dtype=object), count=0)
    with pytest.raises(ValueError):
        rounding.ints_to_planes(np.array([0.5]))
    with pytest.raises(ValueError):
        rounding.planes_to_ints(np.zeros((0, 3), np.int32))
    # every name speaks for itself
    for name in ("ints_to_planes", "to_balanced_digits"):
        for a in (np.array([HALF]), np.array([10 ** 400], dtype=object)):
            with pytest.raises(ValueError, match=f"^{name}: a value does not fit in 1 balanced digits of 24 bits$"):
                getattr(rounding, name)(a, count=1)
        with pytest.raises(ValueError, match=f"^{name}: the values must be integers, got dtype float64$"):
            getattr(rounding, name)(np.array([0.5]))


# ---- the matmul= hooks -------------------------------------------------------------------------------------------------------------------------------------------
P = du.PMAX


def _fractions_of(A, den):
    """an integer matrix made rational: entry (i, j) divided by den[(i + j) % len(den)]"""
    return [[Fraction(int(v), den[(i + j) % len(den)]) for j, v in enumerate(row)] for i, row in enumerate(np.asarray(A, dtype=object))]


def _systems():
    """(name, A, b): a square integer system, a square rational one, a wide, a tall and a rank-deficient one"""
    rng = np.random.default_rng(7)
    A, b = du.random_system(1, 6, 20, P)
    wide = rng.integers(-9, 10, size=(4, 7))
    tall = rng.integers(-9, 10, size=(7, 4))
    x0 = [Fraction(int(v), 3) for v in rng.integers(-5, 6, size=4)]
    deficient = rng.integers(-5, 6, size=(5, 6))
    deficient[4] = deficient[0] + 2 * deficient[1]
    x1 = [Fraction(int(v), 7) for v in rng.integers(-5, 6, size=6)]
    return [
        ("square", A, b),
        ("rational", _fractions_of(A, (1, 2, 3, 5)), [Fraction(int(v), 7) for v in b]),
        ("wide", _fractions_of(wide, (1, 2)), [Fraction(int(v), 3) for v in rng.integers(-9, 10, size=4)]),
        ("tall", tall.astype(object), du.matvec(tall.astype(object), x0)),
        ("deficient", deficient.astype(object), du.matvec(deficient.astype(object), x1)),
    ]


def test_solve_dixon_with_a_matmul_stand_in():
    for name, A, b in _systems()[:2]:
        ref = rounding.solve_dixon(A, b, lift=du.lift)
        for reconstruct in (None, _host_reconstruct):
            mm = zu.CountingMatmul()
            got = rounding.solve_dixon(A, b, lift=du.lift, reconstruct=reconstruct, matmul=mm)
            assert list(got) == list(ref) and (got.p, got.steps) == (ref.p, ref.steps)
            assert mm.calls == [((6, 6), (6,)), ((6, 6), (6,))], name          # Ai x of the lifted integers, then Ai y == L bi
            assert rounding.solve_dixon(A, b, lift=du.lift, reconstruct=reconstruct, matmul=zu.CountingMatmul(), check=False) == list(ref)
        for call in (0, 1):                                           # either check sees one corrupted entry
            with pytest.raises(ArithmeticError):
                rounding.solve_dixon(A, b, lift=du.lift, matmul=zu.CountingMatmul(corrupt=call))
        none = zu.CountingMatmul()
        rounding.solve_dixon(A, b, lift=du.lift, matmul=none, check=False)
        assert none.calls == []


def _host_reconstruct(X, p, N, D, device=0, want_x=False):
    x = du.horner(np.asarray(X), p)
    sol = [du.reconstruct(v, p ** np.asarray(X).shape[0], N, D) for v in x]
    return (sol, x) if want_x else sol


def test_solve_system_pseudoinverse_with_a_matmul_stand_in():
    for name, A, b in _systems():
        if name == "deficient":
            with pytest.raises(rounding.SingularSystemError):
                rounding.solve_system_pseudoinverse(A, b, lift=du.lift, matmul=zu.CountingMatmul())
            continue
        ref = rounding.solve_system_pseudoinverse(A, b, lift=du.lift)
        mm = zu.CountingMatmul()
        got = rounding.solve_system_pseudoinverse(A, b, lift=du.lift, matmul=mm)
        assert got == ref and all(type(v) is Fraction for v in got), name
        nrows, ncols = np.asarray(A, dtype=object).shape
        k = min(nrows, ncols)
        if ncols > nrows:                                           # Gram, the two checks of the solve, the back-substitution
            assert mm.calls == [((nrows, ncols), (ncols, nrows)), ((k, k), (k,)), ((k, k), (k,)), ((ncols, nrows), (nrows,))], name
        else:                                                       # Gram, A^T b, the two checks
            assert mm.calls == [((ncols, nrows), (nrows, ncols)), ((ncols, nrows), (nrows,)), ((k, k), (k,)), ((k, k), (k,))], name
        with pytest.raises(ArithmeticError):
            rounding.solve_system_pseudoinverse(A, b, lift=du.lift, matmul=zu.CountingMatmul(corrupt=len(mm.calls) - 2 if ncols > nrows else 2))


from tests import modp_util as mu

_batch = mu.host_batch


def test_project_to_affine_space_with_a_matmul_stand_in():
    for name, A, b in _systems():
        for settings in (rounding.RoundingSettings(), rounding.RoundingSettings(pseudo=False)):
            ref = rounding.project_to_affine_space(A, b, settings=settings, lift=du.lift, batch=_batch)
            mm = zu.CountingMatmul()
            got = rounding.project_to_affine_space(A, b, settings=settings, lift=du.lift, batch=_batch, matmul=mm)
            assert got == ref and ref[2], (name, settings.pseudo)
            nrows, ncols = np.asarray(A, dtype=object).shape
            shapes = [c[0] + c[1] for c in mm.calls]
            if not settings.pseudo and name == "tall":              # the normal equations: M^T M, M^T c, the two checks of the solve, their test
                assert mm.calls == [((4, 7), (7, 4)), ((4, 7), (7,)), ((4, 4), (4,)), ((4, 4), (4,)), ((4, 4), (4,))]
            elif not settings.pseudo and name == "deficient":       # 4 pivots in 5 rows: the same five products
                assert mm.calls == [((4, 5), (5, 4)), ((4, 5), (5,)), ((4, 4), (4,)), ((4, 4), (4,)), ((4, 4), (4,))]
            elif not settings.pseudo:
                assert len(mm.calls) == 2 and ref[1] is True        # a square pivot system: only the checks of the solve
            else:
                assert mm.calls[-1] == ((nrows, ncols), (ncols,)), (name, shapes)         # residual_free on the whole system, last
                assert len(mm.calls) >= 4
    # a corrupted residual test is seen as wrong slacks, nothing else changes
    name, A, b = _systems()[2]
    ref = rounding.project_to_affine_space(A, b, lift=du.lift, batch=_batch)
    count = zu.CountingMatmul()
    rounding.project_to_affine_space(A, b, lift=du.lift, batch=_batch, matmul=count)
    got = rounding.project_to_affine_space(A, b, lift=du.lift, batch=_batch, matmul=zu.CountingMatmul(corrupt=len(count.calls) - 1))
    assert ref[1] is True and got == (ref[0], False, True)


def test_is_valid_solution_with_a_matmul_stand_in():
    for name, A, b in _systems():
        x, ok, _ = rounding.project_to_affine_space(A, b, lift=du.lift, batch=_batch)
        assert ok
        nrows, ncols = np.asarray(A, dtype=object).shape
        mm = zu.CountingMatmul()
        assert rounding.is_valid_solution([], A, b, x, matmul=mm) == rounding.is_valid_solution([], A, b, x) == (True, [])
        assert mm.calls == [((nrows, ncols), (ncols,))]
        wrong = list(x)
        wrong[1] += Fraction(3, 11)
        ref = rounding.is_valid_solution([], A, b, wrong)
        got = rounding.is_valid_solution([], A, b, wrong, matmul=zu.CountingMatmul())
        assert got == ref and not ref[0] and all(type(f[2]) is Fraction for f in got[1]), name
        assert not rounding.is_valid_solution([], A, b, x, matmul=zu.CountingMatmul(corrupt=0))[0]
    assert rounding.is_valid_solution([], [[1, 2]], [3], [1, 1], check_slacks=False, matmul=zu.CountingMatmul()) == (True, [])


def test_zz_matmul_refuses_what_is_no_integer_matrix():
    with pytest.raises(ValueError):
        rounding.zz_matmul([[1, 2]], [[1, 2]])
    with pytest.raises(ValueError):
        rounding.zz_matmul([[0.5]], [[1]])
    with pytest.raises(ValueError):
        rounding.zz_matmul([[Fraction(1, 2)]], [[1]])
    out = rounding.zz_matmul(np.zeros((3, 0), np.int64), np.zeros((0, 2), np.int64))      # an empty inner extent: zeros, no device
    assert out.shape == (3, 2) and out.dtype == object and not out.any()
    assert rounding.zz_matmul(np.zeros((0, 4), np.int64), np.zeros(4, np.int64)).shape == (0,)


# ---- the binding and the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbol_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32, "double *": _lib.p_d}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_zz_gemm\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "m", "k", "n", "nda", "A", "ndb", "B", "ndc", "C", "info"]
    assert ret == "int" and _lib.SYMBOLS["clrs_zz_gemm"] == (C.c_int, [table[re.sub(r"\w+$", "", a).strip()] for a in args])
    ret, args = re.search(r"^\s*(\w+)\s+clrs_zz_gemm_times\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    assert ret == "int" and [re.search(r"(\w+)$", a).group(1) for a in args.split(",")] == ["gemm_ms", "combine_ms", "whole_ms"]
    assert _lib.SYMBOLS["clrs_zz_gemm_times"] == (C.c_int, [_lib.p_d] * 3)
    L = _lib.load()
    assert hasattr(L, "clrs_zz_gemm") and hasattr(L, "clrs_zz_gemm_times")
    for name in ("ints_to_planes", "planes_to_ints", "zz_matmul"):
        assert name in rounding.__all__ and hasattr(rounding, name)
    import inspect
    for fn in (rounding.solve_dixon, rounding.solve_system_pseudoinverse, rounding.project_to_affine_space, rounding.is_valid_solution):
        assert inspect.signature(fn).parameters["matmul"].default is None


def test_refusals_need_no_device():
    """what clrs_zz_gemm refuses, it refuses before it touches a device, and it writes nothing"""
    L = _lib.load()
    A, B = np.ones((2, 3, 4), np.int32), np.ones((2, 4, 5), np.int32)
    Cd, info = np.full((4, 3, 5), zu.SENTINEL, np.int32), np.full(4, zu.SENTINEL, np.int32)
    pi = zu._pi

    def call(m=3, k=4, n=5, nda=2, A=A, ndb=2, B=B, ndc=4, Cd=Cd, info=info):
        return L.clrs_zz_gemm(0, m, k, n, nda, pi(A), ndb, pi(B), ndc, pi(Cd), pi(info))
    assert call(m=-1) == -1 and call(k=-1) == -1 and call(n=-1) == -1 and b"negative" in L.clrs_last_error()
    for name in ("nda", "ndb", "ndc"):
        assert call(**{name: 0}) == -1 and call(**{name: 32768}) == -1 and call(**{name: -3}) == -1 and b"32767" in L.clrs_last_error()
    # 2^31 elements or more: the pointers are never followed
    assert call(m=1 << 16, k=1 << 14, nda=2) == -1 and b"2^31" in L.clrs_last_error()
    assert call(k=1 << 16, n=1 << 14, ndb=2) == -1 and b"2^31" in L.clrs_last_error()
    assert call(m=1 << 16, n=1 << 14, k=1, ndc=2, nda=1, ndb=1) == -1 and b"2^31" in L.clrs_last_error()
    assert call(m=0, n=0, k=1 << 30, nda=1, ndb=7) == -1 and b"2^30" in L.clrs_last_error()
    assert call(m=0, n=0, k=1 << 16, nda=1 << 14, ndb=1 << 14) == -1 and b"2^30" in L.clrs_last_error()
    for name in ("A", "B", "Cd", "info"):
        assert call(**{name: None}) == -1 and b"null" in L.clrs_last_error()
    for v in (HALF + 1, -HALF - 1):
        for which in ("A", "B"):
            bad = (A if which == "A" else B).copy()
            bad[1, 2, 3] = v
            assert call(**{which: bad}) == -1 and b"digit" in L.clrs_last_error()
    assert (Cd == zu.SENTINEL).all() and (info == zu.SENTINEL).all()
    # an empty product gives zeros (or nothing) without a device; null pointers of empty operands are accepted
    assert call(k=0, A=None, B=None) == 0 and not Cd.any() and info.tolist() == [0, 0, 0, 0]
    assert call(m=0, A=None, Cd=None) == 0 and call(n=0, B=None, Cd=None) == 0
    assert L.clrs_zz_gemm_times(None, None, None) == -1
    assert zu.device_times() == [0.0, 0.0, 0.0]
    assert L.clrs_config_set(b"zz_gemm_chunk_bytes", 4096) == 0 and L.clrs_config_set(b"zz_gemm_chunk_bytes", 0) == 0


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    if torch.cuda.is_available():
        assert rounding.zz_matmul([[1, 2], [3, 4]], [5, 6]).tolist() == [17, 39]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.zz_matmul([[1, 2], [3, 4]], [5, 6])

"""CPU side of the exact solve by Dixon's p-adic lifting (clrs_modp_dixon_lift, clrs_amd.rounding): the digit helpers, the limb
arithmetic of csrc/clrs_modp_lift_arith.h compiled for the host against Python integers, the bound and the reconstruction on hand examples, the Python layer
with the restatement of tests/dixon_util.py as a stand-in for the device call (the package has no CPU implementation of it), the binding and the refusals."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import modp_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMES = (2, 3, 10007, 8388593)


# ---- digits -----------------------------------------------------------------------------------------------------------------------------------------------
def test_digit_helpers_round_trip():
    planes = rounding.to_balanced_digits(du.BOUNDARY)
    assert planes.dtype == np.int32 and planes.shape == (6, len(du.BOUNDARY))              # 10^40 < 2^133 needs six digits of 24 bits
    assert planes.min() >= -2 ** 23 and planes.max() < 2 ** 23
    assert [int(v) for v in rounding.from_balanced_digits(planes)] == du.BOUNDARY
    for j, v in enumerate(du.BOUNDARY):
        assert planes[:, j].tolist() == du.balanced(v, 6)
    # the digits of the boundary values themselves
    assert rounding.to_balanced_digits([2 ** 23 - 1]).tolist() == [[2 ** 23 - 1]]
    assert rounding.to_balanced_digits([2 ** 23]).tolist() == [[-2 ** 23], [1]]
    assert rounding.to_balanced_digits([-2 ** 23]).tolist() == [[-2 ** 23]]
    assert rounding.to_balanced_digits([-2 ** 23 - 1]).tolist() == [[2 ** 23 - 1], [-1]]
    assert rounding.to_balanced_digits([-2 ** 47 - 2 ** 23]).tolist() == [[-2 ** 23], [-2 ** 23]]
    assert rounding.to_balanced_digits([0]).tolist() == [[0]]
    # a count, a matrix, numpy integers and Python integers alike
    M = np.array([[1, -2 ** 40], [2 ** 23, 7]], dtype=np.int64)
    for a in (M, M.astype(object)):
        d = rounding.to_balanced_digits(a, count=4)
        assert d.shape == (4, 2, 2) and [[int(v) for v in row] for row in rounding.from_balanced_digits(d)] == M.tolist()
    with pytest.raises(ValueError):
        rounding.to_balanced_digits([2 ** 23], count=1)
    with pytest.raises(ValueError):
        rounding.to_balanced_digits([0.5])


def test_extreme_matrix_has_the_digits_the_gpu_test_relies_on():
    """both digits of an off-diagonal entry of the extreme matrix are -2^23, the digit of largest magnitude; the diagonal's low digit is -2^23 + 3"""
    A, b = du.extreme_system(5)
    d = rounding.to_balanced_digits(A)
    assert d.shape == (2, 5, 5) and d[:, 0, 1].tolist() == [-2 ** 23, -2 ** 23] and d[:, 2, 2].tolist() == [-2 ** 23 + 3, -2 ** 23]


# ---- the host build of clrs_modp_lift_arith.h ----------------------------------------------------------------------------------------------------------------
def test_host_digit_split_and_carry():
    rng = np.random.default_rng(1)
    vals = [0, 1, -1, 2 ** 23 - 1, 2 ** 23, -2 ** 23, -2 ** 23 - 1, 2 ** 47 + 2 ** 23, -(2 ** 47 + 2 ** 23), 2 ** 61, -2 ** 61, 2 ** 61 + 2 ** 38, -2 ** 61 - 2 ** 38]
    vals += [int(v) for v in rng.integers(-2 ** 61, 2 ** 61, size=10 ** 4)]
    digits, carry = du.host_split(vals, 3)
    for v, d, c in zip(vals, digits, carry):
        assert all(-2 ** 23 <= int(t) < 2 ** 23 for t in d)
        assert du.value(d) + (c << 72) == v                       # the digits and the carry out make the value
    digits, carry = du.host_split(vals, 4)
    assert all(c == 0 for c in carry) and [du.value(d) for d in digits] == vals
    assert [d.tolist() for d in digits[:9]] == [du.balanced(v, 4) for v in vals[:9]]


@pytest.mark.parametrize("p", PRIMES)
def test_host_division_by_p(p):
    """random multiples of p of both signs in 1 to 6 limbs: the quotient limbs sum to the quotient, the remainder is 0, and after lift_renorm they are the
    balanced digits of the quotient; then numbers that are no multiples: floor division, remainder in [0, p)"""
    rng = np.random.default_rng(p)
    for nl in range(1, 7):
        top = (2 ** 23 - 1) * sum(2 ** (24 * l) for l in range(nl))  # every digit 2^23 - 1: every |value| <= top fits in nl balanced limbs
        qs = [0, 1, -1, top // p, -(top // p)] + [int(rng.integers(0, 2 ** 62)) % (top // p + 1) * (1 if i % 2 else -1) for i in range(400)]
        for mult in (True, False):
            vals = [q * p for q in qs] if mult else [max(-top, min(top, q * p + int(rng.integers(0, p)))) for q in qs]
            limbs = np.array([du.balanced(v, nl) for v in vals], dtype=np.int32)
            quot, rem = du.host_div(p, limbs)
            assert [int(r) for r in rem] == [v % p for v in vals]
            assert [du.value(q) for q in quot] == [v // p for v in vals]
            assert all(-2 ** 22 <= int(t) <= 2 ** 24 for t in quot.flat)
            norm, carry = du.host_renorm(quot)
            assert all(c == 0 for c in carry)
            assert [row.tolist() for row in norm] == [du.balanced(v // p, nl) for v in vals]


@pytest.mark.parametrize("p", PRIMES)
def test_host_residue_of_a_limb_vector(p):
    rng = np.random.default_rng(p + 7)
    for nl in (1, 2, 5, 6):
        limbs = rng.integers(-2 ** 23, 2 ** 23, size=(500, nl)).astype(np.int32)
        limbs[0], limbs[1] = -2 ** 23, 2 ** 23 - 1
        assert du.host_residue(p, limbs) == [du.value(row) % p for row in limbs]
    pw = np.zeros(8, np.int32)
    assert du.host_lib().lift_power_table_host(p, 8, pw.ctypes.data_as(_lib.p_i32)) == 0
    assert pw.tolist() == [pow(2, 24 * l, p) for l in range(8)]


def test_host_renorm_reports_a_carry_out():
    norm, carry = du.host_renorm(np.array([[2 ** 24, 2 ** 23 - 1]], dtype=np.int32))      # 2^24 + (2^23 - 1) 2^24 = 2^47: one limb too many
    assert carry == [1] and norm.tolist() == [[0, -2 ** 23]]


@pytest.mark.parametrize("case", ("one digit", "three digits", "extreme", "boundaries", "p=2"))
def test_host_build_of_the_lifting_step(case):
    """a whole lifting with the pieces the kernels are made of (lift_carry per limb, lift_finish_row per row; plain loops for the wave sums) equals the
    restatement digit for digit, with both counters zero"""
    A, b, p = {"one digit": lambda: (*du.random_system(41, 9, 20, 10007), 10007),
               "three digits": lambda: (*du.random_system(42, 7, 71, du.PMAX, bbits=133), du.PMAX),
               "extreme": lambda: (*du.extreme_system(65), du.PMAX),
               "boundaries": lambda: (*du.boundary_system(10007), 10007),
               "p=2": lambda: (*du.random_system(43, 17, None, 2, lo_entries=8), 2)}[case]()
    K = du.steps_and_bounds(A, b, p)[0]
    X, r, cnt = du.host_lift(A, b, p, K)
    want_X, want_r, _ = du.lift(A, b, p, K)
    assert cnt == [0, 0] and np.array_equal(X, want_X) and r == want_r


def test_host_finish_row_counts_a_remainder():
    L = du.host_lib()
    L.lift_step_host.argtypes = [C.c_int] * 4 + [_lib.p_i32] * 6
    pi = lambda a: a.ctypes.data_as(_lib.p_i32)
    # n = 1, A = (3), C = (1) is no inverse of 3 mod 7: r - A x = 5 - 3 * 5 = -10 is no multiple of 7
    Cm, Ad, r, rbar, x, cnt = (np.array(v, np.int32) for v in ([1], [3], [5, 0, 0, 0], [5], [0], [0, 0]))
    assert L.lift_step_host(1, 1, 3, 7, pi(Cm), pi(Ad), pi(r), pi(rbar), pi(x), pi(cnt)) == 0
    assert cnt.tolist() == [1, 0] and x.tolist() == [5] and r.tolist() == [-2, 0, 0, 0]   # floor(-10 / 7)


# ---- the bound and the reconstruction ----------------------------------------------------------------------------------------------------------------------
def test_dixon_steps_on_a_hand_example():
    """A = (2 3; 3 10), b = (1, 1): D2 = 13 * 109 = 1417, N2 = 2 * 1417 = 2834, 4 N2 D2 = 16063112; 11^6 = 1771561 is below it and 11^8 above: K = 4"""
    assert 4 * 2834 * 1417 == 16063112 and 11 ** 6 <= 16063112 < 11 ** 8
    assert rounding.dixon_steps([[2, 3], [3, 10]], [1, 1], 11) == (4, 54, 38)              # isqrt(2834) = 53, isqrt(1417) = 37
    assert rounding.dixon_steps([[2, 3], [3, 10]], [1, 1], 11) == du.steps_and_bounds([[2, 3], [3, 10]], [1, 1], 11)
    assert rounding.dixon_steps([[0]], [0], 2) == (2, 2, 2)                                  # every factor at least 1: 2^(2K) > 4
    A, b = du.random_system(3, 9, 70, 10007)
    for p in (2, 10007, du.PMAX):
        assert rounding.dixon_steps(A, b, p) == du.steps_and_bounds(A, b, p)


def test_rational_reconstruction():
    m = 10007 ** 3
    third = pow(3, -1, m)
    assert rounding.rational_reconstruction(third, m, 100, 100) == F(1, 3)
    a = -22 * pow(7, -1, m) % m
    assert rounding.rational_reconstruction(a, m, 100, 100) == F(-22, 7)
    assert rounding.rational_reconstruction(a - 5 * m, m, 100, 100) == F(-22, 7)            # any representative
    assert rounding.rational_reconstruction(0, m, 100, 100) == 0 and rounding.rational_reconstruction(m - 5, m, 100, 100) == -5
    assert rounding.rational_reconstruction(a, m, 21, 100) is None and rounding.rational_reconstruction(a, m, 100, 6) is None
    for a in (third, a, 12345678):
        assert rounding.rational_reconstruction(a, m, 100, 100) == du.reconstruct(a, m, 100, 100)


# ---- the Python layer, the restatement as the device call ----------------------------------------------------------------------------------------------------
def test_prev_prime():
    assert [rounding.prev_prime(x) for x in (3, 4, 12, 14, 2 ** 23, 8388593)] == [2, 3, 11, 13, 8388593, 8388587]
    assert all(not rounding._is_prime(v) for v in range(8388588, 8388593))
    with pytest.raises(ValueError):
        rounding.prev_prime(2)


def test_solve_dixon_two_by_two():
    sol = rounding.solve_dixon([[2, 3], [3, 10]], [1, 1], lift=du.lift)
    assert list(sol) == [F(7, 11), F(-1, 11)] and sol.p == 8388593 and sol.primes == [8388593]
    assert sol.steps == du.steps_and_bounds([[2, 3], [3, 10]], [1, 1], 8388593)[0]
    assert list(rounding.solve_dixon([[2, 3], [3, 10]], [[1], [1]], lift=du.lift)) == list(sol)       # a column vector
    assert list(rounding.solve_dixon([], [], lift=du.lift)) == []


def test_solve_dixon_with_fractions():
    A = [[F(1, 2), F(1, 3), 0], [F(2, 5), 1, F(1, 7)], [0, F(3, 4), -2]]
    b = [F(3, 4), F(1, 2), 5]
    sol = rounding.solve_dixon(A, b, lift=du.lift)
    assert list(sol) == du.gauss_solve(A, b) and du.matvec(A, sol) == b


def test_solve_dixon_takes_the_next_prime():
    sol = rounding.solve_dixon([[8388593, 0], [0, 1]], [1, 2], lift=du.lift)
    assert list(sol) == [F(1, 8388593), 2] and sol.primes == [8388593, 8388587] and sol.p == 8388587
    with pytest.raises(rounding.SingularSystemError):
        rounding.solve_dixon([[8388593, 0], [0, 1]], [1, 2], maxprimes=1, lift=du.lift)


def test_solve_dixon_refuses():
    with pytest.raises(rounding.SingularSystemError) as e:
        rounding.solve_dixon([[1, 2], [2, 4]], [1, 2], lift=du.lift)
    assert isinstance(e.value, ValueError)
    with pytest.raises(ValueError):
        rounding.solve_dixon([[2, 3], [3, 10]], [1, 1], maxprimes=0, lift=du.lift)
    with pytest.raises(ValueError):
        rounding.solve_dixon([[2, 3, 1], [3, 10, 1]], [1, 1], lift=du.lift)
    # a lift that returns a wrong digit is caught by the check on the lifted integers

    def wrong(A, b, p, steps, device=0):
        X, r, rank = du.lift(A, b, p, steps)
        X[0, 0] = (int(X[0, 0]) + 1) % p
        return X, r, rank
    with pytest.raises(ArithmeticError):
        rounding.solve_dixon([[2, 3], [3, 10]], [1, 1], lift=wrong)


def test_solve_system_pseudoinverse():
    A = [[1, 2, F(1, 2)], [0, 1, -1]]                             # 2 x 3: the minimum-norm solution A^T (A A^T)^-1 b
    b = [F(3, 2), 4]
    G = [[sum(F(x) * y for x, y in zip(r, s)) for s in A] for r in A]
    y = du.gauss_solve(G, b)
    want = [sum(F(A[r][c]) * y[r] for r in range(2)) for c in range(3)]
    v = rounding.solve_system_pseudoinverse(A, b, lift=du.lift)
    assert v == want and du.matvec(A, v) == b
    At = [[A[r][c] for r in range(2)] for c in range(3)]           # 3 x 2: the least-squares solution (A^T A)^-1 A^T b
    b3 = [1, F(-1, 3), 2]
    G = [[sum(F(At[r][i]) * At[r][j] for r in range(3)) for j in range(2)] for i in range(2)]
    rhs = [sum(F(At[r][i]) * b3[r] for r in range(3)) for i in range(2)]
    assert rounding.solve_system_pseudoinverse(At, b3, lift=du.lift) == du.gauss_solve(G, rhs)
    assert rounding.solve_system_pseudoinverse([[2, 0], [0, 4]], [1, 1], lift=du.lift) == [F(1, 2), F(1, 4)]     # square: the tall branch
    with pytest.raises(rounding.SingularSystemError):
        rounding.solve_system_pseudoinverse([[1, 2, 3], [2, 4, 6]], [1, 2], lift=du.lift)


def test_rounding_settings():
    s = rounding.RoundingSettings()
    assert s.pseudo is True and s.pseudo_columnfactor == 1.05 and s.extracolumns_linindep is False
    assert rounding.RoundingSettings(pseudo_columnfactor=0.5).pseudo_columnfactor == 1


WIDE_A = [[F(1, 2), F(1, 3), 0, 1, 2, 1, 0, 3], [0, F(2, 5), 1, F(1, 7), 0, 2, 1, 1], [1, 0, 2, 0, 1, F(1, 3), 5, 0]]
WIDE_B = [F(3, 4), F(1, 2), 2]


def _project(A, b, **kw):
    return rounding.project_to_affine_space(A, b, batch=mu.host_batch, lift=du.lift, **kw)


def test_project_a_consistent_wide_system():
    x, ok, finished = _project(WIDE_A, WIDE_B)
    assert ok and finished and len(x) == 8 and du.matvec(WIDE_A, x) == WIDE_B
    # round(1.05 * 3) = 3 columns: the pivots alone, so the result is the solution of the square pivot system
    piv = list(rounding.system_pivots(WIDE_A, WIDE_B, batch=mu.host_batch)[0])
    assert piv == [0, 1, 2] and [x[c] for c in piv] == du.gauss_solve([[row[c] for c in piv] for row in WIDE_A], WIDE_B) and not any(x[3:])
    # five columns: the pivots and two more, chosen by the generator; the minimum-norm solution on them
    s = rounding.RoundingSettings(pseudo_columnfactor=1.7)
    x5, ok, finished = _project(WIDE_A, WIDE_B, settings=s, rng=np.random.default_rng(4))
    assert ok and finished and du.matvec(WIDE_A, x5) == WIDE_B
    extra = [int(c) for c in np.random.default_rng(4).permutation([3, 4, 5, 6, 7])][:2]
    cols = piv + extra
    sub = [[row[c] for c in cols] for row in WIDE_A]
    assert [x5[c] for c in cols] == rounding.solve_system_pseudoinverse(sub, WIDE_B, lift=du.lift) and sum(1 for v in x5 if v != 0) <= 5
    # the extra columns independent of each other
    s = rounding.RoundingSettings(pseudo_columnfactor=2.0, extracolumns_linindep=True)
    x6, ok, finished = _project(WIDE_A, WIDE_B, settings=s)
    assert ok and finished and du.matvec(WIDE_A, x6) == WIDE_B


def test_project_with_a_dependent_row():
    A = WIDE_A + [[x + y for x, y in zip(WIDE_A[0], WIDE_A[2])]]
    b = WIDE_B + [WIDE_B[0] + WIDE_B[2]]
    for s in (None, rounding.RoundingSettings(pseudo=False)):     # pseudo = False: four rows, three pivots, the normal equations
        x, ok, finished = _project(A, b, settings=s)
        assert ok and finished and du.matvec(A, x) == b


def test_project_an_inconsistent_system():
    A = WIDE_A + [[x + y for x, y in zip(WIDE_A[0], WIDE_A[2])]]
    b = WIDE_B + [WIDE_B[0] + WIDE_B[2] + 1]
    x, ok, finished = _project(A, b)
    assert x == [0] * 8 and ok is False and finished is False


def test_project_a_square_system_without_the_pseudoinverse():
    A = [[4, 1], [1, 3]]
    x, ok, finished = _project(A, [1, 1], settings=rounding.RoundingSettings(pseudo=False))
    assert x == [F(2, 11), F(3, 11)] and ok is True and finished is True
    assert _project(A, [1, 1])[0] == x
    # the reference's schedule of primes starts at next_prime(max |[A b]|) = 11 for (2 3; 3 10), which divides the determinant: b becomes a pivot column
    # and the system is reported inconsistent, as the reference does
    assert _project([[2, 3], [3, 10]], [1, 1]) == ([0, 0], False, False)


# ---- the binding -------------------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbol_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_dixon_lift\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "n", "p", "nd", "A_digits", "nbl", "b_limbs", "steps", "X", "r_limbs", "info"]
    want = [table[re.sub(r"\w+$", "", a).strip()] for a in args]
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_dixon_lift"] == (C.c_int, want)
    assert hasattr(_lib.load(), "clrs_modp_dixon_lift")
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    assert jl.count(":clrs_modp_dixon_lift") == 1 and "function solve_dixon(A::Nemo.ZZMatrix, b::Nemo.ZZMatrix" in jl
    for name in ("to_balanced_digits", "from_balanced_digits", "prev_prime", "dixon_steps", "dixon_lift", "rational_reconstruction", "SingularSystemError",
                 "solve_dixon", "solve_system_pseudoinverse", "project_to_affine_space"):
        assert name in rounding.__all__ and hasattr(rounding, name)


def test_refusals_need_no_device():
    """what clrs_modp_dixon_lift refuses, it refuses before it touches a device"""
    L = _lib.load()
    pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)
    A = np.array([[[2, 3], [3, 10]]], np.int32)
    b = np.array([[1, 1]], np.int32)
    X, r, info = (np.full(s, du.SENTINEL, np.int32) for s in ((3, 2), (3, 2), (4,)))
    call = lambda n=2, p=13, nd=1, A=A, nbl=1, b=b, steps=3, X=X, r=r, info=info: L.clrs_modp_dixon_lift(0, n, p, nd, pi(A), nbl, pi(b), steps, pi(X), pi(r), pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9, -7):
        assert call(p=p) == -1
    assert call(n=-1) == -1 and call(n=32768) == -1
    assert call(nd=0) == -1 and call(nbl=0) == -1 and call(steps=-1) == -1
    assert call(A=np.array([[[2, 3], [3, 2 ** 23]]], np.int32)) == -1
    assert call(A=np.array([[[2, 3], [3, -2 ** 23 - 1]]], np.int32)) == -1
    assert call(b=np.array([[1, 2 ** 23]], np.int32)) == -1
    assert call(A=None) == -1 and call(b=None) == -1 and call(X=None) == -1 and call(r=None) == -1 and call(info=None) == -1
    assert b"null" in L.clrs_last_error()
    assert all(int(v) == du.SENTINEL for a in (X, r, info) for v in a.flat)
    # n = 0: rank 0, no device
    assert L.clrs_modp_dixon_lift(0, 0, 13, 1, None, 1, None, 3, None, None, pi(info)) == 0 and info.tolist() == [0, 3, 0, 0]
    with pytest.raises(ValueError):
        rounding.dixon_lift([[2, 3], [3, 10]], [1, 1], 4, 3)
    with pytest.raises(ValueError):
        rounding.dixon_lift([[2, 3, 4], [3, 10, 4]], [1, 1], 13, 3)


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    if torch.cuda.is_available():
        assert list(rounding.solve_dixon([[2, 3], [3, 10]], [1, 1])) == [F(7, 11), F(-1, 11)]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.solve_dixon([[2, 3], [3, 10]], [1, 1])

"""Dixon's p-adic lifting on the device (clrs_modp_dixon_lift: k_lift_residues, the elimination of clrs_modp_rref, k_lift_x, k_lift_r)
against the restatement of tests/dixon_util.py with `==` -- the p-adic digits are unique -- and, independently of it, against the identity
A sum_k X[k] p^k == b - p^K r and the exact Fraction solve; the refusals; the front ends of clrs_amd.rounding on the device."""
import functools
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import modp_util as mu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
_pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)


def device_lift(A, b, p, steps):
    """one raw call on sentinel-filled outputs: (code, X, r_limbs, info, nd, nbl)"""
    Ad, bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(b)
    nd, nbl, n = Ad.shape[0], bl.shape[0], Ad.shape[1]
    X = np.full((steps, n), du.SENTINEL, np.int32)
    r = np.full((max(nbl, nd + 1) + 1, n), du.SENTINEL, np.int32)
    info = np.full(4, du.SENTINEL, np.int32)
    code = _lib.load().clrs_modp_dixon_lift(0, n, int(p), nd, _pi(Ad), nbl, _pi(bl), int(steps), _pi(X) if X.size else None, _pi(r), _pi(info))
    return code, X, r, info, nd, nbl


def check_case(A, b, p, steps=None):
    n = A.shape[0]
    K, N, D = du.steps_and_bounds(A, b, p)
    full = steps is None
    steps = K if full else steps
    want_X, want_r, rank = du.lift(A, b, p, steps)
    assert rank == n                                              # the generators yield matrices invertible mod p
    code, X, r, info, nd, nbl = device_lift(A, b, p, steps)
    assert code == 0, _lib.load().clrs_last_error()
    assert info.tolist() == [n, steps, 0, 0]
    assert X.min(initial=0) >= 0 and X.max(initial=0) < p
    assert np.array_equal(X, want_X)
    got_r = [int(v) for v in rounding.from_balanced_digits(r)]
    assert got_r == want_r
    # independently of the restatement: A x == b - p^steps r
    x = du.horner(X, p)
    m = p ** steps
    assert [int(v) for v in A.dot(du.objects(x))] == [int(v) - m * w for v, w in zip(b, got_r)]
    if full and n <= 33:
        sol = [du.reconstruct(v, m, N, D) for v in x]
        assert sol == du.gauss_solve(A, b)
    return nd, nbl


CASES = {
    "n=1": lambda: (*du.random_system(11, 1, 20, 10007), 10007),
    "n=2": lambda: (*du.random_system(12, 2, 20, 10007), 10007),
    "n=17 p=2": lambda: (*du.random_system(13, 17, None, 2, lo_entries=8), 2),
    # one digit: one full wave of columns (64 lanes x 4 ints = 256 would be one trip; 64 columns are 16 lanes) and one column either side
    "n=63": lambda: (*du.random_system(14, 63, 12, 10007), 10007),
    "n=64": lambda: (*du.random_system(15, 64, 12, 10007), 10007),
    "n=65": lambda: (*du.random_system(16, 65, 12, 10007), 10007),
    "n=129": lambda: (*du.random_system(17, 129, 8, 10007), 10007),          # a row count not divisible by 4: the last workgroup has one row
    "n=257": lambda: (*du.random_system(18, 257, 3, 10007), 10007),          # 260 padded ints = 65 lanes' worth: a second trip of the column loop
    "n=33 two digits": lambda: (*du.random_system(19, 33, 40, du.PMAX), du.PMAX),
    "n=65 three digits": lambda: (*du.random_system(20, 65, 71, du.PMAX, bbits=133), du.PMAX),
    "n=65 extreme": lambda: (*du.extreme_system(65), du.PMAX),
    "n=16 boundaries": lambda: (*du.boundary_system(10007), 10007),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@pytest.mark.parametrize("name", list(CASES))
def test_shapes_against_the_restatement(name):
    A, b, p = _case(name)
    nd, nbl = check_case(A, b, p)
    if name == "n=65 three digits":
        assert nd == 3 and nbl > nd                               # 72-bit entries, b around 10^40
    if name == "n=65 extreme":
        assert nd == 2 and max(abs(int(v)) for v in A.dot(du.objects([du.PMAX - 1] * 65))) > 2 ** 75
    if name in ("n=63", "n=64", "n=65", "n=129", "n=257"):
        assert nd == 1


def test_zero_right_hand_side():
    A, _, p = _case("n=17 p=2")
    A2, _, p2 = _case("n=33 two digits")
    for M, q in ((A, p), (A2, p2)):
        code, X, r, info, _, _ = device_lift(M, du.objects([0] * M.shape[0]), q, 5)
        assert code == 0 and info.tolist() == [M.shape[0], 5, 0, 0] and not X.any() and not r.any()


@pytest.mark.parametrize("steps", (0, 1))
def test_no_step_and_one_step(steps):
    A, b, p = _case("n=65 three digits")
    check_case(A, b, p, steps=steps)
    if steps == 0:                                                # the residual is b itself
        code, X, r, info, _, _ = device_lift(A, b, p, 0)
        assert code == 0 and [int(v) for v in rounding.from_balanced_digits(r)] == [int(v) for v in b]


def test_singular_mod_p_is_no_error():
    A, b = du.objects([[2, 3], [3, 10]]), du.objects([1, 1])
    code, X, r, info, _, _ = device_lift(A, b, 11, 4)
    assert code == 0 and info.tolist() == [1, 0, 0, 0]
    assert (X == du.SENTINEL).all() and (r == du.SENTINEL).all()
    assert rounding.dixon_lift(A, b, 11, 4) == (None, None, 1)
    X, r, rank = rounding.dixon_lift(A, b, 13, 4)
    want = du.lift(A, b, 13, 4)
    assert rank == 2 and np.array_equal(X, want[0]) and [int(v) for v in r] == want[1]
    # a larger one: a zero row at every prime
    A = du.objects(np.arange(36).reshape(6, 6) % 7)
    A[4] = 0
    assert rounding.dixon_lift(A, du.objects([1] * 6), 10007, 3)[2] == du.inverse_mod_p(A, 10007)[1] < 6


def test_refusals_leave_the_library_working():
    L = _lib.load()
    A = np.array([[[2, 3], [3, 10]]], np.int32)
    b = np.array([[1, 1]], np.int32)
    X, r, info = (np.full(s, du.SENTINEL, np.int32) for s in ((3, 2), (3, 2), (4,)))
    call = lambda n=2, p=13, nd=1, A=A, nbl=1, b=b, steps=3, X=X, r=r, info=info: L.clrs_modp_dixon_lift(0, n, p, nd, _pi(A), nbl, _pi(b), steps, _pi(X), _pi(r), _pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9):
        assert call(p=p) == INVALID
    assert call(n=-1) == INVALID and call(n=32768) == INVALID and call(nd=0) == INVALID and call(nbl=0) == INVALID and call(steps=-1) == INVALID
    assert call(A=np.array([[[2, 3], [3, 2 ** 23]]], np.int32)) == INVALID and call(b=np.array([[1, -2 ** 23 - 1]], np.int32)) == INVALID
    assert call(A=None) == INVALID and call(info=None) == INVALID
    assert all(int(v) == du.SENTINEL for a in (X, r, info) for v in a.flat)
    assert L.clrs_modp_dixon_lift(0, 0, 13, 1, None, 1, None, 3, None, None, _pi(info)) == 0 and info.tolist() == [0, 3, 0, 0]
    assert call() == 0 and info.tolist() == [2, 3, 0, 0]
    want = du.lift([[2, 3], [3, 10]], [1, 1], 13, 3)
    assert np.array_equal(X, want[0]) and [int(v) for v in rounding.from_balanced_digits(r)] == want[1]


# ---- the front ends on the device, n = 48, against Fraction arithmetic ---------------------------------------------------------------------------------------
def test_solve_dixon_on_the_device():
    A, b = du.random_system(31, 48, 6, du.PMAX)
    A = [[F(int(v)) for v in row] for row in A]
    A[0] = [v / 3 for v in A[0]]                                  # a row with denominators
    b = [F(int(v), 5) for v in b]
    sol = rounding.solve_dixon(A, b)
    assert list(sol) == du.gauss_solve(A, b) and sol.primes == [du.PMAX] and sol.steps > 0
    assert list(sol) == list(rounding.solve_dixon(A, b, lift=du.lift))


def test_solve_system_pseudoinverse_on_the_device():
    rng = np.random.default_rng(32)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 51))]
    b = [F(int(v)) for v in rng.integers(-9, 10, size=48)]
    G = [[sum(x * y for x, y in zip(r, s)) for s in A] for r in A]
    y = du.gauss_solve(G, b)
    v = rounding.solve_system_pseudoinverse(A, b)
    assert v == [sum(A[r][c] * y[r] for r in range(48)) for c in range(51)] and du.matvec(A, v) == b


def test_project_to_affine_space_on_the_device():
    rng = np.random.default_rng(33)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 60))]
    A[47] = [x + y for x, y in zip(A[0], A[1])]                    # a dependent row
    x0 = [F(int(v), 7) for v in rng.integers(-9, 10, size=60)]
    b = du.matvec(A, x0)
    x, ok, finished = rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5))
    assert ok and finished and du.matvec(A, x) == b
    assert sum(1 for v in x if v != 0) <= round(1.05 * 48)
    host = rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5), batch=mu.host_batch, lift=du.lift)
    assert (x, ok, finished) == host
    b[47] += 1
    assert rounding.project_to_affine_space(A, b) == ([0] * 60, False, False)

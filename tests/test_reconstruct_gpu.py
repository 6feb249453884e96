"""The rational reconstruction on the device (clrs_modp_dixon_reconstruct: k_rec_horner, k_rec_euclid) against
rounding.rational_reconstruction on Python integers with `==`: limb counts at the lane-stride edges, small primes, entry counts, named single entries with
quotients far longer than a limb, the refusals, and the front ends of clrs_amd.rounding with `reconstruct=dixon_reconstruct`."""
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import modp_util as mu
from tests import reconstruct_util as ru

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
_pi = ru._pi


def check_case(X, p, N, D, kinds=None, extra_limbs=0):
    """one raw call against the oracle, entry by entry; returns info"""
    steps, n = X.shape
    m = p ** steps
    Lm = ru.length(m)
    code, num, den, neg, status, xl, info = ru.device_reconstruct(X, p, N, D, nx=Lm + extra_limbs, nl=max(ru.length(N), ru.length(D), 1) + extra_limbs)
    assert code == 0, _lib.load().clrs_last_error()
    assert info[0] == Lm and info[3] == 0 and 0 <= info[1] <= info[2] <= n * info[1]
    x = ru.horner(X, p)
    assert xl.min() >= 0 and xl.max() < ru.BASE and [ru.value(row) for row in xl] == x                # the Python Horner, every entry
    want = ru.oracle(x, m, N, D)
    got = [(int(status[i]), int(neg[i]), ru.value(num[i]), ru.value(den[i])) for i in range(n)]
    assert num.min() >= 0 and num.max() < ru.BASE and den.min() >= 0 and den.max() < ru.BASE
    assert got == want                                              # status, sign, numerator, denominator: accepted and rejected alike
    if kinds is not None:
        assert "fraction" in kinds and (n == 1 or "random" in kinds)
        if D > 0:
            assert all(w[0] == 0 for w, k in zip(want, kinds) if k == "fraction")
    # the Python front end on the same call
    fr, xs = rounding.dixon_reconstruct(X, p, N, D, want_x=True)
    assert xs == x and fr == [rounding.rational_reconstruction(v, m, N, D) for v in x]
    assert all(f is None or (f.numerator, f.denominator) == (F(f.numerator, f.denominator).numerator, F(f.numerator, f.denominator).denominator) for f in fr)
    assert rounding.dixon_reconstruct.last_info == [int(v) for v in info]
    return info


@pytest.mark.parametrize("steps,Lm", ((1, 1), (2, 2), (3, 3), (65, 63), (66, 64), (67, 65), (134, 129)))
def test_limb_counts_at_the_lane_stride_edges(steps, Lm):
    X, kinds, N, D = ru.mixed_case(ru.PMAX, steps, 5)
    info = check_case(X, ru.PMAX, N, D, kinds)
    assert info[0] == Lm
    if steps == 67:
        assert 350 < info[1] < 600                                  # the quotients of a random entry at 65 limbs (417 to 486 on the host)


@pytest.mark.parametrize("p,steps", ((2, 1), (2, 24), (2, 25), (10007, 2), (10007, 40)))
def test_small_primes(p, steps):
    X, kinds, N, D = ru.mixed_case(p, steps, 5)
    check_case(X, p, N, D, kinds)


@pytest.mark.parametrize("n", (1, 5, 130))
def test_entry_counts(n):
    X, kinds, N, D = ru.mixed_case(ru.PMAX, 67, n)
    info = check_case(X, ru.PMAX, N, D, kinds, extra_limbs=3 if n == 5 else 0)        # (rows wider than they need to be: the rest is zero)
    if n == 130:
        assert info[2] > 20000                                      # 65 random entries of more than 350 steps each


@pytest.mark.parametrize("name", list(ru.named_cases()))
def test_named_single_entries(name):
    a, N, D, want = ru.named_cases()[name]
    X = ru.padic_digits(a, ru.PMAX, 67)
    info = check_case(X, ru.PMAX, N, D)
    assert rounding.dixon_reconstruct(X, ru.PMAX, N, D) == [want]
    if name in ("a=3, N=1", "a=2^30+12345, N=2^20"):
        assert want is not None and info[1] >= 63                   # a quotient of more than 1500 bits: at least 63 pieces of 24
    if name in ("a=p", "D one below"):
        assert want is None
    if name in ("a=0", "a=1"):
        assert info[1] == 0


def test_all_named_entries_in_one_call_with_the_widest_bounds():
    """the same entries side by side under N = 2^20, D = m: waves that stop at once beside waves that run long"""
    cases = ru.named_cases()
    X = np.concatenate([ru.padic_digits(c[0], ru.PMAX, 67) for c in cases.values()], axis=1)
    check_case(X, ru.PMAX, 2 ** 20, ru.P67)
    check_case(X, ru.PMAX, 0, ru.P67)                               # N = 0: the whole Euclid, down to the gcd
    check_case(X, ru.PMAX, ru.P67, 1)                               # N = m: no step at all, every entry is x / 1


def test_refusals_leave_the_library_working():
    L = _lib.load()
    X = ru.padic_digits(pow(3, -1, 13 ** 3), 13, 3)
    X = np.concatenate([X, ru.padic_digits(-22 * pow(7, -1, 13 ** 3) % 13 ** 3, 13, 3)], axis=1)
    Nl, Dl = np.array([33], np.int32), np.array([33, 0], np.int32)
    num, den, neg, status, xl, info = (np.full(s, ru.SENTINEL, np.int32) for s in ((2, 1), (2, 1), (2,), (2,), (2, 1), (4,)))

    def call(n=2, p=13, steps=3, X=X, nN=1, N=Nl, nD=2, D=Dl, nl=1, num=num, den=den, neg=neg, status=status, nx=1, xl=xl, info=info):
        return L.clrs_modp_dixon_reconstruct(0, n, p, steps, _pi(X), nN, _pi(N), nD, _pi(D), nl, _pi(num), _pi(den), _pi(neg), _pi(status), nx, _pi(xl), _pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9):
        assert call(p=p) == INVALID
    assert call(n=-1) == INVALID and call(n=32768) == INVALID and call(steps=0) == INVALID
    bad = X.copy()
    bad[1, 1] = 13
    assert call(X=bad) == INVALID and call(N=np.array([1 << 24], np.int32)) == INVALID and call(D=np.array([33, 1], np.int32)) == INVALID
    assert call(nx=0) == INVALID and call(X=None) == INVALID and call(info=None) == INVALID and call(status=None) == INVALID
    assert all(int(v) == ru.SENTINEL for a in (num, den, neg, status, xl, info) for v in a.flat)
    assert L.clrs_modp_dixon_reconstruct(0, 0, 13, 3, None, 1, None, 1, None, 1, None, None, None, None, 0, None, _pi(info)) == 0 and info.tolist() == [0, 0, 0, 0]
    assert call() == 0 and info[0] == 1 and info[3] == 0
    assert status.tolist() == [0, 0] and neg.tolist() == [0, 1] and num[:, 0].tolist() == [1, 22] and den[:, 0].tolist() == [3, 7]
    assert xl[:, 0].tolist() == ru.horner(X, 13)
    assert call(xl=None) == 0                                       # x_limbs may be null
    import ctypes as C
    h, e = C.c_double(-1.0), C.c_double(-1.0)
    assert L.clrs_modp_dixon_reconstruct_times(C.byref(h), C.byref(e)) == 0 and h.value >= 0.0 and e.value >= 0.0


# ---- the front ends on the device, n = 48, against Fraction arithmetic and against the default path ------------------------------------------------------------
def test_solve_dixon_with_the_device_reconstruction():
    A, b = du.random_system(31, 48, 6, du.PMAX)
    A = [[F(int(v)) for v in row] for row in A]
    A[0] = [v / 3 for v in A[0]]                                  # a row with denominators
    b = [F(int(v), 5) for v in b]
    sol = rounding.solve_dixon(A, b, reconstruct=rounding.dixon_reconstruct)
    host = rounding.solve_dixon(A, b)
    assert list(sol) == du.gauss_solve(A, b) == list(host) and (sol.p, sol.primes, sol.steps) == (host.p, host.primes, host.steps)
    assert list(rounding.solve_dixon(A, b, reconstruct=rounding.dixon_reconstruct, check=False)) == list(host)


def test_solve_system_pseudoinverse_with_the_device_reconstruction():
    rng = np.random.default_rng(32)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 51))]
    b = [F(int(v)) for v in rng.integers(-9, 10, size=48)]
    G = [[sum(x * y for x, y in zip(r, s)) for s in A] for r in A]
    y = du.gauss_solve(G, b)
    v = rounding.solve_system_pseudoinverse(A, b, reconstruct=rounding.dixon_reconstruct)
    assert v == [sum(A[r][c] * y[r] for r in range(48)) for c in range(51)] and du.matvec(A, v) == b
    assert v == rounding.solve_system_pseudoinverse(A, b)


def test_project_to_affine_space_with_the_device_reconstruction():
    rng = np.random.default_rng(33)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 60))]
    A[47] = [x + y for x, y in zip(A[0], A[1])]                    # a dependent row
    x0 = [F(int(v), 7) for v in rng.integers(-9, 10, size=60)]
    b = du.matvec(A, x0)
    x, ok, finished = rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5), reconstruct=rounding.dixon_reconstruct)
    assert ok and finished and du.matvec(A, x) == b
    assert (x, ok, finished) == rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5))
    assert (x, ok, finished) == rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5), batch=mu.host_batch, lift=du.lift)

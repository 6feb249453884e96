"""The lifting with a matrix of right-hand sides and the basis change built on it (clrs_modp_dixon_lift_multi), without a device: the
per-entry residual update of csrc/clrs_modp_lift_arith.h compiled for the host against a restatement in Python integers, a host step loop against the
single-column restatement of tests/dixon_util.py, the Python front ends of clrs_amd.rounding with stand-ins for the device calls against Fraction
arithmetic, the binding and the refusals.  Everything is exact: every comparison is `==`."""
import ctypes as C
import json
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_multi_util as dm
from tests import dixon_util as du
from tests import modp_util as mu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
UNREDUCED = rounding.RoundingSettings(reduce_kernelvectors=False)
PLAIN = rounding.RoundingSettings(reduce_kernelvectors=False, normalize_transformation=False)
HOOKS = dict(lift=dm.lift_columns, batch=mu.host_batch)


# ---- liftm_entry against Python integers -------------------------------------------------------------------------------------------------------------------
def _compare_entries(lo, hi, r, p):
    """lo, hi (nd, count) Python integers, r (nrl + 1, count) limbs: the host build against the restatement, entry by entry; returns the flags"""
    got_r, got_rbar, got_flags = dm.host_entries(lo, hi, r, p)
    for e in range(len(lo[0])):
        limbs, res, flags = dm.entry_restated([row[e] for row in lo], [row[e] for row in hi], [int(v) for v in np.asarray(r)[:, e]], p)
        assert int(got_flags[e]) == flags, (e, int(got_flags[e]), flags)
        if not flags & 2:
            assert [int(v) for v in got_r[:, e]] == limbs and int(got_rbar[e]) == res, e
    return [int(v) for v in got_flags]


def _divisible_case(rng, nd, nrl, p, count, lo_of, hi_of):
    """entries with r = p q + A x exactly: q random in nrl - 1 limbs (of either sign), (lo, hi) from the given generators"""
    lo = [[lo_of() for _ in range(count)] for _ in range(nd)]
    hi = [[hi_of() for _ in range(count)] for _ in range(nd)]
    r = np.zeros((nrl + 1, count), np.int32)
    for e in range(count):
        q = (int.from_bytes(rng.bytes(3 * (nrl - 1)), "little") >> 2) * (-1 if rng.integers(2) else 1)         # p q stays below 2^(24 nrl - 3)
        s = sum((lo[l][e] + (hi[l][e] << 24)) << (24 * l) for l in range(nd))
        r[:nrl, e] = du.balanced(p * q + s, nrl)
    return lo, hi, r


@pytest.mark.parametrize("p", (2, 10007, du.PMAX))
@pytest.mark.parametrize("nd", (1, 2, 3))
def test_entry_random_planes_against_python_integers(p, nd):
    rng = np.random.default_rng(100 * nd + p % 97)
    nrl, count = nd + 3, 64
    lo_of = lambda: int(rng.integers(-2 ** 23, 2 ** 23 + 1))
    hi_of = lambda: int(rng.integers(-2 ** 30, 2 ** 30))
    # any residual: the division mostly leaves a remainder, and the flag must say so
    lo = [[lo_of() for _ in range(count)] for _ in range(nd)]
    hi = [[hi_of() for _ in range(count)] for _ in range(nd)]
    r = rng.integers(-2 ** 23, 2 ** 23, size=(nrl + 1, count)).astype(np.int32)
    r[nrl] = 0
    flags = _compare_entries(lo, hi, r, p)
    assert p == 2 or any(f & 1 for f in flags)
    # residuals that p divides, positive and negative
    lo, hi, r = _divisible_case(rng, nd, nrl, p, count, lo_of, hi_of)
    assert _compare_entries(lo, hi, r, p) == [0] * count
    assert any(du.value(r[:, e]) < 0 for e in range(count)) and any(du.value(r[:, e]) > 0 for e in range(count))


def test_entry_at_the_largest_magnitudes():
    """hi as large as n = 32767 allows (n 2^22 + n), lo at +-2^23, limbs of r at -2^23 and 2^23 - 1"""
    rng = np.random.default_rng(7)
    top = 32767 * 2 ** 22 + 32767
    for nd in (1, 2, 3):
        nrl = nd + 2
        for p in (2, du.PMAX):
            ext_lo, ext_hi = (lambda: int(rng.choice([-2 ** 23, 2 ** 23]))), (lambda: int(rng.choice([-top, top])))
            lo, hi, r = _divisible_case(rng, nd, nrl, p, 32, ext_lo, ext_hi)
            assert _compare_entries(lo, hi, r, p) == [0] * 32
            # digits of r at the two ends of the balanced range, whatever that does to divisibility
            r = rng.choice(np.array([-2 ** 23, 2 ** 23 - 1], np.int32), size=(nrl + 1, 32))
            r[nrl] = 0
            r[nrl - 1] = 0                                         # (room for the quotient: the top limb of a lifted residual is empty, nrl = max(nbl, nd + 1) + 1)
            _compare_entries([[ext_lo() for _ in range(32)] for _ in range(nd)], [[ext_hi() for _ in range(32)] for _ in range(nd)], r, p)


def test_entry_planted_remainder_and_planted_overflow():
    rng = np.random.default_rng(8)
    nd, nrl, p = 2, 4, 10007
    lo_of, hi_of = (lambda: int(rng.integers(-2 ** 23, 2 ** 23 + 1))), (lambda: int(rng.integers(-2 ** 30, 2 ** 30)))
    lo, hi, r = _divisible_case(rng, nd, nrl, p, 16, lo_of, hi_of)
    v = du.value(r[:, 5]) + 1                                     # entry 5: one more than a multiple of p
    r[:nrl, 5] = du.balanced(v, nrl)
    flags = _compare_entries(lo, hi, r, p)
    assert flags == [1 if e == 5 else 0 for e in range(16)]
    # an overflow: a top limb that is no balanced digit, so that the quotient by 2 needs more than nrl limbs
    lo, hi, r = _divisible_case(rng, nd, nrl, 2, 16, lo_of, hi_of)
    r[nrl - 1, 9] = 2 ** 30
    flags = _compare_entries(lo, hi, r, 2)
    assert [f & 2 for f in flags] == [2 if e == 9 else 0 for e in range(16)]


# ---- the host step loop against the single-column restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("one digit", "three digits", "p=2", "extreme", "boundary"))
def test_host_step_loop_against_the_restatement_column_by_column(name):
    if name == "one digit":
        (A, _), p, steps = du.random_system(41, 9, 12, 10007), 10007, 6
        B = dm.random_rhs(42, 9, 5, 12)
    elif name == "three digits":
        (A, _), p, steps = du.random_system(43, 7, 71, du.PMAX), du.PMAX, 5
        B = dm.random_rhs(44, 7, 4, 62) * (1 << 70) + dm.random_rhs(45, 7, 4, 62)
    elif name == "p=2":
        (A, _), p, steps = du.random_system(46, 11, None, 2, lo_entries=8), 2, 12
        B = dm.random_rhs(47, 11, 3, 5)
    elif name == "extreme":
        (A, _), p, steps = du.extreme_system(20), du.PMAX, 4
        B = du.objects([[1, int(i == 0), 2 ** 47 + 2 ** 23] for i in range(20)])
    else:
        (A, b), p, steps = du.boundary_system(10007), 10007, 5
        B = du.objects(np.stack([b, -b, du.objects([1] * 16)], axis=1))
    X, R, cnt = dm.host_lift_multi(A, B, p, steps)
    assert cnt == [0, 0]
    for j in range(B.shape[1]):
        wx, wr, rank = du.lift(A, B[:, j], p, steps)
        assert rank == A.shape[0] and np.array_equal(X[:, :, j], wx) and [int(v) for v in R[:, j]] == wr


# ---- solve_dixon_multi with stand-ins -----------------------------------------------------------------------------------------------------------------------
def _columns_by_gauss(A, B):
    B = np.asarray(B, dtype=object)
    return [du.gauss_solve(A, list(B[:, j])) for j in range(B.shape[1])]


def test_solve_dixon_multi_integers_and_fractions():
    A, _ = du.random_system(51, 7, 6, du.PMAX)
    B = dm.random_rhs(52, 7, 4, 6)
    S = rounding.solve_dixon_multi(A, B, lift=dm.lift_columns)
    assert isinstance(S, rounding.DixonSolutionMatrix) and S.shape == (7, 4) and S.p == du.PMAX and S.primes == [du.PMAX] and S.steps > 0
    assert [list(S[:, j]) for j in range(4)] == _columns_by_gauss(A, B)
    # the number of steps: that of the column of largest norm
    norms = [sum(int(v) ** 2 for v in B[:, j]) for j in range(4)]
    assert S.steps == du.steps_and_bounds(A, B[:, norms.index(max(norms))], du.PMAX)[0]
    Af = [[F(int(v)) for v in row] for row in A]
    Af[2] = [v / 6 for v in Af[2]]
    Bf = [[F(int(v), 1 + (i + j) % 4) for j, v in enumerate(row)] for i, row in enumerate(B)]
    S = rounding.solve_dixon_multi(Af, Bf, lift=dm.lift_columns)
    assert [list(S[:, j]) for j in range(4)] == _columns_by_gauss(Af, Bf)
    # a single solve_dixon per column gives the same fractions
    for j in range(4):
        assert list(S[:, j]) == list(rounding.solve_dixon(Af, [row[j] for row in Bf], lift=du.lift))


def test_solve_dixon_multi_takes_the_next_prime_and_reports_a_singular_matrix():
    A = [[du.PMAX, 1], [0, 1]]                                    # singular mod the first prime, regular mod the second
    B = [[1, 2, 3], [4, 5, 6]]
    S = rounding.solve_dixon_multi(A, B, lift=dm.lift_columns)
    assert S.primes == [du.PMAX, rounding.prev_prime(du.PMAX)] and S.p == S.primes[1]
    assert [list(S[:, j]) for j in range(3)] == _columns_by_gauss(A, B)
    with pytest.raises(rounding.SingularSystemError):
        rounding.solve_dixon_multi([[1, 2], [2, 4]], [[1], [1]], lift=dm.lift_columns)
    with pytest.raises(rounding.SingularSystemError):
        rounding.solve_dixon_multi(A, B, maxprimes=1, lift=dm.lift_columns)
    with pytest.raises(ValueError):
        rounding.solve_dixon_multi(A, B, maxprimes=0, lift=dm.lift_columns)
    with pytest.raises(ValueError):
        rounding.solve_dixon_multi([[1, 2, 3], [4, 5, 6]], B, lift=dm.lift_columns)
    with pytest.raises(ValueError):
        rounding.solve_dixon_multi(A, [[1, 2, 3]], lift=dm.lift_columns)


def test_solve_dixon_multi_empty_shapes_need_no_lift():
    def never(*a, **k):
        raise AssertionError("nothing to lift")
    S = rounding.solve_dixon_multi([[1, 2], [3, 4]], np.zeros((2, 0), dtype=object), lift=never)
    assert S.shape == (2, 0) and S.p is None and S.primes == [] and S.steps == 0
    S = rounding.solve_dixon_multi(np.zeros((0, 0), dtype=object), np.zeros((0, 3), dtype=object), lift=never)
    assert S.shape == (0, 3)
    assert rounding.inverse_qq(np.zeros((0, 0), dtype=object), lift=never).shape == (0, 0)


def test_solve_dixon_multi_hooks_take_matrices_not_columns():
    A, _ = du.random_system(53, 6, 5, du.PMAX)
    B = dm.random_rhs(54, 6, 5, 5)
    want = _columns_by_gauss(A, B)
    mm, rec, lift = dm.Counting(dm.host_matmul), dm.Counting(dm.host_reconstruct), dm.Counting(dm.lift_columns)
    S = rounding.solve_dixon_multi(A, B, lift=lift, reconstruct=rec, matmul=mm)
    assert [list(S[:, j]) for j in range(5)] == want
    assert lift.calls == 1 and lift.shapes[0] == ((6, 6), (6, 5))
    assert mm.calls == 2 and mm.shapes == [((6, 6), (6, 5))] * 2                  # A X of the lifted integers, A Y over the common denominators
    assert rec.calls == 1 and rec.shapes[0][0] == (S.steps, 30)                   # 30 entries: one piece
    mm2, rec2 = dm.Counting(dm.host_matmul), dm.Counting(dm.host_reconstruct)
    S2 = rounding.solve_dixon_multi(A, B, lift=dm.lift_columns, reconstruct=rec2, matmul=mm2, check=False)
    assert np.array_equal(S2, S) and mm2.calls == 0 and rec2.calls == 1
    # the checks do check: a lift that lies about one residue
    def wrong(A, B, p, steps, device=0):
        X, R, rank = dm.lift_columns(A, B, p, steps)
        X[0, 0, 0] = (int(X[0, 0, 0]) + 1) % p
        return X, R, rank
    with pytest.raises(ArithmeticError):
        rounding.solve_dixon_multi(A, B, lift=wrong)
    with pytest.raises(ArithmeticError):
        rounding.solve_dixon_multi(A, B, lift=wrong, reconstruct=dm.host_reconstruct, matmul=dm.host_matmul)


def test_reconstruct_is_fed_pieces_of_at_most_lift_max_n_entries(monkeypatch):
    monkeypatch.setattr(rounding, "LIFT_MAX_N", 7)
    A, _ = du.random_system(55, 4, 4, du.PMAX)
    B = dm.random_rhs(56, 4, 5, 4)
    rec = dm.Counting(dm.host_reconstruct)
    S = rounding.solve_dixon_multi(A, B, lift=dm.lift_columns, reconstruct=rec)
    assert [list(S[:, j]) for j in range(5)] == _columns_by_gauss(A, B)
    assert [s[0][1] for s in rec.shapes] == [7, 7, 6]


# ---- inverse_qq ---------------------------------------------------------------------------------------------------------------------------------------------
def test_inverse_qq_times_the_matrix_is_the_identity():
    A, _ = du.random_system(57, 8, 7, du.PMAX)
    Af = [[F(int(v), 1 + (i * j) % 5) for j, v in enumerate(row)] for i, row in enumerate(A)]
    Binv = rounding.inverse_qq(Af, lift=dm.lift_columns)
    assert dm.frac_matmul(Af, Binv) == dm.identity(8) and dm.frac_matmul(Binv, Af) == dm.identity(8)
    with pytest.raises(rounding.SingularSystemError):
        rounding.inverse_qq([[1, 2, 3], [4, 5, 6], [5, 7, 9]], lift=dm.lift_columns)
    with pytest.raises(ValueError):
        rounding.inverse_qq([[1, 2, 3], [4, 5, 6]], lift=dm.lift_columns)


def test_inverse_qq_of_the_hilbert_matrix_of_order_8():
    from math import comb
    n = 8
    H = [[F(1, i + j + 1) for j in range(n)] for i in range(n)]
    closed = [[F((-1) ** (i + j) * (i + j + 1) * comb(n + i, n - j - 1) * comb(n + j, n - i - 1) * comb(i + j, i) ** 2) for j in range(n)] for i in range(n)]
    got = rounding.inverse_qq(H, lift=dm.lift_columns, reconstruct=dm.host_reconstruct, matmul=dm.host_matmul)
    assert [list(row) for row in got] == closed


def test_inverse_qq_of_a_unimodular_matrix_is_an_integer_matrix():
    rng = np.random.default_rng(58)
    n = 9
    L, U = np.tril(rng.integers(-3, 4, size=(n, n)), -1) + np.eye(n, dtype=np.int64), np.triu(rng.integers(-3, 4, size=(n, n)), 1) + np.eye(n, dtype=np.int64)
    M = du.objects(L.dot(U))
    inv = rounding.inverse_qq(M, lift=dm.lift_columns)
    assert all(v.denominator == 1 for v in inv.flat)
    assert dm.frac_matmul(M, inv) == dm.identity(n)


# ---- complete_basis ------------------------------------------------------------------------------------------------------------------------------------------
def test_complete_basis_is_the_greedy_exact_choice():
    rng = np.random.default_rng(59)
    seen = set()
    for trial in range(24):
        N = int(rng.integers(1, 13))
        s = int(rng.integers(0, N + 1))
        while True:
            V = np.array([[F(int(rng.integers(-2, 3)), int(rng.integers(1, 4))) for _ in range(s)] for _ in range(N)], dtype=object).reshape(N, s)
            V[rng.integers(0, N, size=min(N // 2, N - s))] = F(0)      # zero rows: the e_i there must be taken (at least s rows stay)
            if s == 0 or dm.frac_rank([list(V[:, c]) for c in range(s)]) == s:
                break
        got = rounding.complete_basis(V, batch=mu.host_batch)
        assert list(got) == dm.greedy_completion(V) and len(got) == N - s
        assert s == 0 or got.primes == [du.PMAX]
        seen.add(tuple(got) == tuple(range(s, N)))
    assert seen == {True, False}                                        # not always the last N - s vectors


def test_complete_basis_takes_the_next_prime_and_refuses_dependent_columns():
    V = [[1, 1], [0, du.PMAX], [0, 0]]                                  # the columns agree mod the first prime of the schedule
    got = rounding.complete_basis(V, batch=mu.host_batch)
    assert list(got) == [2] and got.primes == [du.PMAX, rounding.prev_prime(du.PMAX)] and got.p == got.primes[1]
    with pytest.raises(ValueError):
        rounding.complete_basis(V, maxprimes=1, batch=mu.host_batch)
    with pytest.raises(ValueError):
        rounding.complete_basis([[1, 2], [2, 4], [3, 6]], batch=mu.host_batch)
    with pytest.raises(ValueError):
        rounding.complete_basis([[1, 2, 3]], batch=mu.host_batch)
    assert list(rounding.complete_basis(np.zeros((3, 0), dtype=object), batch=mu.host_batch)) == [0, 1, 2]


# ---- basis_transformations -------------------------------------------------------------------------------------------------------------------------------------
def delsarte_kernels(branch="dual"):
    """the kernel of problems.delsarte_exact(8, 3, 1/2) as kernel_vectors(..., rationalize=True) rounds it on the host from the 320-bit oracle's solution
    (tests/golden/delsarte_exact_kernel.json, recorded from tests/test_rationalize_cpu.py's run): {block index: (N, vectors)}"""
    with open(os.path.join(ROOT, "tests", "golden", "delsarte_exact_kernel.json")) as fh:
        blocks = json.load(fh)[branch]
    return {i: (b["N"], [[F(n, d) for n, d in vec] for vec in b["vectors"]]) for i, b in enumerate(blocks)}


HAND_MADE = {
    "fractions": (4, [[F(1, 2), F(1, 3), F(0), F(1)], [F(0), F(2, 5), F(1), F(-1, 7)]]),
    "zero rows": (5, [[F(0), F(3), F(0), F(1, 4), F(0)]]),
    "full": (2, [[F(1), F(1)], [F(1), F(-1)]]),
    "none": (3, []),
}


@pytest.mark.parametrize("kernels", (HAND_MADE, "dual", "primal"))
def test_basis_transformations(kernels):
    kernels = delsarte_kernels(kernels) if isinstance(kernels, str) else kernels
    plain = rounding.basis_transformations(kernels, PLAIN, **HOOKS)
    norm = rounding.basis_transformations(kernels, UNREDUCED, **HOOKS)
    assert list(plain) == list(norm) == list(kernels)
    for key, (N, vectors) in kernels.items():
        Bt, Binv, s = plain[key]
        assert s == len(vectors) and Bt.shape == Binv.shape == (N, N)
        assert dm.frac_matmul(Bt.T, Binv) == dm.identity(N)
        assert [list(Bt[c]) for c in range(s)] == [list(v) for v in vectors]            # the kernel vectors are the first s columns of B
        extra = dm.greedy_completion(np.array(vectors, dtype=object).reshape(s, N).T)
        assert [list(Bt[s + c]) for c in range(N - s)] == [[F(int(r == i)) for r in range(N)] for i in extra]
        Btn, Binvn, sn = norm[key]
        assert sn == s and all(v.denominator == 1 for v in Binvn.flat)
        assert dm.frac_matmul(Btn.T, Binvn) == dm.identity(N)
        for i in range(N):                                                                # row i of Binv times the lcm of its denominators, no more
            lcm = 1
            for v in Binv[i]:
                lcm = lcm * v.denominator // np.gcd(lcm, v.denominator)
            assert list(Binvn[i]) == [v * int(lcm) for v in Binv[i]] and list(Btn[i]) == [v / int(lcm) for v in Bt[i]]
        if s == 0:
            assert dm.frac_matmul(Bt, dm.identity(N)) == dm.identity(N) and [list(r) for r in Binv] == dm.identity(N)
    if "none" in kernels:
        assert plain["none"][2] == 0 and plain["full"][2] == 2


def test_basis_transformations_refuses_the_reduction_it_does_not_have():
    for settings in (None, rounding.RoundingSettings()):
        with pytest.raises(NotImplementedError, match="reduce_kernelvectors.*(HNF|LLL)"):
            rounding.basis_transformations(HAND_MADE, settings, **HOOKS)
    s = rounding.RoundingSettings()
    assert s.reduce_kernelvectors is True and s.normalize_transformation is True
    with pytest.raises(ValueError):
        rounding.basis_transformations({"a": (3, [[F(1), F(2)]])}, UNREDUCED, **HOOKS)


def test_basis_transformations_passes_its_hooks_down():
    mm, rec, lift, batch = dm.Counting(dm.host_matmul), dm.Counting(dm.host_reconstruct), dm.Counting(dm.lift_columns), dm.Counting(mu.host_batch)
    out = rounding.basis_transformations(HAND_MADE, UNREDUCED, batch=batch, lift=lift, reconstruct=rec, matmul=mm)
    want = rounding.basis_transformations(HAND_MADE, UNREDUCED, **HOOKS)
    assert all(np.array_equal(out[k][i], want[k][i]) for k in want for i in (0, 1)) and all(out[k][2] == want[k][2] for k in want)
    assert batch.calls == 3 and lift.calls == 3 and rec.calls == 3 and mm.calls == 6       # three blocks have vectors


# ---- transform / undo_transform -----------------------------------------------------------------------------------------------------------------------------
def _symmetric(rng, N):
    M = np.array([[F(int(rng.integers(-9, 10)), int(rng.integers(1, 6))) for _ in range(N)] for _ in range(N)], dtype=object)
    return np.array([[M[min(i, j), max(i, j)] for j in range(N)] for i in range(N)], dtype=object)


@pytest.mark.parametrize("matmul", (None, dm.host_matmul))
def test_transform_and_undo_transform(matmul):
    rng = np.random.default_rng(60)
    Bt, Binv, s = rounding.basis_transformations(HAND_MADE, UNREDUCED, **HOOKS)["fractions"]
    N = 4
    M = _symmetric(rng, N)
    # s = 0: transform is the congruence by Binv, and undoing it with the inverse of Binv^T gives M back
    T0 = rounding.transform(M, Binv, 0, matmul=matmul)
    assert [list(r) for r in T0] == [[sum(Binv[i, a] * M[a, b] * Binv[j, b] for a in range(N) for b in range(N)) for j in range(N)] for i in range(N)]
    back = rounding.undo_transform(T0, rounding.inverse_qq(Binv.T, lift=dm.lift_columns), 0, matmul=matmul)
    assert [list(r) for r in back] == [list(r) for r in M]
    # s > 0: the lower right (N - s) block of the congruence, by a triple loop
    assert s == 2
    T = rounding.transform(M, Binv, s, matmul=matmul)
    assert T.shape == (N - s, N - s)
    assert [list(r) for r in T] == [[sum(Binv[s + i, a] * M[a, b] * Binv[s + j, b] for a in range(N) for b in range(N)) for j in range(N - s)] for i in range(N - s)]
    # undo_transform pads with s zero rows and columns and multiplies by Binv^T and Binv
    Mt = _symmetric(rng, N - s)
    U = rounding.undo_transform(Mt, Binv, s, matmul=matmul)
    assert [list(r) for r in U] == [[sum(Binv[s + a, i] * Mt[a, b] * Binv[s + b, j] for a in range(N - s) for b in range(N - s)) for j in range(N)] for i in range(N)]
    # a matrix that lives on the complement of the kernel goes there and back: M = Binv^T [0 0; 0 Mt] Binv has the kernel vectors in its kernel
    assert all(sum(U[i, a] * Bt[c, a] for a in range(N)) == 0 for i in range(N) for c in range(s))
    with pytest.raises(ValueError):
        rounding.transform(M, Binv, 5)
    with pytest.raises(ValueError):
        rounding.undo_transform(M, Binv, 2)
    if matmul is not None:
        mm = dm.Counting(matmul)
        rounding.transform(M, Binv, s, matmul=mm)
        assert mm.calls == 2


# ---- the binding and the refusals ----------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32, "double *": _lib.p_d}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_dixon_lift_multi\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "n", "m", "p", "nd", "A_digits", "nbl", "B_limbs", "steps", "X", "R_limbs", "info"]
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_dixon_lift_multi"] == (C.c_int, [table[re.sub(r"\w+$", "", a).strip()] for a in args])
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_dixon_lift_multi_times\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_dixon_lift_multi_times"] == (C.c_int, [table[re.sub(r"\w+$", "", a.strip()).strip()] for a in args.split(",")])
    L = _lib.load()
    assert hasattr(L, "clrs_modp_dixon_lift_multi") and hasattr(L, "clrs_modp_dixon_lift_multi_times")
    assert L.clrs_config_set(b"liftm_chunk_bytes", 4096) == 0 and L.clrs_config_set(b"liftm_chunk_bytes", 0) == 0
    for name in ("dixon_lift_multi", "solve_dixon_multi", "DixonSolutionMatrix", "inverse_qq", "complete_basis", "basis_transformations", "transform",
                 "undo_transform"):
        assert name in rounding.__all__ and hasattr(rounding, name)
    assert "clrs_modp_dixon_lift_multi" in rounding.__doc__ and "basis_transformations" in rounding.__doc__


def test_refusals_need_no_device():
    """what clrs_modp_dixon_lift_multi refuses, it refuses before it touches a device, and it writes nothing"""
    L = _lib.load()
    pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)
    A = np.array([[[2, 3], [3, 10]]], np.int32)
    B = np.array([[[1, 1, 0], [1, 0, 1]]], np.int32)
    X, R, info = (np.full(s, dm.SENTINEL, np.int32) for s in ((3, 2, 3), (3, 2, 3), (6,)))
    call = lambda n=2, m=3, p=13, nd=1, A=A, nbl=1, B=B, steps=3, X=X, R=R, info=info: L.clrs_modp_dixon_lift_multi(0, n, m, p, nd, pi(A), nbl, pi(B), steps, pi(X),
                                                                                                               pi(R), pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9, -7):
        assert call(p=p) == -1
    assert call(n=-1) == -1 and call(n=32768) == -1 and call(m=-1) == -1
    assert call(nd=0) == -1 and call(nbl=0) == -1 and call(steps=-1) == -1 and call(nd=32768) == -1 and call(nbl=32768) == -1
    assert call(A=np.array([[[2, 3], [3, 2 ** 23]]], np.int32)) == -1
    assert call(A=np.array([[[2, 3], [3, -2 ** 23 - 1]]], np.int32)) == -1
    assert call(B=np.array([[[1, 1, 0], [1, 0, 2 ** 23]]], np.int32)) == -1
    assert call(A=None) == -1 and call(B=None) == -1 and call(X=None) == -1 and call(R=None) == -1 and call(info=None) == -1
    assert b"null" in L.clrs_last_error()
    # 2^31 elements or more: of A (nd n^2), of B (nbl n m), of X (steps n m), of R ((nrl + 1) n m); the sizes are tested before any array is read
    assert call(n=32767, nd=3) == -1 and b"2^31" in L.clrs_last_error()
    assert call(n=2, m=2 ** 30) == -1 and call(n=2, m=2 ** 28, steps=4) == -1 and call(n=2, m=2 ** 28, steps=0, nbl=2) == -1
    assert all(int(v) == dm.SENTINEL for a in (X, R, info) for v in a.flat)
    # n = 0 or m = 0: zeros, no device
    assert L.clrs_modp_dixon_lift_multi(0, 0, 3, 13, 1, None, 1, None, 3, None, None, pi(info)) == 0 and info.tolist() == [0, 3, 0, 0, 0, 0]
    info[:] = dm.SENTINEL
    assert call(m=0) == 0 and info.tolist() == [0, 3, 0, 0, 0, 0] and all(int(v) == dm.SENTINEL for a in (X, R) for v in a.flat)
    t = [C.c_double(-1.0) for _ in range(4)]
    assert L.clrs_modp_dixon_lift_multi_times(*[C.byref(v) for v in t]) == 0 and [v.value for v in t] == [0.0] * 4
    assert L.clrs_modp_dixon_lift_multi_times(None, None, None, None) == -1
    # the Python front end refuses on its own
    with pytest.raises(ValueError):
        rounding.dixon_lift_multi([[2, 3], [3, 10]], [[1], [1]], 4, 3)
    with pytest.raises(ValueError):
        rounding.dixon_lift_multi([[2, 3, 4], [3, 10, 4]], [[1], [1]], 13, 3)
    with pytest.raises(ValueError):
        rounding.dixon_lift_multi([[2, 3], [3, 10]], [1, 1], 13, 3)
    X0, R0, rank = rounding.dixon_lift_multi([[2, 3], [3, 10]], np.zeros((2, 0), dtype=np.int64), 13, 3)
    assert X0.shape == (3, 2, 0) and R0.shape == (2, 0) and rank == 2


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    if torch.cuda.is_available():
        assert [list(r) for r in rounding.inverse_qq([[2, 3], [3, 10]])] == [[F(10, 11), F(-3, 11)], [F(-3, 11), F(2, 11)]]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.inverse_qq([[2, 3], [3, 10]])

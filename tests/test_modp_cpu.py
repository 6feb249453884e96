"""CPU side of the pivots of integer systems by RREF mod p (clrs_modp_rref, clrs_amd.rounding): the restatement against a hand example
and the invariants of a reduced row-echelon form, the scalar arithmetic of csrc/clrs_modp_arith.h compiled for the host against Python integers, the Python
layer with the restatement as a stand-in for the device call (the package has no CPU implementation of it), and the binding of the symbol."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import modp_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_on_a_hand_example():
    """mod 7: rows (1 2 3), (2 4 0), (3 6 3).  Column 1 is twice column 0; row 1 - 2 row 0 = (0 0 1), so the form is (1 2 0), (0 0 1), (0 0 0)."""
    piv, rank, R = mu.rref_mod_p([[1, 2, 3], [2, 4, 0], [3, 6, 3]], 7)
    assert list(piv) == [0, 2] and rank == 2
    assert R.tolist() == [[1, 2, 0], [0, 0, 1], [0, 0, 0]]
    # an exchange: the first column's only non-zero is in the last row
    piv, rank, R = mu.rref_mod_p([[0, 1], [0, 3], [5, 1]], 7)
    assert list(piv) == [0, 1] and rank == 2 and R.tolist() == [[1, 0], [0, 1], [0, 0]]


@pytest.mark.parametrize("p", mu.PRIMES)
def test_restatement_meets_the_invariants(p):
    rng = np.random.default_rng(p)
    for A in (mu.random_matrix(rng, 17, 33, p), mu.random_matrix(rng, 33, 17, p), mu.planted(rng, 12, 20, [2, 3, 9], p, zero_cols=[0, 1]),
              np.zeros((4, 5), np.int64)):
        piv, rank, R = mu.rref_mod_p(A, p)
        mu.check_invariants(R, piv, rank, p)
    piv, rank, _ = mu.rref_mod_p(mu.planted(rng, 12, 20, [2, 3, 9], p, zero_cols=[0, 1]), p)
    assert list(piv) == [2, 3, 9]


# ---- the host build of clrs_modp_arith.h ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (2, 3, 10007, 8388593))
def test_host_reduction_against_python_integers(p):
    top = 32 * (p - 1) ** 2 + (p - 1)
    assert top < 2 ** 53
    rng = np.random.default_rng(p)
    xs = [0, p - 1, p, (p - 1) ** 2, top] + [int(v) for v in rng.integers(0, top + 1, size=10 ** 4, dtype=np.int64)]
    assert mu.host_reduce(p, xs) == [x % p for x in xs]
    a = [int(v) for v in rng.integers(0, p, size=10 ** 4)] + [p - 1, 0]
    b = [int(v) for v in rng.integers(0, p, size=10 ** 4)] + [p - 1, p - 1]
    assert mu.host_mul(p, a, b) == [x * y % p for x, y in zip(a, b)]


@pytest.mark.parametrize("p", (2, 3, 10007, 8388593))
def test_host_inverses_against_python_integers(p):
    rng = np.random.default_rng(p + 1)
    xs = list(range(1, p)) if p < 10 else [1, p - 1] + [int(v) for v in rng.integers(1, p, size=10 ** 4)]
    inv = mu.host_inv(p, xs)
    assert inv == [pow(x, -1, p) for x in xs]
    assert all(0 < v < p for v in inv)


def test_host_primality():
    L = mu.host_lib()

    def is_prime(n):
        return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))
    assert [bool(L.modp_is_prime_host(n)) for n in range(-3, 3000)] == [is_prime(n) for n in range(-3, 3000)]
    # 8388593 is the largest prime below 2^23; 8388591 = 3 * 2796197, 8388607 = 2^23 - 1 = 47 * 178481
    assert [L.modp_is_prime_host(n) for n in (8388591, 8388593, 8388607)] == [0, 1, 0]
    assert 8388591 % 3 == 0 and 8388607 == 47 * 178481 and is_prime(8388593) and not any(is_prime(n) for n in range(8388594, 2 ** 23))


# ---- the Python layer, the restatement as the device call --------------------------------------------------------------------------------------------------
def test_next_prime():
    assert [rounding.next_prime(x) for x in (0, 1, 2, 10, 11, 10 ** 4)] == [2, 2, 3, 11, 13, 10007]
    assert rounding.next_prime(-5) == 2


def test_schedule_of_primes_on_the_two_by_two():
    """max |A| = 10, so the first prime is 11; det = 11: mod 11 the pivots are [0], mod 13 they are [0, 1]"""
    A = [[2, 3], [3, 10]]
    assert list(mu.rref_mod_p(A, 11)[0]) == [0] and list(mu.rref_mod_p(A, 13)[0]) == [0, 1]
    piv = rounding.find_pivots_modular(A, batch=mu.host_batch)
    assert list(piv) == [0, 1] and piv.primes == [11, 13] and piv.p == 13
    one = rounding.find_pivots_modular(A, maxprimes=1, batch=mu.host_batch)
    assert list(one) == [0] and one.primes == [11] and one.p == 11


def test_three_rows_two_columns_runs_every_round():
    A = [[1, 2], [3, 4], [5, 6]]                         # max 6: primes 7, 11, 13; rank 2 at each
    piv = rounding.find_pivots_modular(A, batch=mu.host_batch)
    assert list(piv) == [0, 1] and piv.primes == [7, 11, 13] and piv.p == 7
    # the FIRST of the longest lists: det (2 3; 3 10) = 11, so the first round is the short one and the second is returned
    B = [[2, 3], [3, 10], [4, 6]]
    piv = rounding.find_pivots_modular(B, batch=mu.host_batch)
    assert list(piv) == [0, 1] and piv.primes == [11, 13, 17] and piv.p == 13
    five = rounding.find_pivots_modular(A, maxprimes=5, batch=mu.host_batch)
    assert five.primes == [7, 11, 13, 17, 19]
    with pytest.raises(ValueError):
        rounding.find_pivots_modular(A, maxprimes=0, batch=mu.host_batch)


def test_zero_and_empty_matrices():
    piv = rounding.find_pivots_modular(np.zeros((3, 4), int), batch=mu.host_batch)
    assert list(piv) == [] and piv.primes == [2, 3, 5] and piv.p == 2
    for empty in ([], np.zeros((0, 5), int), np.zeros((5, 0), int)):
        piv = rounding.find_pivots_modular(empty, batch=mu.host_batch)
        assert list(piv) == [] and piv.primes == []


def test_large_integers_are_reduced_on_the_host():
    big = 10 ** 30
    A = [[big + 1, big + 2, 3], [2 * big + 2, 2 * big + 4, 7], [5, 7, big]]
    piv = rounding.find_pivots_modular(A, batch=mu.host_batch)
    assert piv.primes[0] == 10007                         # min(max |A|, 10^4) = 10^4
    assert list(piv) == [0, 1, 2]
    res = rounding._residues(rounding._integer_matrix(A, "test"), 10007)
    assert res.dtype == np.int32 and res.tolist() == [[v % 10007 for v in row] for row in A]
    neg = rounding._residues(rounding._integer_matrix([[-1, -big]], "test"), 10007)
    assert neg.tolist() == [[10006, (-big) % 10007]]
    with pytest.raises(ValueError):
        rounding.find_pivots_modular([[0.5, 1]], batch=mu.host_batch)


def test_system_pivots():
    A, b = mu.example_system()
    piv, rows, ok = rounding.system_pivots(A, b, batch=mu.host_batch)
    assert ok and list(piv) == [0, 1] and list(rows) == [0, 1]
    assert len(piv.primes) == 3 and piv.primes[0] == rounding.next_prime(840)   # three rows, rank two: every round runs; the largest cleared entry is 2 * 420
    b2 = list(b)
    b2[2] += Fraction(1, 3)
    piv, rows, ok = rounding.system_pivots(A, b2, batch=mu.host_batch)
    assert not ok and piv[-1] == 5 and list(piv) == [0, 1, 5] and list(rows) == [0, 1, 2]
    piv, rows, ok = rounding.system_pivots(np.zeros((3, 5), int), np.zeros(3, int), batch=mu.host_batch)
    assert ok and list(piv) == [] and list(rows) == []
    # integers and a column vector for b
    piv, rows, ok = rounding.system_pivots([[1, 2], [2, 4]], [[3], [6]], batch=mu.host_batch)
    assert ok and list(piv) == [0] and list(rows) == [0]


# ---- the binding -----------------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbol_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_rref\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "nrows", "ncols", "p", "A", "pivots", "rank", "R"]
    want = [table[re.sub(r"\w+$", "", a).strip()] for a in args]
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_rref"] == (C.c_int, want)
    assert hasattr(_lib.load(), "clrs_modp_rref")
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    assert jl.count(":clrs_modp_rref") == 1 and "function find_pivots_modular(A::AbstractMatrix{<:Integer}, p::Integer" in jl
    assert "function find_pivots_modular(A::AbstractMatrix{<:Integer}; maxprimes" in jl
    for name in ("rref_mod_p", "next_prime", "find_pivots_modular", "system_pivots"):
        assert name in rounding.__all__


def test_refusals_need_no_device():
    """what clrs_modp_rref refuses, it refuses before it touches a device"""
    L = _lib.load()
    A = np.array([[1, 2], [3, 4]], np.int32)
    piv, rank = np.full(2, mu.SENTINEL, np.int32), np.full(1, mu.SENTINEL, np.int32)
    pi = lambda a: a.ctypes.data_as(_lib.p_i32)
    for p in (1, 4, 10005, 2 ** 23 + 9, -7):
        assert L.clrs_modp_rref(0, 2, 2, p, pi(A), pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, -1, 2, 7, pi(A), pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 2, -1, 7, pi(A), pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 65536, 32768, 7, pi(A), pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 2, 2, 3, pi(A), pi(piv), pi(rank), None) == -1            # 3 and 4 are no residues mod 3
    assert L.clrs_modp_rref(0, 2, 2, 7, pi(np.array([[1, -2], [3, 4]], np.int32)), pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 2, 2, 7, pi(A), None, pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 2, 2, 7, None, pi(piv), pi(rank), None) == -1
    assert L.clrs_modp_rref(0, 2, 2, 7, pi(A), pi(piv), None, None) == -1
    assert list(piv) == [mu.SENTINEL] * 2 and rank[0] == mu.SENTINEL
    # an empty matrix: rank 0, no device
    assert L.clrs_modp_rref(0, 0, 5, 7, None, None, pi(rank), None) == 0 and rank[0] == 0
    with pytest.raises(ValueError):
        rounding.rref_mod_p(A, 4)


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    A = [[2, 3], [3, 10]]
    if torch.cuda.is_available():
        piv, rank = rounding.rref_mod_p(A, 13)
        assert list(piv) == [0, 1] and rank == 2
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.rref_mod_p(A, 13)

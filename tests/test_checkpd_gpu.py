"""The leading minors mod many primes on the device (clrs_modp_minors: k_minors_residues, k_minors_ldl) against Bareiss' exact minors
on Python integers and the per-prime restatement of tests/pd_util.py, with `==`: block sizes at every tile and mask boundary, primes where breakdowns are
the rule, prime counts beyond the compute units and beyond one chunk, digit counts, extreme digits, the refusals, and rounding.checkpd on the device against
the host stand-in."""
import functools

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import pd_util as pu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
THREE = (pu.PMAX, 10007, 2)


@functools.lru_cache(maxsize=None)
def case(kind, n, bits, seed=0):
    """(matrix, exact minors), computed once"""
    M = pu.random_spd(100 + n + seed, n, bits) if kind == "spd" else pu.random_symmetric(200 + n + seed, n, bits)
    return M, pu.bareiss_minors(M)


def check_raw(M, exact, primes, chunk_bytes=0, digits=None):
    """one raw call on sentinel-filled outputs against both oracles; returns (breakdown, info)"""
    n = len(M)
    code, minors, brk, info = pu.device_minors(M, primes, chunk_bytes=chunk_bytes, digits=digits)
    assert code == 0, _lib.load().clrs_last_error()
    npad = (n + 15) // 16 * 16
    assert info[0] == npad * (npad + 1 + 17) * 8 and info[1] == len(primes) and info[3] == 0
    for q, p in enumerate(primes):
        row, k = pu.minors_mod_np(M, int(p))
        assert int(brk[q]) == k and minors[q].tolist() == row, (n, p)                 # the restatement: residues, the breakdown, -1 behind it
        valid = n if k == 0 else k
        assert row[:valid] == [v % int(p) for v in exact[:valid]]                      # and the exact minors at every valid position
        assert all(v == -1 for v in minors[q, valid:])
    assert info[2] == int(np.count_nonzero(brk))
    return brk, info


@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 31, 32, 33, 64, 65))
def test_block_sizes_at_the_tile_and_mask_boundaries(n):
    M, exact = case("spd", n, 40)                                   # two digits; positive definite: breakdowns are rare at the large prime
    brk, _ = check_raw(M, exact, THREE)
    assert brk[0] == 0 and all(v > 0 for v in exact)
    S, sexact = case("sym", n, 3)                                   # small indefinite entries: breakdowns are the rule at 2 and common at 10007
    check_raw(S, sexact, THREE)


def test_128_rows_with_one_digit_entries():
    M, exact = case("sym", 128, 20)
    for i in range(128):
        assert abs(M[i][i]) < 1 << 22
    assert rounding.to_balanced_digits(np.asarray(M, dtype=object)).shape[0] == 1
    brk, info = check_raw(M, exact, THREE)
    assert info[0] == 128 * (129 + 17) * 8 and brk[0] == 0


@pytest.mark.parametrize("nprimes", (1, 2, 65))
def test_prime_counts(nprimes):
    M, exact = case("spd", 17, 40)
    primes = [int(p) for p in rounding._primes_descending()[:nprimes]]
    check_raw(M, exact, primes)


def test_more_primes_than_compute_units_and_more_than_one_chunk():
    M, exact = case("spd", 33, 40)
    primes = [int(p) for p in rounding._primes_descending()[:298]] + [10007, 2]
    _, info = check_raw(M, exact, primes)                           # one chunk, 300 workgroups
    assert info[1] == 300
    _, info = check_raw(M, exact, primes, chunk_bytes=64 * 33 * 33 * 8)               # 64 primes per chunk: five chunks, the last of 44
    assert info[1] == 300
    check_raw(M, exact, primes, chunk_bytes=1)                      # a bound below one matrix: one prime per chunk


@pytest.mark.parametrize("nd,bits", ((1, 20), (2, 40), (3, 60), (70, 1670)))
def test_digit_counts(nd, bits):
    M, exact = case("sym", 18, bits)
    M = [row[:] for row in M]
    M[3][3] = (1 << bits) - 1                                       # the full digit count whatever the random entries are
    exact = pu.bareiss_minors(M)
    assert rounding.to_balanced_digits(np.asarray(M, dtype=object)).shape[0] == nd
    check_raw(M, exact, THREE + (8388587,))


def test_extreme_digits():
    """digits at both ends of [-2^23, 2^23], the upper end included (to_balanced_digits never produces it; the C function takes it)"""
    rng = np.random.default_rng(9)
    n, nd, top = 19, 3, 1 << 23
    planes = np.zeros((nd, n, n), np.int64)
    for l in range(nd):
        t = rng.choice([-top, top, 0, top - 1, -top + 1, 12345], size=(n, n))
        planes[l] = np.tril(t) + np.tril(t, -1).T
    planes[nd - 1][np.diag_indices(n)] = top
    M = [[int(v) for v in row] for row in rounding.from_balanced_digits(planes)]
    check_raw(M, pu.bareiss_minors(M), THREE, digits=planes.astype(np.int32))
    allmax = np.full((2, 16, 16), top, np.int32)                    # every digit 2^23: rank one, minor 2 is zero mod every prime
    M = [[int(v) for v in row] for row in rounding.from_balanced_digits(allmax)]
    brk, _ = check_raw(M, pu.bareiss_minors(M), THREE, digits=allmax)
    assert brk.tolist() == [2, 2, 1]


def test_python_front_end_is_the_raw_call():
    M, exact = case("spd", 17, 40)
    minors, brk = rounding.leading_minors_mod(M, THREE)
    assert minors.dtype == np.int32 and minors.shape == (3, 17) and brk.shape == (3,)
    for q, p in enumerate(THREE):
        row, k = pu.minors_mod_np(M, p)
        assert minors[q].tolist() == row and int(brk[q]) == k
    assert rounding.leading_minors_mod.last_info[1] == 3 and rounding.leading_minors_mod.last_info[3] == 0
    import ctypes as C
    a, b, c = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
    assert _lib.load().clrs_modp_minors_times(C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value >= 0.0 and b.value >= 0.0 and c.value >= a.value + b.value > 0.0


@pytest.mark.parametrize("name", pu.PLANTED)
def test_planted_matrices_on_the_device_equal_the_stand_in(name):
    A, pd, order = pu.planted(name)
    dev, host = rounding.checkpd(A), rounding.checkpd(A, minors=pu.host_minors)
    assert dev == host and dev.pd == pd and (order is None or dev.failed_order == order)


def test_is_valid_solution_on_the_device():
    good, bad = pu.random_spd(1, 20, 100), pu.planted("negative minor 9 of 20")[0]
    assert rounding.is_valid_solution([good, pu.hilbert(20)], check_slacks=False) == (True, [])
    assert rounding.is_valid_solution([good, bad], [[1, 2]], [5], [1, 2]) == (False, [("block", 1, 9)])


def test_refusals_leave_the_library_working():
    L = _lib.load()
    M, exact = case("spd", 2, 40)
    digits = rounding.to_balanced_digits(np.asarray(M, dtype=object))
    minors, brk, info = np.full((3, 2), pu.SENTINEL, np.int32), np.full(3, pu.SENTINEL, np.int32), np.full(4, pu.SENTINEL, np.int32)
    big = np.zeros((1, 129, 129), np.int32)
    pr = np.array(THREE, np.int32)
    assert L.clrs_modp_minors(0, 129, 1, pu._pi(big), 3, pu._pi(pr), pu._pi(minors), pu._pi(brk), pu._pi(info)) == INVALID
    rep = np.array([10007, 2, 10007], np.int32)
    assert L.clrs_modp_minors(0, 2, digits.shape[0], pu._pi(digits), 3, pu._pi(rep), pu._pi(minors), pu._pi(brk), pu._pi(info)) == INVALID
    assert all(int(v) == pu.SENTINEL for a in (minors, brk, info) for v in a.flat)
    check_raw(M, exact, THREE)

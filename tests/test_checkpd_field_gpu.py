"""The leading minors of a matrix over a number field mod split primes on the device (clrs_modp_minors_field: k_minors_residues_field, k_minors_ldl;
clrs_modp_field_frobenius: k_field_frobenius) against the per-pair restatement of tests/pd_field_util.py with `==` on sentinel-filled
outputs: block sizes at the tile boundaries, every degree, digit counts and extreme digits, prime counts past a wave's 4 x 64 and past one chunk, the
one-pair breakdown, the Frobenius kernel against the host's, the refusals, and rounding.checkpd_field on the device against the host stand-ins."""
import ctypes as C
import functools

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import pd_field_util as fu
from tests import pd_util as pu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID


def points(seed, primes, d):
    """d distinct points in [0, p) per prime, 0 and p - 1 among them where they fit: the raw call takes any distinct points"""
    rng = np.random.default_rng(seed)
    out = []
    for p in primes:
        rr = {0, p - 1} if d >= 3 else {p - 1}
        while len(rr) < d:
            rr.add(int(rng.integers(0, p)))
        out.append(sorted(rr)[:d])
    return out


def restate(mats, primes, roots):
    """per pair (row, breakdown) by the restatement of tests/pd_util.py on M(r) mod p"""
    return [[pu.minors_mod_np(fu.evaluate_mod(mats, int(r), int(p)), int(p)) for r in rr] for p, rr in zip(primes, roots)]


def check_raw(mats, primes, roots, chunk_bytes=0, digits=None, want=None):
    """one raw call on sentinel-filled outputs against the restatement (`want`: computed before), pair by pair; returns (breakdown, info)"""
    d, n = len(mats), len(mats[0])
    want = restate(mats, primes, roots) if want is None else want
    code, minors, brk, info = fu.device_field_minors(mats, primes, roots, chunk_bytes=chunk_bytes, digits=digits)
    assert code == 0, _lib.load().clrs_last_error()
    npad = (n + 15) // 16 * 16
    assert info[0] == npad * (npad + 1 + 17) * 8 and info[1] == len(primes) * d and info[3] == 0
    for q, p in enumerate(primes):
        for i, r in enumerate(roots[q]):
            row, k = want[q][i]
            assert int(brk[q, i]) == k and minors[q, i].tolist() == row, (n, d, p, r)
    assert info[2] == int(np.count_nonzero(brk))
    return brk, info


@functools.lru_cache(maxsize=None)
def mats_of(d, n, bits, seed=0):
    return fu.random_coefficient_matrices(500 + seed, d, n, bits)


@pytest.mark.parametrize("deg", (2, 3, 4))
@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_block_sizes_and_degrees(n, deg):
    primes = [pu.PMAX, 10007, 5]                                     # at 5 breakdowns are the rule
    check_raw(mats_of(deg, n, 40), primes, points(n, primes, deg))  # two digits
    check_raw(mats_of(deg, n, 3), primes, points(n + 1, primes, deg))


def test_128_rows_with_one_digit_entries():
    mats = mats_of(2, 128, 20)
    digits = np.swapaxes(rounding.to_balanced_digits(np.array(mats, dtype=object)), 0, 1)
    assert digits.shape == (2, 1, 128, 128)
    primes = [pu.PMAX, 10007]
    _, info = check_raw(mats, primes, points(1, primes, 2))
    assert info[0] == 128 * (129 + 17) * 8


@pytest.mark.parametrize("deg", (2, 3, 4))
def test_true_roots_give_the_images_of_the_exact_minors(deg):
    """at the roots of the minimal polynomial the residues are the images of the minors in Z[g] (Bareiss in the ring), not just the minors of some matrix"""
    name = {2: "x2-2", 3: "x3-2", 4: "x4-x-1"}[deg]
    fld, A, _, _ = fu.planted("gram " + name)
    scale, lc, M = fu.normal_form(fld, A)
    mats = [[[int(e[c]) for e in row] for row in M] for c in range(deg)]
    primes, roots = rounding.split_primes(fld, 2)
    exact = [fu.to_h_coordinates(lc, m) for m in fu.bareiss_minors_field(fld.minpoly, M)]
    minors, brk = rounding.leading_minors_field_mod(mats, primes, roots)
    assert minors.shape == (2, deg, len(A)) and brk.tolist() == [[0] * deg] * 2
    for q, p in enumerate(primes):
        for i, r in enumerate(roots[q]):
            assert minors[q, i].tolist() == [sum(c * pow(r, j, p) for j, c in enumerate(m)) % p for m in exact]
    assert rounding.leading_minors_field_mod.last_info[1] == 2 * deg and rounding.leading_minors_field_mod.last_info[3] == 0
    a, b, c = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
    assert _lib.load().clrs_modp_minors_field_times(C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value >= 0.0 and b.value >= 0.0 and c.value >= a.value + b.value > 0.0


@pytest.mark.parametrize("nd,bits", ((1, 20), (3, 60), (70, 1670)))
def test_digit_counts(nd, bits):
    mats = [[row[:] for row in M] for M in mats_of(3, 18, bits)]
    mats[1][3][3] = (1 << bits) - 1                                  # the full digit count whatever the random entries are
    assert rounding.to_balanced_digits(np.array(mats, dtype=object)).shape[0] == nd
    primes = [pu.PMAX, 8388587, 10007, 5]
    check_raw(mats, primes, points(nd, primes, 3))


def test_extreme_digits():
    """digits at both ends of [-2^23, 2^23], the upper end included (to_balanced_digits never produces it; the C function takes it)"""
    rng = np.random.default_rng(9)
    d, n, nd, top = 4, 19, 3, 1 << 23
    planes = np.zeros((d, nd, n, n), np.int64)
    for c in range(d):
        for l in range(nd):
            t = rng.choice([-top, top, 0, top - 1, -top + 1, 12345], size=(n, n))
            planes[c, l] = np.tril(t) + np.tril(t, -1).T
    planes[:, nd - 1][:, np.arange(n), np.arange(n)] = top
    mats = [[[int(v) for v in row] for row in rounding.from_balanced_digits(planes[c])] for c in range(d)]
    primes = [pu.PMAX, 10007, 5]
    check_raw(mats, primes, points(3, primes, d), digits=planes.astype(np.int32))
    allmax = np.full((2, 2, 16, 16), top, np.int32)                  # every digit 2^23: every residue matrix has rank one at most
    mats = [[[int(v) for v in row] for row in rounding.from_balanced_digits(allmax[c])] for c in range(2)]
    brk, _ = check_raw(mats, primes, points(4, primes, 2), digits=allmax)
    assert np.all((brk == 1) | (brk == 2))


@pytest.mark.parametrize("nprimes", (1, 257))
def test_prime_counts(nprimes):
    """one prime, and one past the 4 x 64 primes of a wave: a second row of the grid with one live lane"""
    primes = [int(p) for p in rounding._primes_descending()[:nprimes]]
    check_raw(mats_of(2, 17, 40), primes, points(nprimes, primes, 2))
    if nprimes == 257:
        check_raw(mats_of(4, 5, 40), primes, points(7, primes, 4))


def test_more_than_one_chunk():
    mats = mats_of(3, 33, 40)
    primes = [int(p) for p in rounding._primes_descending()[:128]] + [10007, 5]
    roots = points(5, primes, 3)
    want = restate(mats, primes, roots)
    _, info = check_raw(mats, primes, roots, want=want)
    assert info[1] == 390
    _, info = check_raw(mats, primes, roots, chunk_bytes=65 * 33 * 33 * 8 * 3, want=want)      # 65 primes (195 matrices) per chunk: two chunks
    assert info[1] == 390
    _, info = check_raw(mats, primes, roots, chunk_bytes=64 * 33 * 33 * 8 * 3 + 7, want=want)  # 64 primes per chunk: three chunks, the last of 2 primes
    assert info[1] == 390
    check_raw(mats, primes[:9], roots[:9], chunk_bytes=1, want=want[:9])              # a bound below one prime's matrices: one prime per chunk


def test_one_pair_breaks_down():
    fld, A, _, _ = fu.planted("one pair breaks down at 5 of 8")
    p, roots = fu.first_split_prime("x2-5")
    _, _, M = fu.normal_form(fld, A)
    mats = [[[int(e[c]) for e in row] for row in M] for c in range(2)]
    second = rounding.split_primes(fld, 2)
    brk, info = check_raw(mats, second[0], second[1])
    assert second[0][0] == p and brk.tolist() == [[5, 0], [0, 0]] and info[2] == 1


@pytest.mark.parametrize("name", fu.FIELDS)
def test_frobenius_on_the_first_4096_primes(name):
    fld = fu.field(name)
    primes = [int(p) for p in rounding._primes_descending()[:4096]]
    got = rounding.field_frobenius(fld.minpoly, primes)
    assert got.dtype == np.int32 and got.shape == (4096, fld.degree) and np.array_equal(got, fu.host_frobenius_many(fld.minpoly, primes))
    for q in (0, 1, 4095):
        assert got[q].tolist() == fu.host_frobenius(fld.minpoly, primes[q])
    small = [2, 3, 5, 7, 11, 13, 10007]                              # 2 divides the leading coefficient of 2x^2 - 5; 5 its discriminant
    assert rounding.field_frobenius(fld.minpoly, small).tolist() == [fu.host_frobenius(fld.minpoly, p) for p in small]


def test_split_primes_on_the_device_equals_the_host_scan():
    for name in ("x2-5", "x4-x-1", "2x2-5"):
        fld = fu.field(name)
        assert rounding.split_primes(fld, 6, frobenius=rounding.field_frobenius) == rounding.split_primes(fld, 6)


@pytest.mark.parametrize("name", fu.PLANTED)
def test_planted_matrices_on_the_device_equal_the_stand_in(name):
    fld, A, pd, order = fu.planted(name)
    host = fu.planted_host_certificate(name)[0]
    dev = rounding.checkpd_field(A, fld)
    assert dev == host and dev.pd == pd and (order is None or dev.failed_order == order)
    if name in ("gram x4-x-1", "one pair breaks down at 5 of 8"):    # the prime scan on the device as well
        assert rounding.checkpd_field(A, fld, primes=functools.partial(rounding.split_primes, frobenius=rounding.field_frobenius)) == host


def test_is_valid_solution_on_the_device():
    fld, good, _, _ = fu.planted("gram x2-5")
    bad = fu.planted("negative minor 9 of 20")[1]
    assert rounding.is_valid_solution([good, bad], check_slacks=False, field=fld) == (False, [("block", 1, 9)])
    assert rounding.is_valid_solution([good], check_slacks=False, field=fld) == (True, [])


def test_refusals_leave_the_library_working():
    L = _lib.load()
    mats = mats_of(2, 2, 40)
    digits = np.ascontiguousarray(np.swapaxes(rounding.to_balanced_digits(np.array(mats, dtype=object)), 0, 1))
    primes = [pu.PMAX, 10007, 5]
    roots = points(1, primes, 2)
    pr, rt = np.array(primes, np.int32), np.array(roots, np.int32)
    minors, brk, info = np.full((3, 2, 2), fu.SENTINEL, np.int32), np.full((3, 2), fu.SENTINEL, np.int32), np.full(4, fu.SENTINEL, np.int32)
    call = lambda n, deg, D, P, R: L.clrs_modp_minors_field(0, n, deg, D.shape[1], fu._pi(D), 3, fu._pi(P), fu._pi(R), fu._pi(minors), fu._pi(brk), fu._pi(info))
    assert call(129, 2, np.zeros((2, 1, 129, 129), np.int32), pr, rt) == INVALID
    assert call(2, 5, digits, pr, rt) == INVALID
    same = rt.copy()
    same[1, 1] = same[1, 0]
    assert call(2, 2, digits, pr, same) == INVALID
    assert call(2, 2, digits, np.array([10007, 5, 10007], np.int32), rt) == INVALID
    assert all(int(v) == fu.SENTINEL for a in (minors, brk, info) for v in a.flat)
    out = np.full((3, 2), fu.SENTINEL, np.int32)
    f = np.array([-5, 0, 1], np.int64)
    assert L.clrs_modp_field_frobenius(0, 2, f.ctypes.data_as(_lib.p_i64), 3, fu._pi(np.array([7, 9, 11], np.int32)), fu._pi(out)) == INVALID
    assert all(int(v) == fu.SENTINEL for v in out.flat)
    check_raw(mats, primes, roots)
    assert rounding.field_frobenius([-5, 0, 1], [11, 7]).tolist() == [[0, 1], [0, 6]]

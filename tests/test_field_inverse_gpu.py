"""The determinant and the adjugate of a matrix over a number field mod split primes on the device (clrs_modp_field_adjugate: k_field_residues_full,
k_field_gj_adjugate) against the per-pair restatement of tests/field_inverse_util.py with `==` on sentinel-filled outputs: block sizes
at the padding boundaries, every degree, digit counts and extreme digits, the pivoting, planted dependent columns, prime counts past a wave's 4 x 64 and
past one chunk, the refusals, the images of the exact adjugate at true roots; and rounding.inverse_field / basis_transformations(field=...) on the device
against the host stand-ins and against inverse_qq on the regular representation."""
import ctypes as C
import functools
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from clrs_amd.rounding import RoundingSettings
from tests import field_inverse_util as iu
from tests import pd_field_util as fu
from tests import pd_util as pu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
PRIMES = [pu.PMAX, 10007, 5]                                         # at 5 singular pairs are the rule


def check_raw(mats, primes, roots, chunk_bytes=0, digits=None, want=None):
    """one raw call on sentinel-filled outputs against the restatement (`want`: computed before), pair by pair; returns (det, breakdown, info)"""
    d, n = len(mats), len(mats[0])
    want = iu.restate(mats, primes, roots) if want is None else want
    code, adj, det, brk, info = iu.device_field_adjugate(mats, primes, roots, chunk_bytes=chunk_bytes, digits=digits)
    assert code == 0, _lib.load().clrs_last_error()
    assert info[0] == iu.lds_bytes(n) and info[1] == len(primes) * d and info[3] == 0
    for q, p in enumerate(primes):
        for i, r in enumerate(roots[q]):
            a, dt, k = want[q][i]
            assert int(brk[q, i]) == k and int(det[q, i]) == dt and np.array_equal(adj[q, i], a), (n, d, p, r)
    assert info[2] == int(np.count_nonzero(brk))
    return det, brk, info


@functools.lru_cache(maxsize=None)
def mats_of(d, n, bits, seed=0):
    return iu.random_square_matrices(700 + seed, d, n, bits)


@pytest.mark.parametrize("deg", (2, 3, 4))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 33))
def test_block_sizes_and_degrees(n, deg):
    check_raw(mats_of(deg, n, 40), PRIMES, iu.points(n, PRIMES, deg))                       # two digits
    check_raw(mats_of(deg, n, 3), PRIMES, iu.points(n + 1, PRIMES, deg))


def test_128_rows_with_one_digit_entries():
    mats = mats_of(2, 128, 20)
    digits = np.swapaxes(rounding.to_balanced_digits(np.array(mats, dtype=object)), 0, 1)
    assert digits.shape == (2, 1, 128, 128)
    primes = [pu.PMAX, 10007]
    _, brk, info = check_raw(mats, primes, iu.points(1, primes, 2))
    assert info[0] == 128 * (129 + 2) * 8 + 32 + 2 * 128 * 4 == 135200 and not np.any(brk)


@pytest.mark.parametrize("nd,bits", ((1, 20), (2, 44), (40, 950)))
def test_digit_counts(nd, bits):
    mats = [[row[:] for row in M] for M in mats_of(3, 18, bits)]
    mats[1][3][5] = (1 << bits) - 1                                  # the full digit count whatever the random entries are
    assert rounding.to_balanced_digits(np.array(mats, dtype=object)).shape[0] == nd
    primes = [pu.PMAX, 8388587, 10007, 5]
    check_raw(mats, primes, iu.points(nd, primes, 3))


def test_extreme_digits():
    """digits at both ends of [-2^23, 2^23], the upper end included (to_balanced_digits never produces it; the C function takes it)"""
    rng = np.random.default_rng(9)
    d, n, nd, top = 4, 19, 3, 1 << 23
    planes = rng.choice([-top, top, 0, top - 1, -top + 1, 12345], size=(d, nd, n, n)).astype(np.int64)
    planes[:, nd - 1][:, np.arange(n), np.arange(n)] = top
    mats = [[[int(v) for v in row] for row in rounding.from_balanced_digits(planes[c])] for c in range(d)]
    check_raw(mats, PRIMES, iu.points(3, PRIMES, d), digits=planes.astype(np.int32))
    allmax = np.full((2, 2, 16, 16), top, np.int32)                  # every digit 2^23: every residue matrix has rank one at most
    mats = [[[int(v) for v in row] for row in rounding.from_balanced_digits(allmax[c])] for c in range(2)]
    _, brk, _ = check_raw(mats, PRIMES, iu.points(4, PRIMES, 2), digits=allmax)
    assert np.all((brk == 1) | (brk == 2))


def test_a_cyclic_shift_gives_the_sign_of_the_determinant():
    """P A with P the cyclic shift of 17 rows (even) and of 16 rows (odd): every pivot lies off the diagonal, det(P A) = sign(P) det(A)"""
    primes = [pu.PMAX, 10007]
    for n, sign in ((17, 1), (16, -1)):
        mats = mats_of(2, n, 30, seed=n)
        shifted = [[M[(i + 1) % n] for i in range(n)] for M in mats]
        roots = iu.points(n, primes, 2)
        det, brk, _ = check_raw(mats, primes, roots)
        sdet, sbrk, _ = check_raw(shifted, primes, roots)
        assert not np.any(brk) and not np.any(sbrk)
        assert np.array_equal(sdet, (sign * det.astype(np.int64)) % np.array(primes)[:, None])


def test_a_first_column_with_its_only_entry_in_the_last_row():
    for n in (2, 33, 128):
        mats = [[row[:] for row in M] for M in mats_of(2, n, 20, seed=3)]
        for M in mats:
            for i in range(n - 1):
                M[i][0] = 0
        mats[0][n - 1][0], mats[1][n - 1][0] = 1, 0                  # never zero, whatever the root
        primes = [pu.PMAX, 10007]
        _, brk, _ = check_raw(mats, primes, iu.points(n, primes, 2))
        assert not np.any(brk)


@pytest.mark.parametrize("n", (17, 40))
def test_planted_dependent_columns_break_down_where_planted(n):
    rng = np.random.default_rng(n)
    primes = [pu.PMAX, 10007]                                        # (not 5: there an earlier column depends by chance)
    for c in (0, 7, 16, n - 1):
        mats = [np.array(M, dtype=object) for M in mats_of(3, n, 12, seed=5)]
        comb = [int(v) for v in rng.integers(-9, 10, size=c)]
        for M in mats:                                               # the same rational combination in every plane: it holds at every root
            M[:, c] = sum((w * M[:, k] for k, w in enumerate(comb)), np.zeros(n, dtype=object))
        det, brk, info = check_raw([M.tolist() for M in mats], primes, iu.points(c, primes, 3))
        assert np.all(brk == c + 1) and not np.any(det) and info[2] == 6


@pytest.mark.parametrize("nprimes", (1, 257))
def test_prime_counts(nprimes):
    """one prime, and one past the 4 x 64 primes of a wave: a second row of the residue grid with one live lane"""
    primes = [int(p) for p in rounding._primes_descending()[:nprimes]]
    check_raw(mats_of(2, 9, 40), primes, iu.points(nprimes, primes, 2))
    if nprimes == 257:
        check_raw(mats_of(4, 3, 40), primes, iu.points(7, primes, 4))


def test_more_than_one_chunk():
    mats = mats_of(3, 17, 40)
    primes = [int(p) for p in rounding._primes_descending()[:128]] + [10007, 5]
    roots = iu.points(5, primes, 3)
    want = iu.restate(mats, primes, roots)
    _, _, info = check_raw(mats, primes, roots, want=want)
    assert info[1] == 390
    _, _, info = check_raw(mats, primes, roots, chunk_bytes=65 * 17 * 17 * 8 * 3, want=want)        # 65 primes (195 pairs) per chunk: two chunks
    assert info[1] == 390
    _, _, info = check_raw(mats, primes, roots, chunk_bytes=64 * 17 * 17 * 8 * 3 + 7, want=want)    # 64 primes per chunk: three chunks, the last of 2 primes
    assert info[1] == 390
    check_raw(mats, primes[:9], roots[:9], chunk_bytes=1, want=want[:9])                    # a bound below one prime's matrices: one prime per chunk


@pytest.mark.parametrize("deg", (2, 3, 4))
def test_true_roots_give_the_images_of_the_exact_adjugate(deg):
    """at the roots of the minimal polynomial the residues are the images of det and adj in Z[g] (elimination in the field), not just those of some matrix"""
    name = {2: "x2-2", 3: "x3-2", 4: "x4-x-1"}[deg]
    fld, B, inv = iu.planted(name, 6)
    f = fld.minpoly
    det = iu.determinant_exact(f, B)
    adj = [[fu.mul(f, det, e) for e in row] for row in inv]
    mats = [[[int(e[c]) for e in row] for row in B] for c in range(deg)]
    primes, roots = rounding.split_primes(fld, 2)
    got, gdet, brk = rounding.field_adjugate_mod(mats, primes, roots)
    assert got.shape == (2, deg, 6, 6) and brk.tolist() == [[0] * deg] * 2
    image = lambda e, r, p: sum(int(c) * pow(r, j, p) for j, c in enumerate(e)) % p
    for q, p in enumerate(primes):
        for i, r in enumerate(roots[q]):
            assert int(gdet[q, i]) == image(det, r, p) and got[q, i].tolist() == [[image(e, r, p) for e in row] for row in adj]
    assert rounding.field_adjugate_mod.last_info == [iu.lds_bytes(6), 2 * deg, 0, 0]
    a, b, c = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
    assert _lib.load().clrs_modp_field_adjugate_times(C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value >= 0.0 and b.value >= 0.0 and c.value >= a.value + b.value > 0.0


def test_refusals_leave_the_library_working():
    L = _lib.load()
    mats = mats_of(2, 2, 40)
    digits = np.ascontiguousarray(np.swapaxes(rounding.to_balanced_digits(np.array(mats, dtype=object)), 0, 1))
    roots = iu.points(1, PRIMES, 2)
    pr, rt = np.array(PRIMES, np.int32), np.array(roots, np.int32)
    adj, det = np.full((3, 2, 2, 2), iu.SENTINEL, np.int32), np.full((3, 2), iu.SENTINEL, np.int32)
    brk, info = np.full((3, 2), iu.SENTINEL, np.int32), np.full(4, iu.SENTINEL, np.int32)
    null = C.POINTER(C.c_int32)()

    def call(n, deg, D, P, R, out=None):
        return L.clrs_modp_field_adjugate(0, n, deg, D.shape[1], iu._pi(D), 3, iu._pi(P), iu._pi(R), iu._pi(adj) if out is None else out, iu._pi(det), iu._pi(brk),
                                          iu._pi(info))
    assert call(2, 1, digits, pr, rt) == INVALID and call(2, 5, digits, pr, rt) == INVALID
    assert call(129, 2, np.zeros((2, 1, 129, 129), np.int32), pr, rt) == INVALID
    assert call(2, 2, digits, np.array([10007, pu.PMAX, 5], np.int32), rt) == INVALID       # unsorted: the primes descend
    assert call(2, 2, digits, np.array([pu.PMAX, 10007, 10007], np.int32), rt) == INVALID   # a repeated prime
    assert call(2, 2, digits, np.array([pu.PMAX, 10007, 9], np.int32), rt) == INVALID       # no prime
    high = rt.copy()
    high[2, 1] = 5
    assert call(2, 2, digits, pr, high) == INVALID                                           # a root >= p
    same = rt.copy()
    same[1, 1] = same[1, 0]
    assert call(2, 2, digits, pr, same) == INVALID
    assert call(2, 2, digits, pr, rt, out=null) == INVALID
    wide = digits.copy()
    wide[0, 0, 0, 0] = (1 << 23) + 1
    assert call(2, 2, wide, pr, rt) == INVALID
    assert all(int(v) == iu.SENTINEL for a in (adj, det, brk, info) for v in a.flat)
    check_raw(mats, PRIMES, roots)
    with pytest.raises(ValueError):
        rounding.field_adjugate_mod([[[1, 2], [3, 4]]], [pu.PMAX], [[1]])


@pytest.mark.parametrize("case,key", iu.GOLDEN_BLOCKS)
def test_inverse_field_on_the_device_equals_the_stand_in(case, key):
    fld = fu.field("x2-5")
    _, _, _, _, B, want = iu.golden_basis(case, key)
    host = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    dev = rounding.inverse_field(B, fld, matmul=rounding.zz_matmul)
    assert iu.as_lists(dev.inverse) == want and dev.det == host.det and np.array_equal(dev.adjugate, host.adjugate)
    assert (dev.primes, dev.roots, dev.discarded, dev.scale) == (host.primes, host.roots, [], host.scale)
    assert len(dev.primes) == iu.GOLDEN_PRIMES[(case, key)] and rounding.field_adjugate_mod.last_info[3] == 0


def test_inverse_field_over_the_other_fields_and_its_failures():
    for name in ("x4-x-1", "2x2-5"):
        fld, B, want = iu.planted(name, 8)
        assert iu.as_lists(rounding.inverse_field(B, fld).inverse) == want
    fld = fu.field("x2-5")
    f5 = fld.minpoly
    p, _ = fu.first_split_prime("x2-5")
    B = [[fu.el(f5, p), fu.el(f5, 2 * p, p)], [fu.el(f5, 3, -1), fu.el(f5, 2, 1)]]         # determinant p (the CPU test's matrix)
    assert iu.determinant_exact(f5, B) == fu.el(f5, p)
    result = rounding.inverse_field(B, fld)
    assert result.discarded == [p] and iu.as_lists(result.inverse) == iu.inverse_exact(f5, B)
    g = fu.el(f5, 0, 1)
    col = [fu.el(f5, 1, 2), fu.el(f5, -3, 1), fu.el(f5, 2)]
    with pytest.raises(rounding.SingularSystemError):
        rounding.inverse_field([[col[i], fu.mul(f5, g, col[i]), fu.el(f5, i, 1)] for i in range(3)], fld)
    with pytest.raises(rounding.SingularSystemError):                # plain entries: inverse_qq says the same
        rounding.inverse_field([[1, 2], [2, 4]], fld)


@pytest.mark.parametrize("case", ("600-cell", "icosahedron"))
def test_basis_transformations_on_the_device_equal_the_stand_ins(case):
    fld = fu.field("x2-5")
    kernels = iu.golden_kernels(case)
    settings = RoundingSettings(reduce_kernelvectors=False)
    host = rounding.basis_transformations(kernels, settings, field=fld, **iu.host_hooks())
    dev = rounding.basis_transformations(kernels, settings, field=fld, matmul=rounding.zz_matmul)
    assert list(dev) == list(kernels)
    for key, (N, vectors) in kernels.items():
        assert np.array_equal(dev[key][0], host[key][0]) and np.array_equal(dev[key][1], host[key][1]) and dev[key][2] == host[key][2] == len(vectors)
        B = [list(r) for r in zip(*iu.as_lists(dev[key][0]))]
        assert iu.matmul_exact(fld.minpoly, B, iu.as_lists(dev[key][1])) == iu.identity(fld.minpoly, N)


def test_inverse_field_against_inverse_qq_of_the_regular_representation():
    """block "20" doubled to 18 x 18: every entry x + y g becomes [[x, 5 y], [y, x]] (multiplication by it on the basis 1, g), a ring map into the rational
    matrices, so the inverse over QQ of the image is the image of the inverse over the field"""
    fld = fu.field("x2-5")
    N, _, _, _, B, _ = iu.golden_basis("600-cell", "20")
    rep = lambda e: [[e[0], 5 * e[1]], [e[1], e[0]]]
    regular = [[rep(B[i][j])[a][b] for j in range(N) for b in range(2)] for i in range(N) for a in range(2)]
    assert len(regular) == 18
    over_qq = np.asarray(rounding.inverse_qq(regular, matmul=rounding.zz_matmul))
    inv = rounding.inverse_field(B, fld).inverse
    assert [[F(over_qq[2 * i + a, 2 * j + b]) for j in range(N) for b in range(2)] for i in range(N) for a in range(2)] == \
        [[rep(inv[i, j])[a][b] for j in range(N) for b in range(2)] for i in range(N) for a in range(2)]

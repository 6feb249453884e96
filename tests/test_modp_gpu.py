"""The reduced row-echelon form mod p on the device (clrs_modp_rref: k_modp_panel, k_modp_pivot_rows, k_modp_update, k_modp_gather)
against the restatement of tests/modp_util.py with `==` -- the arithmetic is exact and the form is unique -- and against the invariants of a reduced
row-echelon form, which need no second implementation; the refusals; the front ends of clrs_amd.rounding on the device."""
import functools

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import modp_util as mu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
PMAX = 8388593
_pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)


def device_rref(A, p, want_R=True):
    """one raw call: (code, pivots with the sentinel behind the rank, rank, R)"""
    A = np.ascontiguousarray(A, dtype=np.int32)
    nrows, ncols = A.shape
    piv = np.full(max(min(nrows, ncols), 1), mu.SENTINEL, np.int32)
    rank = np.full(1, mu.SENTINEL, np.int32)
    R = np.full((nrows, ncols), mu.SENTINEL, np.int32) if want_R else None
    code = _lib.load().clrs_modp_rref(0, nrows, ncols, int(p), _pi(A), _pi(piv), _pi(rank), _pi(R))
    return code, piv, int(rank[0]), R


def check_case(A, p, want_rank=None):
    A = np.asarray(A, dtype=np.int64)
    ref_piv, ref_rank, ref_R = mu.rref_mod_p(A, p)
    if want_rank is not None:
        assert ref_rank == want_rank
    code, piv, rank, R = device_rref(A, p)
    assert code == 0, _lib.load().clrs_last_error()
    assert rank == ref_rank and list(piv[:rank]) == list(ref_piv)
    assert np.array_equal(R, ref_R)
    assert all(v == mu.SENTINEL for v in piv[rank:])
    mu.check_invariants(R, piv[:rank], rank, p)
    code, piv2, rank2, _ = device_rref(A, p, want_R=False)
    assert code == 0 and rank2 == rank and np.array_equal(piv2, piv)


W = 16                # MODP_W of csrc/clrs_modp.hip, the panel width: the shapes below straddle it
TRIP = 256            # rows one trip of the panel's workgroup clears (4 * 64 row slots); its pivot search walks 1024 rows per trip
CASES = ("1x1 zero", "1x1", "1x17", "17x1", "1x17 late pivot", "16x16 zero", "16x16 anti-diagonal", "17x33", "33x17", "40x70 rank 9", "48x64 identity first",
         "64x48 late pivots", "256x40 rank 20", "257x40 rank 20", "1025x40 rank 20")


@functools.lru_cache(maxsize=None)
def _cases(p):
    """name -> (matrix, the rank the restatement must find or None); drawn once per prime in a fixed order"""
    rng = np.random.default_rng(1000 + p % 997)
    out = {}
    out["1x1 zero"] = np.zeros((1, 1), np.int64), 0
    out["1x1"] = np.full((1, 1), p - 1, np.int64), 1
    out[f"1x{W + 1}"] = mu.random_matrix(rng, 1, W + 1, p), None
    out[f"{W + 1}x1"] = mu.random_matrix(rng, W + 1, 1, p), None
    out[f"1x{W + 1} late pivot"] = np.array([[0] * W + [1]], np.int64), 1
    out[f"{W}x{W} zero"] = np.zeros((W, W), np.int64), 0
    out[f"{W}x{W} anti-diagonal"] = np.fliplr(np.diag(rng.integers(1, p, size=W))), W           # every pivot needs a row exchange
    out[f"{W + 1}x{2 * W + 1}"] = mu.random_matrix(rng, W + 1, 2 * W + 1, p), None
    out[f"{2 * W + 1}x{W + 1}"] = mu.random_matrix(rng, 2 * W + 1, W + 1, p), None
    # planted rank 9: the panels 0 and 2 (columns 0-15, 32-47) zero, so two whole panels have no pivot; the nine pivots in panel 1 beside dependent columns
    out["40x70 rank 9"] = mu.planted(rng, 40, 70, [W + c for c in (0, 1, 3, 4, 6, 8, 11, 13, 15)], p, zero_cols=list(range(W)) + list(range(2 * W, 3 * W))), 9
    # the loop must stop at rank == nrows with the last panel untouched but final
    out[f"{3 * W}x{4 * W} identity first"] = np.concatenate([np.eye(3 * W, dtype=np.int64)[rng.permutation(3 * W)], mu.random_matrix(rng, 3 * W, W, p)], axis=1), 3 * W
    # every pivot in the last panel
    out[f"{4 * W}x{3 * W} late pivots"] = np.concatenate([np.zeros((4 * W, 2 * W), np.int64), mu.random_matrix(rng, 4 * W, W, p)], axis=1), None
    # the panel has no LDS-resident path, so no boundary between two paths; what its loops branch on instead is the trip: one trip, one row more, and one
    # row more than a trip of the pivot search, at 40 columns and rank 20
    for nrows in (TRIP, TRIP + 1, 4 * TRIP + 1):
        out[f"{nrows}x40 rank 20"] = mu.planted(rng, nrows, 40, list(range(1, 40, 2)), p), 20
    assert tuple(out) == CASES
    return out


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("p", mu.PRIMES)
def test_shapes_against_the_restatement(p, name):
    A, want_rank = _cases(p)[name]
    check_case(A, p, want_rank)


def test_300_by_700():
    rng = np.random.default_rng(7)
    check_case(mu.random_matrix(rng, 300, 700, 10007), 10007, 300)


def test_largest_accumulation_the_bound_allows():
    """every residue in [p - 4, p - 1] at the largest prime: 16 products of nearly (p - 1)^2 plus a residue in every entry of the update"""
    rng = np.random.default_rng(8)
    check_case(mu.random_matrix(rng, 33, 70, PMAX, lo=PMAX - 4), PMAX)


def test_refusals_leave_the_library_working():
    L = _lib.load()
    A = np.array([[1, 2], [3, 4]], np.int32)
    for p in (1, 4, 10005, 2 ** 23 + 9):
        assert device_rref(A, p)[0] == INVALID
    assert device_rref(np.array([[1, 7], [3, 4]]), 7)[0] == INVALID                       # a residue equal to p
    assert device_rref(np.array([[1, -2], [3, 4]]), 7)[0] == INVALID
    piv, rank = np.full(2, mu.SENTINEL, np.int32), np.full(1, mu.SENTINEL, np.int32)
    assert L.clrs_modp_rref(0, -1, 2, 7, _pi(A), _pi(piv), _pi(rank), None) == INVALID
    assert L.clrs_modp_rref(0, 2, -1, 7, _pi(A), _pi(piv), _pi(rank), None) == INVALID
    assert L.clrs_modp_rref(0, 65536, 32768, 7, _pi(A), _pi(piv), _pi(rank), None) == INVALID
    assert L.clrs_modp_rref(0, 2, 2, 7, _pi(A), None, _pi(rank), None) == INVALID
    assert list(piv) == [mu.SENTINEL] * 2 and rank[0] == mu.SENTINEL
    assert L.clrs_modp_rref(0, 0, 3, 7, None, None, _pi(rank), None) == 0 and rank[0] == 0
    check_case(A, 7, 2)


def test_front_ends_on_the_device():
    piv = rounding.find_pivots_modular([[2, 3], [3, 10]])
    assert list(piv) == [0, 1] and piv.primes == [11, 13]
    piv, rank, R = rounding.rref_mod_p([[2, 3], [3, 10]], 11, want_rref=True)
    assert list(piv) == [0] and rank == 1 and R.tolist() == mu.rref_mod_p([[2, 3], [3, 10]], 11)[2].tolist()
    # 20 x 60 Python integers around 10^30, five planted dependent columns (each the sum of its two left neighbours), and the transpose
    rng = np.random.default_rng(9)
    A = np.array([[10 ** 30 + int(v) for v in row] for row in rng.integers(-10 ** 6, 10 ** 6, size=(20, 60))], dtype=object)
    for c in (2, 5, 9, 14, 18):
        A[:, c] = A[:, c - 1] + A[:, c - 2]
    for M in (A, A.T):
        got, want = rounding.find_pivots_modular(M), rounding.find_pivots_modular(M, batch=mu.host_batch)
        assert list(got) == list(want) and got.primes == want.primes
        assert list(got) == list(rounding.find_pivots_modular(M))                         # two calls on the same input are identical
    assert list(rounding.find_pivots_modular(A)) == [c for c in range(25) if c not in (2, 5, 9, 14, 18)]
    As, b = mu.example_system()
    b2 = list(b)
    b2[2] += 1
    for args in ((As, b), (As, b2), (np.zeros((3, 5), int), np.zeros(3, int))):
        got, want = rounding.system_pivots(*args), rounding.system_pivots(*args, batch=mu.host_batch)
        assert [list(got[0]), list(got[1]), got[2]] == [list(want[0]), list(want[1]), want[2]]
    assert rounding.system_pivots(As, b)[2] and not rounding.system_pivots(As, b2)[2]

"""The lifting with a matrix of right-hand sides on the device (clrs_modp_dixon_lift_multi: k_liftm_x, k_zz_gemm, k_liftm_r) with `==`
against the restatement of tests/dixon_util.py on every column and against the existing single-column clrs_modp_dixon_lift on that column; the chunks, the
refusals, and the front ends of clrs_amd.rounding on the device."""
import functools
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_multi_util as dm
from tests import dixon_util as du
from tests import modp_util as mu

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
STEPS = 5
_pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)


def device_lift_multi(A, B, p, steps):
    """one raw call on sentinel-filled outputs: (code, X, R_limbs, info, nd, nbl)"""
    Ad, Bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(B)
    nd, nbl, (n, m) = Ad.shape[0], Bl.shape[0], B.shape
    X = np.full((steps, n, m), dm.SENTINEL, np.int32)
    R = np.full((max(nbl, nd + 1) + 1, n, m), dm.SENTINEL, np.int32)
    info = np.full(6, dm.SENTINEL, np.int32)
    code = _lib.load().clrs_modp_dixon_lift_multi(0, n, m, int(p), nd, _pi(Ad), nbl, _pi(Bl), int(steps), _pi(X) if X.size else None, _pi(R), _pi(info))
    return code, X, R, info, nd, nbl


def check_case(A, B, p, steps=STEPS, chunks=1):
    """the device call against the restatement and against the single-column device call, column by column; returns (X, R, nd)"""
    n, m = B.shape
    code, X, Rl, info, nd, nbl = device_lift_multi(A, B, p, steps)
    assert code == 0, _lib.load().clrs_last_error()
    assert info.tolist() == [n, steps, 0, 0, chunks, 0]
    assert X.min(initial=0) >= 0 and X.max(initial=0) < p
    R = rounding.from_balanced_digits(Rl)
    for j in range(m):
        want_X, want_r, rank = du.lift(A, B[:, j], p, steps)
        assert rank == n and np.array_equal(X[:, :, j], want_X), j
        assert [int(v) for v in R[:, j]] == want_r, j
        one_X, one_r, one_rank = rounding.dixon_lift(A, B[:, j], p, steps)
        assert one_rank == n and np.array_equal(X[:, :, j], one_X) and [int(v) for v in one_r] == want_r, j
    return X, R, nd


@functools.lru_cache(maxsize=None)
def _matrix(n, nd, p):
    """an n x n matrix of nd digits, invertible mod p, from a fixed seed"""
    if p == 2:
        return du.random_system(1000 + n, n, None, 2, lo_entries=8 if nd == 1 else 1 << (24 * (nd - 1) + 3))[0]
    return du.random_system(1000 + 10 * n + nd, n, (12, 40, 71)[nd - 1], p)[0]


def _rhs(n, m, nd):
    return dm.random_rhs(2000 + 100 * n + m, n, m, 12) if nd == 1 else dm.random_rhs(2000 + n + m, n, m, 60) * (1 << (24 * nd)) + dm.random_rhs(3000 + n + m, n, m, 60)


# every n with m in {1, 65}, every m with n = 65, and a handful beside them: the digits, the primes, the two-tile sizes together
CASES = ([(n, m, 1, 10007) for n in (1, 2, 15, 16, 17, 63, 64, 65, 130) for m in (1, 65)] + [(65, m, 1, 10007) for m in (2, 17, 64)] +
         [(17, 17, 2, du.PMAX), (65, 17, 3, du.PMAX), (130, 65, 2, du.PMAX), (64, 64, 3, 10007), (17, 64, 1, 2), (65, 65, 1, 2), (130, 2, 3, 2), (16, 17, 2, 10007),
          (63, 2, 1, du.PMAX)])


@pytest.mark.parametrize("n,m,nd,p", CASES)
def test_shapes_against_the_restatement_and_the_single_column_call(n, m, nd, p):
    A = _matrix(n, nd, p)
    X, R, got_nd = check_case(A, _rhs(n, m, nd), p)
    assert got_nd == nd


def test_extreme_and_boundary_systems():
    big = 2 ** 47 + 2 ** 23
    for A, p in ((du.extreme_system(130)[0], du.PMAX), (du.boundary_system(10007)[0], 10007), (du.boundary_system(du.PMAX)[0], du.PMAX)):
        n = A.shape[0]
        B = du.objects([[int(i == 1), 1, big if i % 2 else -big] for i in range(n)])        # e_1, all ones, entries at +-(2^47 + 2^23)
        X, R, nd = check_case(A, B, p)
        assert nd >= 2
        # independently of the restatement: A x == B - p^steps R
        x = np.zeros(B.shape, dtype=object)
        for k in range(STEPS - 1, -1, -1):
            x = x * p + X[k].astype(object)
        assert np.array_equal(A.dot(x), B - p ** STEPS * R)


@pytest.mark.parametrize("n", [160, 240])                          # 10 and 15 steps of k_liftm_x: across its period of 7 once and twice
def test_row_sums_past_2_53_need_the_periodic_reduction(n):
    """Operands planted so that the first product of the lifting, X_0 = A^-1 B mod p, has exact row sums that are odd and above 2^53: no fp64 value equals
    them, so k_liftm_x is right only if it reduces on the way.  C = -(2J + I) mod p (J all ones: p - 2 off the diagonal, p - 3 on it) is the inverse mod p of
    A = -(I - 2J / (2n + 1)) mod p, taken entrywise into [0, p): one digit; every entry of B is p - 2."""
    p = du.PMAX
    t = 2 * pow(2 * n + 1, -1, p) % p
    A = du.objects([[(t - 1) % p if i == j else t for j in range(n)] for i in range(n)])
    C = np.array([[p - 3 if i == j else p - 2 for j in range(n)] for i in range(n)], dtype=object)
    assert ((A.dot(C) - np.eye(n, dtype=np.int64)) % p == 0).all()
    rowsum = (n - 1) * (p - 2) ** 2 + (p - 3) * (p - 2)
    assert rowsum > 2 ** 53 and rowsum % 2 == 1 and int(float(rowsum)) != rowsum
    X, R, nd = check_case(A, du.objects(np.full((n, 2), p - 2)), p, steps=2)
    assert nd == 1 and (X[0] == rowsum % p).all()


def test_chunks_do_not_change_the_result():
    L = _lib.load()
    n, m, nd, p = 65, 65, 2, du.PMAX
    A, B = _matrix(n, nd, p), _rhs(n, m, nd)
    one = device_lift_multi(A, B, p, STEPS)
    assert one[0] == 0 and one[3].tolist() == [n, STEPS, 0, 0, 1, 0]
    nrl = one[2].shape[0]
    percol = n * (16 * nd + 16 + 4 * (nrl + 1))                    # P, Xd and Rbar, the limbs of R with the working limb
    try:
        for cols, chunks in ((22, 3), (17, 4), (1, 65)):
            assert L.clrs_config_set(b"liftm_chunk_bytes", cols * percol + percol // 2) == 0
            got = device_lift_multi(A, B, p, STEPS)
            assert got[0] == 0, L.clrs_last_error()
            assert got[3].tolist() == [n, STEPS, 0, 0, chunks, 0]
            assert np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2])
        assert L.clrs_config_set(b"liftm_chunk_bytes", 1) == 0           # never less than one column
        got = device_lift_multi(A, B[:, :3], p, 2)
        assert got[0] == 0 and got[3].tolist() == [n, 2, 0, 0, 3, 0] and np.array_equal(got[1], one[1][:2, :, :3])
    finally:
        L.clrs_config_set(b"liftm_chunk_bytes", 0)
    check_case(A, B, p)


def test_no_step():
    A, B = _matrix(17, 2, du.PMAX), _rhs(17, 17, 2)
    X, R, _ = check_case(A, B, du.PMAX, steps=0)
    assert X.shape == (0, 17, 17) and np.array_equal(R, B)          # the residual is B itself


def test_times_of_the_last_call():
    import ctypes as C
    check_case(_matrix(65, 1, 10007), _rhs(65, 17, 1), 10007)
    t = [C.c_double(-1.0) for _ in range(4)]
    assert _lib.load().clrs_modp_dixon_lift_multi_times(*[C.byref(v) for v in t]) == 0
    x, g, r, whole = (v.value for v in t)
    print("k_liftm_x, k_zz_gemm, k_liftm_r, whole call (ms):", x, g, r, whole)
    assert x > 0 and g > 0 and r > 0 and whole >= x + g + r


def test_singular_mod_p_is_no_error():
    A, B = du.objects([[2, 3], [3, 10]]), du.objects([[1, 0, 5], [1, 1, 7]])
    code, X, R, info, _, _ = device_lift_multi(A, B, 11, 4)
    assert code == 0 and info.tolist() == [1, 0, 0, 0, 0, 0]
    assert (X == dm.SENTINEL).all() and (R == dm.SENTINEL).all()
    assert rounding.dixon_lift_multi(A, B, 11, 4) == (None, None, 1)
    X, R, rank = rounding.dixon_lift_multi(A, B, 13, 4)
    want = dm.lift_columns(A, B, 13, 4)
    assert rank == 2 and np.array_equal(X, want[0]) and np.array_equal(R, want[1])
    assert rounding.dixon_lift_multi.last_info == [2, 4, 0, 0, 1, 0]
    A = du.objects(np.arange(36).reshape(6, 6) % 7)
    A[4] = 0
    assert rounding.dixon_lift_multi(A, du.objects(np.ones((6, 2), dtype=np.int64)), 10007, 3)[2] == du.inverse_mod_p(A, 10007)[1] < 6


def test_refusals_leave_the_outputs_and_the_library_working():
    L = _lib.load()
    A = np.array([[[2, 3], [3, 10]]], np.int32)
    B = np.array([[[1, 1, 0], [1, 0, 1]]], np.int32)
    X, R, info = (np.full(s, dm.SENTINEL, np.int32) for s in ((3, 2, 3), (3, 2, 3), (6,)))
    call = lambda n=2, m=3, p=13, nd=1, A=A, nbl=1, B=B, steps=3, X=X, R=R, info=info: L.clrs_modp_dixon_lift_multi(0, n, m, p, nd, _pi(A), nbl, _pi(B), steps, _pi(X),
                                                                                                               _pi(R), _pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9):
        assert call(p=p) == INVALID
    assert call(n=-1) == INVALID and call(m=-1) == INVALID and call(n=32768) == INVALID and call(nd=0) == INVALID and call(nbl=0) == INVALID
    assert call(steps=-1) == INVALID and call(m=2 ** 30) == INVALID
    assert call(A=np.array([[[2, 3], [3, 2 ** 23]]], np.int32)) == INVALID and call(B=np.array([[[1, 1, 0], [1, 0, -2 ** 23 - 1]]], np.int32)) == INVALID
    assert call(A=None) == INVALID and call(info=None) == INVALID
    assert all(int(v) == dm.SENTINEL for a in (X, R, info) for v in a.flat)
    assert call() == 0 and info.tolist() == [2, 3, 0, 0, 1, 0]
    want = dm.lift_columns([[2, 3], [3, 10]], [[1, 1, 0], [1, 0, 1]], 13, 3)
    assert np.array_equal(X, want[0]) and np.array_equal(rounding.from_balanced_digits(R), want[1])


# ---- the front ends on the device ---------------------------------------------------------------------------------------------------------------------------
def test_inverse_qq_on_the_device():
    n = 65
    A = _matrix(n, 1, du.PMAX)
    inv = rounding.inverse_qq(A, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul)
    assert inv.p == du.PMAX and inv.steps > 0 and rounding.dixon_lift_multi.last_info[:6] == [n, inv.steps, 0, 0, 1, 0]
    # B Binv == I on the host, in Python integers over the common denominator of the inverse
    num, den = rounding._common_denominator(inv.flat)
    prod = A.dot(num.reshape(n, n))
    assert all(int(prod[i, j]) == (den if i == j else 0) for i in range(n) for j in range(n))
    host = rounding.inverse_qq(A, lift=dm.lift_columns)
    assert np.array_equal(inv, host) and np.array_equal(rounding.inverse_qq(A), host)


@functools.lru_cache(maxsize=None)
def _delsarte_blocks():
    """solvesdp_mw on delsarte_exact(8, 3, 1/2) at 10 limbs, then the kernel rounded on the device (as tests/test_rationalize_gpu.py does)"""
    import clrs_amd
    from clrs_amd import problems as P
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    with data_planes(10):
        f = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5, prec=640))
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    assert res.error_code == 0 and res.status == "Optimal"
    blocks = rounding.kernel_vectors(f, res, res, settings=rounding.RoundingSettings(), check_dimensions=True, rationalize=True)
    return {i: (int(n), rounding.vectors_to_fractions(k)) for i, (n, k) in enumerate(zip(f.block_n, blocks))}


def test_basis_transformations_of_delsarte_exact_on_the_device():
    kernels = _delsarte_blocks()
    assert [len(v) for _, v in kernels.values()] == [1, 0, 0, 0, 0, 0, 0, 4, 2]
    for settings in (rounding.RoundingSettings(reduce_kernelvectors=False), rounding.RoundingSettings(reduce_kernelvectors=False, normalize_transformation=False)):
        got = rounding.basis_transformations(kernels, settings, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul)
        want = rounding.basis_transformations(kernels, settings, batch=mu.host_batch, lift=dm.lift_columns)
        assert list(got) == list(want)
        for key in want:
            assert np.array_equal(got[key][0], want[key][0]) and np.array_equal(got[key][1], want[key][1]) and got[key][2] == want[key][2]
            N = kernels[key][0]
            assert dm.frac_matmul(got[key][0].T, got[key][1]) == dm.identity(N)
    with pytest.raises(NotImplementedError):
        rounding.basis_transformations(kernels)

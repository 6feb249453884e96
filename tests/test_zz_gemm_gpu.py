"""GPU tests of the exact integer matrix product (clrs_zz_gemm).  Outputs are filled with sentinels before every call, the planes are
compared with `==` against `to_balanced_digits(exact, count=ndc)`, the oracle is Python integer arithmetic, and no call may report an impossibility."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import zz_util as zu

pytestmark = pytest.mark.gpu


def _check(name, Ad, Bd, extra=0):
    exact = zu.exact_product(Ad, Bd)
    ndc = zu.digits_needed(exact) + extra
    code, Cd, info = zu.device_gemm(Ad, Bd, ndc)
    assert code == 0, (name, _lib.load().clrs_last_error())
    assert info[0] == 0 and info[1] >= 1 and info[2] >= 1 and info[3] == 0, (name, info)
    assert np.array_equal(Cd, zu.expected_planes(exact, ndc)), name
    return info


@pytest.mark.parametrize("nd", (1, 2))
def test_shapes_at_the_tile_edges(nd):
    """m, n in {1, 15, 16, 17, 63, 64, 65}, k = 17"""
    for name, Ad, Bd in zu.shape_cases():
        if Ad.shape[0] == nd:
            info = _check(name, Ad, Bd)
            m, n = Ad.shape[1], Bd.shape[2]
            assert info[2] == -(-nd * m // 64) * -(-nd * n // 64), name       # the workgroups of one 64 x 64 tiling of P


@pytest.mark.parametrize("mode", ("random", "equal", "mix"))
def test_inner_extents_across_the_flush_boundary(mode):
    """m = n = 17; every digit +-(2^23 - 1) with random signs or all signs equal, and a mix with +-2^23"""
    for name, Ad, Bd in zu.k_cases():
        if name.endswith(mode):
            _check(name, Ad, Bd)


def test_digit_counts():
    for name, Ad, Bd in zu.digit_cases():
        _check(name, Ad, Bd)


def test_the_check_shape_and_its_ranges():
    """33 x 33 of two digits times a vector of 300 digits; the same product in one range and forced into several: equal planes, info[1] as expected"""
    name, Ad, Bd = zu.vector_case()
    exact = zu.exact_product(Ad, Bd)
    ndc = zu.digits_needed(exact)
    want = zu.expected_planes(exact, ndc)
    L = _lib.load()
    try:
        for bound in (0, 16 * 2 * 33 * 7, 16 * 2 * 33 * 299, 1):
            assert L.clrs_config_set(b"zz_gemm_chunk_bytes", bound) == 0
            code, Cd, info = zu.device_gemm(Ad, Bd, ndc)
            assert code == 0 and info[0] == 0 and info[3] == 0
            assert info[1] == zu.chunks_expected(2, 33, 1, 300, bound if bound else 256 << 20)
            assert np.array_equal(Cd, want), bound
        assert zu.chunks_expected(2, 33, 1, 300, 16 * 2 * 33 * 7) == 43 and zu.chunks_expected(2, 33, 1, 300, 1) == 300
        # a matrix on the right, ranges that cut between its digits
        Ad, Bd = zu.random_digits(21, 3, 19, 40), zu.random_digits(22, 5, 40, 23)
        exact = zu.exact_product(Ad, Bd)
        ndc = zu.digits_needed(exact)
        planes = []
        for bound in (0, 16 * 3 * 19 * 23 * 2, 16 * 3 * 19 * 23):
            assert L.clrs_config_set(b"zz_gemm_chunk_bytes", bound) == 0
            code, Cd, info = zu.device_gemm(Ad, Bd, ndc)
            assert code == 0 and info[1] == {0: 1, 16 * 3 * 19 * 23 * 2: 3, 16 * 3 * 19 * 23: 5}[bound]
            planes.append(Cd)
        assert all(np.array_equal(p, zu.expected_planes(exact, ndc)) for p in planes)
    finally:
        L.clrs_config_set(b"zz_gemm_chunk_bytes", 0)


def test_result_digits_sufficient_larger_and_too_few():
    Ad, Bd = zu.random_digits(31, 2, 18, 20), zu.random_digits(32, 2, 20, 17)
    exact = zu.exact_product(Ad, Bd)
    assert any(v < 0 for v in exact.flat) and any(v > 0 for v in exact.flat)
    _check("exact", Ad, Bd)
    _check("larger", Ad, Bd, extra=1)
    _check("much larger: past nda + ndb + 2", Ad, Bd, extra=5)
    ndc = zu.digits_needed(exact)
    too_long = sum(1 for v in exact.flat if rounding.to_balanced_digits(np.array([v], dtype=object)).shape[0] > ndc - 1)
    code, Cd, info = zu.device_gemm(Ad, Bd, ndc - 1)
    assert code == -1 and b"fit" in _lib.load().clrs_last_error()
    assert info[0] == too_long > 0 and info[3] == 0 and (Cd == zu.SENTINEL).all()
    _check("after the refusal", Ad, Bd)
    with pytest.raises(_lib.ClrsError):
        rounding._zz_gemm_planes(Ad, Bd, ndc - 1)
    assert rounding.zz_matmul.last_info[0] == too_long


def test_zero_operands():
    Ad, Z = zu.random_digits(41, 2, 17, 33), np.zeros((3, 33, 5), np.int32)
    _check("A times 0", Ad, Z)
    _check("0 times B", np.zeros((1, 4, 33), np.int32), zu.random_digits(42, 2, 33, 9))
    code, Cd, info = zu.device_gemm(Ad, Z, 4)
    assert code == 0 and not Cd.any()


def test_zz_matmul_on_entries_of_mixed_sizes():
    rng = np.random.default_rng(51)
    sizes = [1, 20, 24, 47, 100, 1000, 5000]
    A = np.array([[int.from_bytes(rng.bytes(sizes[(i + j) % 7] // 8 + 1), "little") * (-1) ** (i * j) for j in range(13)] for i in range(19)], dtype=object)
    B = np.array([[int.from_bytes(rng.bytes(sizes[(2 * i + j) % 7] // 8 + 1), "little") * (-1) ** (i + j) for j in range(6)] for i in range(13)], dtype=object)
    A[3, 4], B[2, 2] = 0, 0
    out = rounding.zz_matmul(A, B)
    assert out.dtype == object and out.shape == (19, 6) and all(type(v) is int for v in out.flat) and (out == A.dot(B)).all()
    assert rounding.zz_matmul.last_info[0] == 0 and rounding.zz_matmul.last_info[3] == 0
    v = rounding.zz_matmul(A, B[:, 0])
    assert v.shape == (19,) and (v == A.dot(B[:, 0])).all()
    small = rng.integers(-2 ** 40, 2 ** 40, size=(5, 8))
    assert (rounding.zz_matmul(small, small.T) == small.astype(object).dot(small.T.astype(object))).all()
    assert rounding.zz_matmul([[1, 2], [3, 4]], [[5], [6]]).tolist() == [[17], [39]]


def test_event_times_are_finite_and_positive():
    _check("timed", zu.random_digits(61, 2, 70, 90), zu.random_digits(62, 2, 90, 66))
    times = zu.device_times()
    assert all(math.isfinite(t) and t > 0.0 for t in times) and times[2] >= times[0], times


# ---- the front ends on the device, n = 48, with the device lift and reconstruction, against Fraction arithmetic and against the default path -------------------------
def _device(**kw):
    return dict(reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul, **kw)


def test_solve_dixon_with_the_device_products():
    A, b = du.random_system(31, 48, 6, du.PMAX)
    A = [[F(int(v)) for v in row] for row in A]
    A[0] = [v / 3 for v in A[0]]                                  # a row with denominators
    b = [F(int(v), 5) for v in b]
    count = zu.CountingMatmul(inner=rounding.zz_matmul)
    sol = rounding.solve_dixon(A, b, reconstruct=rounding.dixon_reconstruct, matmul=count)
    host = rounding.solve_dixon(A, b)
    assert list(sol) == du.gauss_solve(A, b) == list(host) and (sol.p, sol.primes, sol.steps) == (host.p, host.primes, host.steps)
    assert count.calls == [((48, 48), (48,)), ((48, 48), (48,))]
    with pytest.raises(ArithmeticError):
        rounding.solve_dixon(A, b, reconstruct=rounding.dixon_reconstruct, matmul=zu.CountingMatmul(corrupt=1, inner=rounding.zz_matmul))


def test_solve_system_pseudoinverse_with_the_device_products():
    rng = np.random.default_rng(32)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 51))]
    b = [F(int(v)) for v in rng.integers(-9, 10, size=48)]
    G = [[sum(x * y for x, y in zip(r, s)) for s in A] for r in A]
    y = du.gauss_solve(G, b)
    v = rounding.solve_system_pseudoinverse(A, b, **_device())
    assert v == [sum(A[r][c] * y[r] for r in range(48)) for c in range(51)] and du.matvec(A, v) == b
    assert v == rounding.solve_system_pseudoinverse(A, b)
    tall = [list(col) for col in zip(*A)]
    bt = [F(int(t), 3) for t in rng.integers(-9, 10, size=51)]
    assert rounding.solve_system_pseudoinverse(tall, bt, **_device()) == rounding.solve_system_pseudoinverse(tall, bt)


def test_project_to_affine_space_and_is_valid_solution_with_the_device_products():
    rng = np.random.default_rng(33)
    A = [[F(int(v)) for v in row] for row in rng.integers(-9, 10, size=(48, 60))]
    A[47] = [x + y for x, y in zip(A[0], A[1])]                    # a dependent row
    x0 = [F(int(v), 7) for v in rng.integers(-9, 10, size=60)]
    b = du.matvec(A, x0)
    x, ok, finished = rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5), **_device())
    assert ok and finished and du.matvec(A, x) == b
    assert (x, ok, finished) == rounding.project_to_affine_space(A, b, rng=np.random.default_rng(5))
    plain = rounding.RoundingSettings(pseudo=False)                 # 47 pivots in 48 rows: the normal equations
    got = rounding.project_to_affine_space(A, b, settings=plain, **_device())
    assert got == rounding.project_to_affine_space(A, b, settings=plain) and got[1] and du.matvec(A, got[0]) == b
    assert rounding.is_valid_solution([], A, b, x, matmul=rounding.zz_matmul) == (True, [])
    wrong = list(x)
    wrong[7] += F(2, 13)
    res = rounding.is_valid_solution([[[2, 1], [1, 2]]], A, b, wrong, matmul=rounding.zz_matmul)
    assert res == rounding.is_valid_solution([[[2, 1], [1, 2]]], A, b, wrong) and not res[0]
    slacks = [s - t for s, t in zip(du.matvec(A, wrong), b)]
    assert res[1] == [("constraint", i, s) for i, s in enumerate(slacks) if s != 0]

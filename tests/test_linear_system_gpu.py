"""GPU tests of the assembly of the rational linear system (clrs_zz_lowrank_system) and of `exact_solution` with every step on the
device.  Outputs are filled with sentinels before every call, the planes are compared with `==` against the digits of Python integers, and no call may report
an impossibility."""
import functools
import math
from fractions import Fraction as F

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd import problems as P
from tests import lrsys_util as lu
from tests import zz_util as zu

pytestmark = pytest.mark.gpu


def _check(name, Ud, Wd, rowptr, pairs, extra=0):
    exact = lu.exact_system(Ud, Wd, rowptr, pairs)
    ndc = zu.digits_needed(exact) + extra
    code, Cd, info = lu.device_system(Ud, Wd, rowptr, pairs, ndc)
    assert code == 0, (name, _lib.load().clrs_last_error())
    assert info[0] == 0 and info[1] >= 1 and info[2] >= 1 and info[3] == 0, (name, info)
    assert np.array_equal(Cd, zu.expected_planes(exact, ndc)), name
    return info


@pytest.mark.parametrize("ndu,ndw", [(1, 1), (2, 3), (9, 9)])
def test_sizes_at_the_tile_edges_with_mixed_rows(ndu, ndw):
    """n in {1, 2, 15, 16, 17, 33}; rows of 0, 1, 2 and 5 terms in one call; all pairs, and a sparse selection that leaves whole tiles empty"""
    for n in (1, 2, 15, 16, 17, 33):
        Ud, Wd, rowptr = lu.mixed_case(100 * n + ndu, n, ndu, ndw)
        nt = -(-n // 16)
        info = _check(f"n{n}", Ud, Wd, rowptr, lu.all_pairs(n))
        assert info[2] == 6 * nt * (nt + 1) // 2, (n, info)             # every tile of the triangle, per row
        info = _check(f"n{n}-sparse", Ud, Wd, rowptr, lu.sparse_pairs(n), extra=2)
        tiles = {(a // 16, b // 16) for a, b in lu.sparse_pairs(n)}
        assert info[2] == 6 * len(tiles) and (n < 33 or len(tiles) < nt * (nt + 1) // 2), (n, info)


def test_extreme_digits_past_a_flush_period():
    """r = 5, ndu = ndw = 30, every digit +-2^23: 150 products in the middle digit, past 28 MFMAs and past 2^53 without the flush"""
    rowptr = lu.row_pointer([5, 0, 5])
    Ud, Wd = lu.extreme_digits(7, 30, 17, 10), lu.extreme_digits(8, 30, 17, 10)
    _check("extreme", Ud, Wd, rowptr, lu.all_pairs(17))
    same = np.abs(Ud)
    _check("extreme, equal signs", same, same, rowptr, lu.all_pairs(17))


def test_panels_of_terms_and_of_digits():
    """rows whose terms, and operands whose digits, do not fit the staged panel at once (clrs_modp_lrsys_arith.h: 160 doubles per row)"""
    rowptr = lu.row_pointer([40, 3, 0, 23])
    Ud, Wd = zu.random_digits(71, 9, 17, 66), zu.random_digits(72, 7, 17, 66)
    assert lu.host_panels(40, 9, 7)[:3] == [17, 9, 7]
    _check("terms", Ud, Wd, rowptr, lu.all_pairs(17))
    rowptr = lu.row_pointer([1, 2])
    Ud, Wd = zu.random_digits(73, 200, 5, 3), zu.random_digits(74, 170, 5, 3)
    assert lu.host_panels(2, 200, 170)[:3] == [1, 160, 160]
    _check("digits", Ud, Wd, rowptr, lu.all_pairs(5))
    Ud = lu.extreme_digits(75, 330, 2, 2)
    _check("digits, extreme", Ud, np.abs(Ud), lu.row_pointer([2]), lu.all_pairs(2))


def test_chunks_of_rows_give_identical_outputs():
    Ud, Wd, rowptr = lu.mixed_case(81, 17, 2, 3, counts=(2, 0, 5, 1, 1, 3, 2))
    pairs = lu.sparse_pairs(17)
    exact = lu.exact_system(Ud, Wd, rowptr, pairs)
    ndc = zu.digits_needed(exact)
    want = zu.expected_planes(exact, ndc)
    per_row = 8 * (2 + 3 - 1) * len(pairs)
    L = _lib.load()
    try:
        for bound, chunks in ((0, 1), (3 * per_row, 3), (per_row, 7), (1, 7)):
            assert L.clrs_config_set(b"lrsys_chunk_bytes", bound) == 0
            code, Cd, info = lu.device_system(Ud, Wd, rowptr, pairs, ndc)
            assert code == 0 and info[0] == 0 and info[3] == 0 and info[1] == chunks, (bound, info)
            assert np.array_equal(Cd, want), bound
    finally:
        L.clrs_config_set(b"lrsys_chunk_bytes", 0)


def test_result_digits_sufficient_larger_and_too_few():
    Ud, Wd, rowptr = lu.mixed_case(91, 18, 2, 2)
    pairs = lu.all_pairs(18)
    exact = lu.exact_system(Ud, Wd, rowptr, pairs)
    assert any(v < 0 for v in exact.flat) and any(v > 0 for v in exact.flat)
    _check("exact", Ud, Wd, rowptr, pairs)
    _check("much larger: past ndu + ndw + 2", Ud, Wd, rowptr, pairs, extra=5)
    ndc = zu.digits_needed(exact)
    too_long = sum(1 for v in exact.flat if zu.digits_restated([v]).shape[0] > ndc - 1)
    code, Cd, info = lu.device_system(Ud, Wd, rowptr, pairs, ndc - 1)
    assert code == lu.INVALID and b"fit" in _lib.load().clrs_last_error()
    assert info[0] == too_long > 0 and info[3] == 0 and (Cd == lu.SENTINEL).all()
    _check("after the refusal", Ud, Wd, rowptr, pairs)
    with pytest.raises(_lib.ClrsError):
        rounding._lowrank_system_planes(Ud, Wd, rowptr, *zip(*pairs), ndc - 1)
    assert rounding.lowrank_system.last_info[0] == too_long
    times = lu.device_times()
    assert all(math.isfinite(t) and t >= 0.0 for t in times) and times[2] > 0.0


def test_lowrank_system_on_entries_of_mixed_sizes():
    rng = np.random.default_rng(95)
    sizes = [1, 20, 24, 47, 100, 1000]
    big = lambda i, j: int.from_bytes(rng.bytes(sizes[(i + 2 * j) % 6] // 8 + 1), "little") * (-1) ** (i + j)
    U = np.array([[big(i, j) for j in range(9)] for i in range(19)], dtype=object)
    W = np.array([[big(j, i) for j in range(9)] for i in range(19)], dtype=object)
    rowptr, pairs = [0, 4, 4, 9], lu.all_pairs(19)
    out = rounding.lowrank_system(U, W, rowptr, pairs)
    assert out.dtype == object and out.shape == (3, len(pairs)) and all(type(v) is int for v in out.flat)
    assert (out == lu.host_assemble(U, W, rowptr, pairs)).all() and rounding.lowrank_system.last_info[0] == 0 and rounding.lowrank_system.last_info[3] == 0


@pytest.mark.parametrize("transformed", (False, True))
def test_linear_system_with_the_device_assembly_and_products(transformed):
    problem = lu.handmade_problem()
    Bs = lu.handmade_Bs(problem) if transformed else None
    A, b, index = rounding.linear_system(problem, Bs=Bs, matmul=rounding.zz_matmul)
    host = rounding.linear_system(problem, Bs=Bs, assemble=lu.host_assemble)
    assert np.array_equal(A, host[0]) and b == host[1] and index == host[2]


@functools.lru_cache(maxsize=None)
def _delsarte_solution():
    """solvesdp_mw on delsarte_exact_problem(8, 3, 1/2).to_sdp(640) at 10 limbs, gap 1e-40 (as tests/test_dixon_multi_gpu.py does)"""
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    problem = P.delsarte_exact_problem(8, 3, F(1, 2))
    with data_planes(10):
        f = clrs_amd.flatten(problem.to_sdp(640))
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    assert res.error_code == 0 and res.status == "Optimal"
    return problem, res


def test_exact_solution_of_delsarte_exact_on_the_device():
    problem, res = _delsarte_solution()
    settings = rounding.RoundingSettings(reduce_kernelvectors=False)
    assemble = lu.Counting(rounding.lowrank_system)
    sol = rounding.exact_solution(problem, res, settings, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul, assemble=assemble)
    lu.check_delsarte_exact_solution(problem, sol)
    assert len(assemble.calls) == 1 and rounding.lowrank_system.last_info[0] == 0 and rounding.lowrank_system.last_info[3] == 0
    with pytest.raises(NotImplementedError):
        rounding.exact_solution(problem, res)

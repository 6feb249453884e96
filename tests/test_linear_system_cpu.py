"""CPU side of the assembly of the rational linear system and of `exact_solution` (clrs_zz_lowrank_system, clrs_amd.rounding): the
index arithmetic of csrc/clrs_modp_lrsys_arith.h compiled for the host and the whole entry restated with it against Python integers, the refusals of the
library (no device is touched), the exact problem against the numeric one, `linear_system` against a dense restatement, the sign and factor conventions on
the 320-bit oracle's solution of delsarte_exact(8, 3, 1/2), `select_columns`, and `exact_solution` with host stand-ins for every device call.  Every
comparison of integers or rationals is `==`."""
import functools
import re
import os
from fractions import Fraction as F

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd import problems as P
from tests import lrsys_util as lu
from tests import zz_util as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_check(name, Ud, Wd, rowptr, pairs, panels=(0, 0, 0), extra=0):
    exact = lu.exact_system(Ud, Wd, rowptr, pairs)
    ndc = zu.digits_needed(exact) + extra
    code, Cd, info = lu.host_system(Ud, Wd, rowptr, pairs, ndc, panels)
    assert code == 0 and info[0] == 0 and info[3] == 0, (name, code, info)
    assert np.array_equal(Cd, zu.expected_planes(exact, ndc)), name
    return info


# ---- the host build of clrs_modp_lrsys_arith.h -------------------------------------------------------------------------------------------------------------------
def test_constants_panels_and_strides():
    tile, cap, flush, most, kmax = lu.host_constants()
    assert (tile, flush, most, kmax) == (16, 28, 31, 1 << 14) and flush <= most
    for rmax, ndu, ndw in [(1, 1, 1), (5, 30, 30), (5, 9, 9), (40, 9, 9), (7, 2, 3), (1, 200, 3), (3, 161, 400), (1000, 1, 1), (2, 160, 160), (1, 160, 161)]:
        tp, dp, dq, ldu, ldw = lu.host_panels(rmax, ndu, ndw)
        assert 1 <= tp <= rmax and 1 <= dp <= ndu and 1 <= dq <= ndw and tp * max(dp, dq) <= cap
        if rmax * max(ndu, ndw) <= cap:
            assert (tp, dp, dq) == (rmax, ndu, ndw)                    # everything at once whenever it fits
        if tp > 1:
            assert (dp, dq) == (ndu, ndw)                              # digits are cut only when one term does not fit
        for ld, length in ((ldu, tp * dp), (ldw, tp * dq)):
            assert length <= ld < length + 32 and ld % 32 == 2
            assert sorted((ld * r) % 32 for r in range(16)) == list(range(0, 32, 2))       # the 16 rows of an operand: the 16 even residues
        assert 16 * (ldu + ldw) * 8 <= 64 * 1024


def test_p_range_and_slots_against_python():
    for p0, dp, q0, dq in [(0, 1, 0, 1), (0, 3, 0, 2), (2, 3, 4, 5), (0, 9, 0, 9), (5, 1, 0, 7), (160, 40, 320, 80)]:
        seen = set()
        for s in range(p0 + q0 - 2, p0 + dp + q0 + dq + 1):
            count, plo, phi = lu.host_p_range(s, p0, dp, q0, dq)
            want = [p for p in range(p0, p0 + dp) if q0 <= s - p < q0 + dq]
            assert count == len(want) and (not want or (plo, phi) == (want[0], want[-1])), (s, p0, dp, q0, dq)
            seen.update((p, s - p) for p in want)
            assert (count >= 1) == (p0 + q0 <= s <= p0 + dp - 1 + q0 + dq - 1)
        assert len(seen) == dp * dq                                    # every pair of digits of the two panels meets exactly one s
    for np_ in (1, 2, 3, 4, 5, 9, 30):
        for lane4 in range(4):
            got = lu.host_slots(lane4, np_, 40)
            assert got == [divmod(lane4 + 4 * k, np_) for k in range(40)]


@pytest.mark.parametrize("ndu,ndw", [(1, 1), (2, 3), (9, 9)])
def test_host_entry_on_random_operands(ndu, ndw):
    for n in (1, 2, 17):
        Ud, Wd, rowptr = lu.mixed_case(100 * n + ndu, n, ndu, ndw)
        _host_check(f"n{n}", Ud, Wd, rowptr, lu.all_pairs(n))
        _host_check(f"n{n}-sparse", Ud, Wd, rowptr, lu.sparse_pairs(n), extra=2)
        for panels in ((1, ndu, ndw), (2, 1, 1), (1, max(ndu - 1, 1), 2), (3, 2, ndw)):
            _host_check(f"n{n}-{panels}", Ud, Wd, rowptr, lu.all_pairs(n), panels)


def test_host_entry_on_extreme_digits_past_a_flush_period():
    """r = 5, ndu = ndw = 30, every digit +-2^23: the middle digit sums 150 products, more than 28 MFMAs of four hold and more than 2^53 without a flush"""
    rowptr = lu.row_pointer([5, 0, 5])
    Ud, Wd = lu.extreme_digits(7, 30, 3, 10), lu.extreme_digits(8, 30, 3, 10)
    assert 150 > 4 * 28 and 150 * 2 ** 46 > 2 ** 53
    info = _host_check("extreme", Ud, Wd, rowptr, lu.all_pairs(3))
    _host_check("extreme in panels", Ud, Wd, rowptr, lu.all_pairs(3), (2, 7, 11))
    same = np.abs(Ud)                                                   # all signs equal: the largest sums there are
    _host_check("extreme, equal signs", same, same, rowptr, lu.all_pairs(3))


def test_host_entry_with_too_few_digits_raises_its_counter_alone():
    Ud, Wd, rowptr = lu.mixed_case(5, 4, 2, 2)
    pairs = lu.all_pairs(4)
    exact = lu.exact_system(Ud, Wd, rowptr, pairs)
    ndc = zu.digits_needed(exact)
    too_long = sum(1 for v in exact.flat if zu.digits_restated([v]).shape[0] > ndc - 1)
    code, Cd, info = lu.host_system(Ud, Wd, rowptr, pairs, ndc - 1)
    assert code == -1 and info[0] == too_long > 0 and info[3] == 0 and (Cd == lu.SENTINEL).all()


# ---- the library: binding, prototypes, refusals (no device is touched) ------------------------------------------------------------------------------------------
def test_binding_and_prototypes():
    for name in ("clrs_zz_lowrank_system", "clrs_zz_lowrank_system_times"):
        assert name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "clrs_hip.h")).read()
    proto = re.search(r"int clrs_zz_lowrank_system\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_lib.SYMBOLS["clrs_zz_lowrank_system"][1]) == 15
    L = _lib.load()
    assert L.clrs_zz_lowrank_system_times(None, None, None) == lu.INVALID


def test_refusals_leave_the_output_untouched():
    Ud, Wd, rowptr = lu.mixed_case(9, 3, 2, 2)
    pairs = lu.all_pairs(3)
    L = _lib.load()

    def refused(Ud=Ud, Wd=Wd, rowptr=rowptr, pairs=pairs, ndc=6, word=b""):
        code, Cd, info = lu.device_system(Ud, Wd, rowptr, pairs, ndc)
        assert code == lu.INVALID and (Cd == lu.SENTINEL).all() and (info == lu.SENTINEL).all(), (code, word)
        assert word in L.clrs_last_error(), L.clrs_last_error()

    big = Ud.copy(); big[1, 2, 3] = lu.HALF + 1
    refused(Ud=big, word=b"digit of U")
    small = Wd.copy(); small[0, 0, 0] = -lu.HALF - 1
    refused(Wd=small, word=b"digit of W")
    edge = Ud.copy(); edge[0, 0, 0], edge[1, 1, 1] = lu.HALF, -lu.HALF            # the ends of the range are digits
    bad = rowptr.copy(); bad[2], bad[3] = bad[3], bad[2]
    if bad[2] != bad[3]:
        refused(rowptr=bad, word=b"rowptr")
    short = rowptr.copy(); short[-1] -= 1
    refused(rowptr=short, word=b"rowptr")
    first = rowptr.copy(); first[0] = 1
    refused(rowptr=first, word=b"rowptr")
    refused(pairs=[(1, 0)], word=b"pair")
    refused(pairs=[(0, 3)], word=b"pair")
    refused(pairs=[(-1, 0)], word=b"pair")
    pi, info = lu._pi, np.zeros(4, np.int32)
    T, ca, cb = int(rowptr[-1]), np.zeros(1, np.int32), np.zeros(1, np.int32)
    out = np.full((2, 6, 1), lu.SENTINEL, np.int32)
    call = lambda *a: L.clrs_zz_lowrank_system(0, *a)
    assert call(-1, T, 6, pi(rowptr), 2, pi(Ud), 2, pi(Wd), 1, pi(ca), pi(cb), 2, pi(out), pi(info)) == lu.INVALID
    assert call(3, T, 6, pi(rowptr), 2, pi(Ud), 2, pi(Wd), -1, pi(ca), pi(cb), 2, pi(out), pi(info)) == lu.INVALID
    for ndu, ndw, ndc in ((0, 2, 2), (2, 32768, 2), (2, 2, 0), (2, 2, 32768)):
        assert call(3, T, 6, pi(rowptr), ndu, pi(Ud), ndw, pi(Wd), 1, pi(ca), pi(cb), ndc, pi(out), pi(info)) == lu.INVALID
    for nulls in range(6):
        a = [pi(rowptr), pi(Ud), pi(Wd), pi(ca), pi(cb), pi(out), pi(info)]
        a[nulls if nulls < 6 else 6] = None
        assert call(3, T, 6, a[0], 2, a[1], 2, a[2], 1, a[3], a[4], 2, a[5], a[6]) == lu.INVALID and b"null" in L.clrs_last_error()
    assert call(3, T, 6, pi(rowptr), 2, pi(Ud), 2, pi(Wd), 1, pi(ca), pi(cb), 2, pi(out), None) == lu.INVALID
    assert call(3, T, 6, pi(rowptr), 2, pi(Ud), 2, pi(Wd), 1 << 20, pi(ca), pi(cb), 32767, pi(out), pi(info)) == lu.INVALID and b"2^31" in L.clrs_last_error()
    assert (out == lu.SENTINEL).all()
    # K = (terms of a row) min(ndu, ndw) must stay below 2^14
    wide = np.zeros((1, 1, 1 << 14), np.int32)
    code, Cd, _ = lu.device_system(wide, wide, [0, 1 << 14], [(0, 0)], 3)
    assert code == lu.INVALID and b"2^14" in L.clrs_last_error() and (Cd == lu.SENTINEL).all()
    with pytest.raises(ValueError):
        rounding.lowrank_system(wide[0].astype(object), wide[0].astype(object), [0, 1 << 14], [(0, 0)])


def test_trivial_cases_need_no_device():
    Ud, Wd, rowptr = lu.mixed_case(11, 3, 2, 2)
    code, Cd, info = lu.device_system(Ud, Wd, rowptr, [], 2)
    assert code == 0 and Cd.shape == (2, 6, 0) and info.tolist() == [0, 0, 0, 0]
    code, Cd, info = lu.device_system(Ud, Wd, [0], lu.all_pairs(3), 2)
    assert code == lu.INVALID                                           # rowptr must end at T
    empty = np.zeros((2, 3, 0), np.int32)
    code, Cd, info = lu.device_system(empty, empty, [0, 0, 0], lu.all_pairs(3), 2)
    assert code == 0 and not Cd.any() and info.tolist() == [0, 0, 0, 0]
    code, Cd, info = lu.device_system(empty, empty, [0], lu.all_pairs(3), 2)
    assert code == 0 and Cd.shape == (2, 0, 6)
    assert lu.device_times() == [0.0, 0.0, 0.0]
    out = rounding.lowrank_system(np.zeros((3, 0), dtype=object), np.zeros((3, 0), dtype=object), [0, 0], lu.all_pairs(3))
    assert out.shape == (1, 6) and all(v == 0 for v in out.flat) and rounding.lowrank_system.last_info == [0, 0, 0, 0]


# ---- the exact problem and the numeric one -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", (256, 640))
def test_exact_problem_is_the_numeric_problem(prec):
    exact = clrs_amd.flatten(P.delsarte_exact_problem(8, 3, F(1, 2)).to_sdp(prec))
    numeric = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5, prec))
    for name, want in vars(numeric).items():
        got = getattr(exact, name)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), name
        else:
            assert got == want, name


# ---- linear_system against the dense restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transformed", (False, True))
def test_linear_system_against_the_dense_restatement(transformed):
    problem = lu.handmade_problem()
    problem.to_sdp().check()                                            # the transposed partners are present
    Bs = lu.handmade_Bs(problem) if transformed else None
    rows, b, index = lu.restated_system(problem, Bs)
    assemble = lu.Counting(lu.host_assemble)
    A, b2, index2 = rounding.linear_system(problem, Bs=Bs, assemble=assemble)
    assert index2 == index == rounding.system_index(problem, Bs) and b2 == b
    assert A.shape == (5, len(index)) and [list(r) for r in A] == rows
    assert len(assemble.calls) == 2                                     # one call per low-rank block
    assert len(index) == (6 if transformed else 10) + 6 + 10 + 2
    assert any(v != 0 for v in A[:3, :6].flat) and all(v == 0 for v in A[3:, :6 if transformed else 10].flat)
    assert all(type(v) is F for v in A.flat)
    # the integer products through `matmul`, counted: two per transformed low-rank block, two per dense entry
    from tests import dixon_multi_util as dm
    count = zu.CountingMatmul()
    A3, _, _ = rounding.linear_system(problem, Bs=Bs, assemble=lu.host_assemble, matmul=count)
    assert np.array_equal(A3, A) and len(count.calls) == ((2 + 2 * 3) if transformed else 0)
    # a selection of columns, one of them twice, in the given order
    cols = [len(index) - 1, 3, 0, 3, 17]
    A4, b4, index4 = rounding.linear_system(problem, Bs=Bs, columns=cols, assemble=lu.host_assemble)
    assert index4 == [index[c] for c in cols] and b4 == b and [list(r) for r in A4] == [[row[c] for c in cols] for row in rows]
    x, ok, finished = rounding.project_to_affine_space(A, b, batch=lu.host_hooks()["batch"], lift=lu.host_hooks()["lift"])
    assert ok and finished and all(sum((A[i, c] * x[c] for c in range(len(index))), F(0)) == b[i] for i in range(5))


# ---- select_columns ------------------------------------------------------------------------------------------------------------------------------------------------
def test_select_columns():
    problem = lu.handmade_problem()
    index = rounding.system_index(problem)
    assert rounding.select_columns(problem, -1) == list(range(len(index)))
    marked = [i for i, e in enumerate(index) if e[0] != "free" and e[2] - e[1] <= 1]
    assert len(marked) == 7 + 5 + 7
    objective = [False] * len(index)
    objective[2], objective[4], objective[-1] = True, True, True     # (0, 0, 2): not next to the diagonal; (0, 1, 1): on it; a free variable
    # 5 constraints, factor 10: all marked columns fit, those of the objective first, then max(8 * 5, 50 - 20) unmarked ones at random -- only 8 are left
    got = rounding.select_columns(index, 10, np.random.default_rng(1), nconstraints=5, objective=objective)
    assert got[:3] == [2, 4, len(index) - 1] and got[3:21] == [i for i in marked if i != 4] and sorted(got) == list(range(len(index)))
    # factor 3: K = 15 < 21 marked: a random 15 of them, the objective's first, and max(1 * 5, 0) unmarked
    got = rounding.select_columns(index, 3, np.random.default_rng(1), nconstraints=5, objective=objective)
    assert len(got) == 15 + 5 and len(set(got)) == 20
    n_obj = len([i for i in got[:15] if objective[i]])
    assert all(objective[i] for i in got[:n_obj]) and not any(objective[i] for i in got[n_obj:15])
    assert set(got[:15]) <= set(marked) | {2, len(index) - 1} and not set(got[15:]) & (set(marked) | {2, len(index) - 1})
    assert got != rounding.select_columns(index, 3, np.random.default_rng(2), nconstraints=5, objective=objective)
    assert got == rounding.select_columns(index, 3, np.random.default_rng(1), nconstraints=5, objective=objective)
    # from the problem itself: every C of the hand-made problem is dense, so every block entry is in the objective
    full = rounding.select_columns(problem, 10, np.random.default_rng(0))
    assert sorted(full) == list(range(len(index)))
    with pytest.raises(ValueError):
        rounding.select_columns(index, 3)
    s = rounding.RoundingSettings()
    assert (s.approximation_decimals, s.redundancyfactor) == (40, 10) and [f.name for f in __import__("dataclasses").fields(s)][-2:] == ["approximation_decimals", "redundancyfactor"]


# ---- the 320-bit oracle's solution of delsarte_exact(8, 3, 1/2) ------------------------------------------------------------------------------------------------------
class _Sol:
    def __init__(self, X, Y, y):
        self.X, self.Y, self.y = X, Y, y


@functools.lru_cache(maxsize=None)
def _oracle_solution():
    """the iterate of the 320-bit oracle at the top of its last iteration, in five limbs (the solve of tests/test_rationalize_cpu.py, run again for the
    snapshot, which carries the limbs the fp64 result does not)"""
    from oracle.oracle import Oracle
    f = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5))
    r = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=1e-40)
    assert r["error_code"] == 0 and abs(r["p_obj"] - 240) <= 1e-12
    r2 = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=1e-40, snapshots=[r["iterations"]], snapshot_limbs=5)
    assert r2["iterations"] == r["iterations"] and len(r2["snap"]["iters"]) == 1
    return _Sol(r2["snap"]["X"][0], r2["snap"]["Y"][0], np.zeros(0))


def test_conventions_on_the_oracle_solution(oracle_built):
    """the oracle's Y satisfies the untransformed full system: a wrong sign or a missing factor 2 leaves a residual of order one"""
    problem = P.delsarte_exact_problem(8, 3, F(1, 2))
    A, b, index = rounding.linear_system(problem, assemble=lu.host_assemble)
    assert A.shape == (7, 7 + 10 + 6)
    Y = rounding._exact_blocks(_oracle_solution().Y, problem.block_n)
    x = rounding.vectorize_solution(Y, [], index)
    resid = max(abs(sum((A[i, c] * x[c] for c in range(len(index))), F(0)) - b[i]) for i in range(7))
    print("delsarte_exact(8, 3, 1/2): max |A x - b| of the oracle's solution =", float(resid))
    assert resid <= F(1, 10 ** 20)
    objective = problem.constant + sum(Y[k][0, 0] for k in range(7))
    assert abs(objective - 240) <= F(1, 10 ** 20)


def test_exact_solution_of_delsarte_exact_on_the_host(oracle_built):
    problem = P.delsarte_exact_problem(8, 3, F(1, 2))
    settings = rounding.RoundingSettings(reduce_kernelvectors=False)
    hooks = lu.host_hooks()
    hooks["assemble"] = lu.Counting(lu.host_assemble)
    sol = rounding.exact_solution(problem, _oracle_solution(), settings, limbs=5, **hooks)
    lu.check_delsarte_exact_solution(problem, sol)
    assert [sol.Bs[k][2] for k in range(9)] == [1, 0, 0, 0, 0, 0, 0, 4, 2]
    assert len(sol.certificates) == 7 and len(hooks["assemble"].calls) == 1          # a_1 .. a_6 and B; the block A gives no columns and no call
    kept = rounding.exact_solution(problem, _oracle_solution(), settings, limbs=5, transformed=True, **lu.host_hooks())
    assert [M.shape[0] for M in kept.Y] == [0, 1, 1, 1, 1, 1, 1, 0, 1] and kept.objective == 240 and kept.Y[8][0, 0] > 0
    with pytest.raises(NotImplementedError):
        rounding.exact_solution(problem, _oracle_solution(), limbs=5, **lu.host_hooks())

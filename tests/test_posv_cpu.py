"""CPU side of the multi-word SPD solve (clrs_mw_posv, csrc/clrs_mw_posv.hip.h): its host restatement (tests/mw_host/mw_posv_host.cpp: the plan of the
library walked on the host, the diagonal blocks by the text the kernel compiles) against mpmath, planted failing pivots, the binding and the prototypes, and
the refusals of the library itself, which come before any device call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from clrs_amd import _lib
from tests import posv_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1          # CLRS_ERR_INVALID


@pytest.mark.parametrize("kind,K,n,nrhs", pu.cases(), ids=lambda v: str(v))
def test_restatement_against_mpmath(kind, K, n, nrhs):
    """eta = ||M x - r||_inf / (||M||_inf ||x||_inf + ||r||_inf), residual in mpmath at 4 x 53 K bits, at most 16 x the worst value measured per limb count
    (posv_util.WORST); that bound is below n 2^(-53 (K - 1)).  X and info are written where they should be and nowhere else."""
    s = pu.system(kind, K, n, nrhs)
    X, info = pu.run_host(s)
    assert info.tolist() == [0, (n + 15) // 16] + [-77] * 5
    assert np.all(X[:, n * nrhs:] == pu.SENTINEL) and np.all(np.isfinite(X))
    eta = s.eta(X)
    print(kind, "K", K, "n", n, "nrhs", nrhs, "log2 eta %.2f" % (math.log2(eta) if eta else -math.inf), "log2 bound %.2f" % math.log2(pu.bound(K, n)))
    assert eta <= pu.bound(K, n)


@pytest.mark.parametrize("col", pu.PLANTS)
def test_planted_failing_pivot_is_named_and_x_is_zero(col):
    s = pu.planted(col)
    X, info = pu.run_host(s)
    assert info[0] == 1 + col and info[1] == 4
    assert np.all(X[:, :s.n * s.nrhs] == 0.0) and np.all(X[:, s.n * s.nrhs:] == pu.SENTINEL)


def test_columns_do_not_depend_on_the_other_right_hand_sides():
    s = pu.system("spd", 5, 33, 3)
    X, _ = pu.run_host(s)
    n = s.n
    for c in range(3):
        one = pu.System.__new__(pu.System)
        one.K, one.n, one.nrhs, one.A, one.B = s.K, n, 1, s.A, np.ascontiguousarray(s.B[:, c * n:(c + 1) * n])
        Xc, _ = pu.run_host(one)
        assert np.array_equal(Xc[:, :n].view(np.uint64), X[:, c * n:(c + 1) * n].view(np.uint64))


def test_lib_binds_the_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const double *": _lib.p_d, "double *": _lib.p_d, "int32_t *": _lib.p_i32}
    names = {"clrs_mw_posv": ["device", "limbs", "n", "nrhs", "A", "a_plane", "B", "b_plane", "X", "x_plane", "info"],
             "clrs_mw_posv_times": ["diag_ms", "gemm_ms", "whole_ms"]}
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    for sym, want_names in names.items():
        ret, args = re.search(r"^\s*(\w+)\s+" + sym + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")] == want_names
        want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
        assert ret == "int" and _lib.SYMBOLS[sym] == (C.c_int, want)
    assert ":clrs_mw_posv," in jl and "function posv(" in jl


def test_refusals_come_before_any_device_call_and_leave_the_outputs_untouched():
    """every refusal of the issue through the library itself (no GPU is needed: nothing is launched), X and info full of sentinels before and after"""
    L = _lib.load()
    s = pu.system("spd", 5, 15, 3)
    A, B, X, info = pu.padded(s)
    X0, info0 = X.copy(), info.copy()

    def call(limbs=5, n=s.n, nrhs=s.nrhs, a=A, ap=A.shape[1], b=B, bp=B.shape[1], x=X, xp=X.shape[1], i=info):
        return L.clrs_mw_posv(0, limbs, n, nrhs, None if a is None else pu._dp(a), ap, None if b is None else pu._dp(b), bp,
                              None if x is None else pu._dp(x), xp, None if i is None else i.ctypes.data_as(_lib.p_i32))
    refused = [("limbs = 3", dict(limbs=3)), ("limbs = 7", dict(limbs=7)), ("limbs = 0", dict(limbs=0)), ("n < 0", dict(n=-1)), ("nrhs < 0", dict(nrhs=-1)),
               ("a_plane", dict(ap=s.n * s.n - 1)), ("b_plane", dict(bp=s.n * s.nrhs - 1)), ("x_plane", dict(xp=s.n * s.nrhs - 1)),
               ("a_plane < 0", dict(ap=-1)), ("null A", dict(a=None)), ("null B", dict(b=None)), ("null X", dict(x=None)), ("null info", dict(i=None))]
    for what, kw in refused:
        assert call(**kw) == INVALID, what
        assert L.clrs_last_error().startswith(b"posv"), what
        assert np.array_equal(X, X0) and np.array_equal(info, info0), what
    # n = 0 or nrhs = 0: nothing to do, nothing touched, null pointers allowed
    assert call(n=0, a=None, b=None, x=None, i=None) == 0 and call(nrhs=0, b=None, x=None, i=None) == 0
    assert np.array_equal(X, X0) and np.array_equal(info, info0)
    d = C.c_double()
    assert L.clrs_mw_posv_times(None, C.byref(d), C.byref(d)) == INVALID and L.clrs_mw_posv_times(C.byref(d), C.byref(d), C.byref(d)) == 0


def test_mw_posv_checks_its_operands_and_host_solve_names_the_column():
    from clrs_amd import mw
    with pytest.raises(ValueError, match="posv: operands must be planar"):
        mw.posv(np.zeros((6, 3, 3)), np.zeros((1, 3, 1)), 5)
    with pytest.raises(ValueError, match="posv: operands must be planar"):
        mw.posv(np.zeros((1, 3, 4)), np.zeros((1, 3, 1)), 5)
    with pytest.raises(ValueError, match="posv: operands must be planar"):
        mw.posv(np.zeros((1, 3, 3)), np.zeros((1, 4, 1)), 5)
    s = pu.planted(16)
    n = s.n
    A3 = np.transpose(s.A.reshape(s.K, n, n), (0, 2, 1))
    B3 = np.transpose(s.B.reshape(s.K, s.nrhs, n), (0, 2, 1))
    with pytest.raises(ArithmeticError, match="column 16"):
        pu.host_solve(A3, B3, s.K)
    g = pu.system("spd", 5, 17, 3)
    X3, info = pu.host_solve(np.transpose(g.A.reshape(5, 17, 17), (0, 2, 1))[:3], np.transpose(g.B.reshape(5, 3, 17), (0, 2, 1)), 5)
    assert X3.shape == (5, 17, 3) and info.tolist() == [0, 2]

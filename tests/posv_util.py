"""Shared by tests/test_posv_cpu.py and tests/test_posv_gpu.py: the host restatement of the multi-word SPD solve (tests/mw_host/mw_posv_host.cpp: the
plan of clrs_mw_posv walked on the host, its diagonal blocks by the text the kernel compiles), the systems of the issue, and the normwise backward error

    eta = ||M x - r||_inf / (||M||_inf ||x||_inf + ||r||_inf)

with the residual in mpmath at four times the bits of the limbs.  WORST[K] is the largest eta measured over all systems below per limb count
(DESIGN.md section 26); the tests bound eta by 16 WORST[K], and that bound is below n 2^(-53 (K - 1)) for every n here (asserted)."""
import ctypes as C
import functools
import os
import subprocess
import zlib

import mpmath as mp
import numpy as np

from clrs_amd import _lib
from tests.test_mw_arith_cpu import from_limbs, rand_values, to_limbs

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_posv_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_posv_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
LIMBS = (4, 5, 6, 8, 10)
SIZES = (1, 15, 16, 17, 33, 49)
NRHS = (1, 3)
SENTINEL = -7.25
PLANTS = (0, 7, 15, 16, 40)          # columns of the failing pivots planted in a 49 x 49 matrix
# the largest eta measured per limb count over cases() (host restatement; the device gives the same bits)
WORST = {4: 2.0 ** -210.27, 5: 2.0 ** -261.88, 6: 2.0 ** -313.09, 8: 2.0 ** -418.24, 10: 2.0 ** -524.82}


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_mw_posv.hip.h", "clrs_mw_gemm.hip.h", "clrs_mw_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mw_posv_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_d, C.c_int, _lib.p_d, C.c_int, _lib.p_d, C.c_int, _lib.p_i32]
    L.mw_posv_host.restype = C.c_int
    return L


def _dp(a):
    return a.ctypes.data_as(_lib.p_d)


def planes_of(rows, K):
    """list of rows of mpmath numbers -> planar (K, rows * cols), column-major"""
    r, c = len(rows), len(rows[0])
    return to_limbs([rows[i][j] for j in range(c) for i in range(r)], K)


class System:
    """M (n x n, symmetric) and R (n x nrhs) as limb planes, and the exact values the limbs hold (mpmath matrices)"""

    def __init__(self, K, M, R):
        mp.mp.prec = 53 * K + 64
        n, nrhs = len(M), len(R[0])
        self.K, self.n, self.nrhs = K, n, nrhs
        self.A, self.B = planes_of(M, K), planes_of(R, K)
        a, b = from_limbs(self.A), from_limbs(self.B)
        self.M = mp.matrix(n, n)
        self.R = mp.matrix(n, nrhs)
        for j in range(n):
            for i in range(n):
                self.M[i, j] = a[i + j * n]
        for j in range(nrhs):
            for i in range(n):
                self.R[i, j] = b[i + j * n]

    def eta(self, X):
        """the largest normwise backward error over the columns of the planar solution X (K, n * nrhs)"""
        K, n = self.K, self.n
        old = mp.mp.prec
        mp.mp.prec = 4 * 53 * K
        try:
            x = from_limbs(X)
            norm_m = max(mp.fsum(abs(self.M[i, j]) for j in range(n)) for i in range(n))
            worst = mp.mpf(0)
            for c in range(self.nrhs):
                xc = x[c * n:(c + 1) * n]
                res = max(abs(mp.fsum([self.M[i, j] * xc[j] for j in range(n)] + [-self.R[i, c]])) for i in range(n))
                den = norm_m * max(abs(v) for v in xc) + max(abs(self.R[i, c]) for i in range(n))
                worst = max(worst, res / den)
            return float(worst)
        finally:
            mp.mp.prec = old


def _gram(rng, n, K, rows=None, shift=None):
    """G^T G + shift I with G (rows x n) of full-limb random numbers of magnitude about 1"""
    rows = n if rows is None else rows
    g = [[v * mp.mpf(2) ** -int(mp.floor(mp.log(abs(v), 2))) for v in rand_values(rng, n, K)] for _ in range(rows)]
    M = [[mp.fsum(g[r][i] * g[r][j] for r in range(rows)) for j in range(n)] for i in range(n)]
    for i in range(n):
        M[i][i] += shift if shift is not None else mp.mpf(n)
    return M


@functools.lru_cache(maxsize=None)
def system(kind, K, n, nrhs):
    mp.mp.prec = 53 * K + 64
    rng = np.random.default_rng(zlib.crc32(repr((kind, K, n, nrhs)).encode()))
    if kind == "spd":
        M = _gram(rng, n, K)
    elif kind == "graded":                         # D M D with powers of two: diagonal entries between 2^-200 and 2^200
        M = _gram(rng, n, K)
        e = [int(v) for v in rng.integers(-100, 101, size=n)]
        if n > 1:
            e[0], e[-1] = 100, -100
        M = [[M[i][j] * mp.mpf(2) ** (e[i] + e[j]) for j in range(n)] for i in range(n)]
    elif kind == "normal":                         # B^T B + 1e-30 I with B 6 x 20: the regularised normal equations of a rank deficient system
        assert n == 20
        M = _gram(rng, n, K, rows=6, shift=mp.mpf(10) ** -30)
    else:
        raise ValueError(kind)
    R = [[v * mp.mpf(2) ** -int(mp.floor(mp.log(abs(v), 2))) for v in rand_values(rng, nrhs, K)] for _ in range(n)]
    return System(K, M, R)


def cases():
    """(kind, K, n, nrhs) of the issue: every size at 5 limbs, every limb count at n = 17, the normal equations at every limb count"""
    out = []
    for kind in ("spd", "graded"):
        out += [(kind, 5, n, r) for n in SIZES for r in NRHS]
        out += [(kind, K, 17, r) for K in LIMBS if K != 5 for r in NRHS]
    out += [("normal", K, 20, r) for K in LIMBS for r in NRHS]
    return out


def bound(K, n):
    b = 16 * WORST[K]
    assert b < n * 2.0 ** (-53 * (K - 1)), "the bound of the issue"
    return b


@functools.lru_cache(maxsize=None)
def planted(col, K=5, n=49):
    """the spd system of order n with the pivot of column `col` made to fail: M[col, col] is lowered to what the columns before it take away"""
    s = system("spd", K, n, 3)
    mp.mp.prec = 53 * K + 64
    Lc = mp.cholesky(s.M)
    M = [[s.M[i, j] for j in range(n)] for i in range(n)]
    M[col][col] = mp.fsum(Lc[col, r] ** 2 for r in range(col)) * (1 - mp.mpf(2) ** -20) - (mp.mpf(2) ** -30 if col == 0 else 0)
    return System(K, M, [[s.R[i, j] for j in range(s.nrhs)] for i in range(n)])


def padded(sysm, pad=5):
    """fresh (A, B, X, info) with planes `pad` longer than the matrices, sentinels in X, info and behind A and B"""
    K, n, nrhs = sysm.K, sysm.n, sysm.nrhs
    A, B = np.full((K, n * n + pad), np.nan), np.full((K, n * nrhs + pad), np.nan)
    A[:, :n * n], B[:, :n * nrhs] = sysm.A, sysm.B
    return A, B, np.full((K, n * nrhs + pad), SENTINEL), np.full(2 + pad, -77, dtype=np.int32)


def run_host(sysm, pad=5):
    A, B, X, info = padded(sysm, pad)
    assert host_lib().mw_posv_host(sysm.K, sysm.n, sysm.nrhs, _dp(A), A.shape[1], _dp(B), B.shape[1], _dp(X), X.shape[1], info.ctypes.data_as(_lib.p_i32)) == 0
    return X, info


def run_device(sysm, pad=5, device=0):
    A, B, X, info = padded(sysm, pad)
    _lib.check(_lib.load().clrs_mw_posv(device, sysm.K, sysm.n, sysm.nrhs, _dp(A), A.shape[1], _dp(B), B.shape[1], _dp(X), X.shape[1],
                                        info.ctypes.data_as(_lib.p_i32)))
    return X, info


def host_solve(A, B, limbs):
    """the stand-in for mw.posv on the host: planar (planes, n, n), (planes, n, nrhs) -> (X (limbs, n, nrhs), info)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, nrhs = A.shape[1], B.shape[2]
    Ap, Bp = np.zeros((limbs, max(n * n, 1))), np.zeros((limbs, max(n * nrhs, 1)))
    Ap[:A.shape[0], :n * n] = np.transpose(A, (0, 2, 1)).reshape(A.shape[0], -1)
    Bp[:B.shape[0], :n * nrhs] = np.transpose(B, (0, 2, 1)).reshape(B.shape[0], -1)
    X, info = np.zeros((limbs, max(n * nrhs, 1))), np.zeros(2, dtype=np.int32)
    assert host_lib().mw_posv_host(limbs, n, nrhs, _dp(Ap), Ap.shape[1], _dp(Bp), Bp.shape[1], _dp(X), X.shape[1], info.ctypes.data_as(_lib.p_i32)) == 0
    if info[0]:
        raise ArithmeticError(f"posv: the pivot of column {int(info[0]) - 1} is not positive")
    return np.ascontiguousarray(np.transpose(X[:, :n * nrhs].reshape(limbs, nrhs, n), (0, 2, 1))), info

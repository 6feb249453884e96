"""Shared by tests/test_modp_cpu.py and tests/test_modp_gpu.py: the restatement of the reduced row-echelon form mod p (plain Gauss-Jordan with numpy int64 and
Python's pow), the scalar arithmetic of csrc/clrs_modp_arith.h compiled for the host (tests/mw_host/modp_host.cpp), a host stand-in for the device call of the
Python layer, the invariants of a reduced row-echelon form, and the matrices of the tests."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

from clrs_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "modp_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmodp_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
PRIMES = (2, 10007, 8388593)          # the smallest, the reference's first, the largest below 2^23
SENTINEL = -7


def rref_mod_p(A, p, device=None):
    """Plain Gauss-Jordan over the integers mod p: (pivots, rank, R).  Column by column, the lowest row at or below the rank front that is non-zero there is
    exchanged to the front, scaled to 1 and cleared from every other row.  Entries may be Python integers of any size."""
    a = np.asarray(A)
    if a.size == 0:
        return np.zeros(0, np.int32), 0, np.zeros(a.shape if a.ndim == 2 else (0, 0), np.int32)
    if a.dtype == object:
        R = np.array([int(v) % p for v in a.flat], dtype=np.int64).reshape(a.shape)
    else:
        R = a.astype(np.int64) % p
    nrows, ncols = R.shape
    pivots, rank = [], 0
    for c in range(ncols):
        if rank == nrows:
            break
        hit = np.flatnonzero(R[rank:, c])
        if hit.size == 0:
            continue
        r = rank + int(hit[0])
        if r != rank:
            R[[rank, r]] = R[[r, rank]]
        R[rank] = R[rank] * pow(int(R[rank, c]), p - 2, p) % p           # (below 2^46)
        f = R[:, c].copy()
        f[rank] = 0
        rows = np.flatnonzero(f)
        R[rows] = (R[rows] - f[rows, None] * R[rank][None, :]) % p
        pivots.append(c)
        rank += 1
    return np.array(pivots, np.int32), rank, R.astype(np.int32)


def host_batch(A, p, device=0):
    """stand-in for `rounding.rref_mod_p` as the `batch` of find_pivots_modular / system_pivots"""
    piv, rank, _ = rref_mod_p(A, p)
    return piv, rank


def check_invariants(R, pivots, rank, p):
    """what makes R a reduced row-echelon form with these pivots, without a second implementation"""
    R = np.asarray(R)
    pivots = [int(c) for c in pivots]
    assert len(pivots) == rank and pivots == sorted(set(pivots))
    assert R.min(initial=0) >= 0 and R.max(initial=0) < p
    assert np.array_equal(R[:rank][:, pivots], np.eye(rank, dtype=R.dtype))
    assert not R[rank:].any()
    for i, c in enumerate(pivots):
        assert not R[i, :c].any()
    p2, r2, R2 = rref_mod_p(R, p)
    assert r2 == rank and list(p2) == pivots and np.array_equal(R2, R)


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC, os.path.join(_CSRC, "clrs_modp_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.modp_reduce_host.argtypes = [C.c_int, C.c_int, _lib.p_d, _lib.p_d]
    L.modp_inv_host.argtypes = [C.c_int, C.c_int, _lib.p_d, _lib.p_d]
    L.modp_mul_host.argtypes = [C.c_int, C.c_int, _lib.p_d, _lib.p_d, _lib.p_d]
    L.modp_is_prime_host.argtypes = [C.c_int]
    for f in (L.modp_reduce_host, L.modp_inv_host, L.modp_mul_host, L.modp_is_prime_host):
        f.restype = C.c_int
    return L


def _host_map(fn, p, *arrays):
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    out = np.zeros(arrays[0].size)
    assert fn(int(p), arrays[0].size, *[a.ctypes.data_as(_lib.p_d) for a in arrays], out.ctypes.data_as(_lib.p_d)) == 0
    return [int(v) for v in out]


def host_reduce(p, xs):
    return _host_map(host_lib().modp_reduce_host, p, xs)


def host_inv(p, xs):
    return _host_map(host_lib().modp_inv_host, p, xs)


def host_mul(p, xs, ys):
    return _host_map(host_lib().modp_mul_host, p, xs, ys)


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------------------
def random_matrix(rng, nrows, ncols, p, lo=0):
    return rng.integers(lo, p, size=(nrows, ncols), dtype=np.int64)


def random_invertible(rng, n, k, p):
    """n x k of full column rank mod p: random, redrawn until the restatement finds k pivots"""
    while True:
        M = random_matrix(rng, n, k, p)
        if rref_mod_p(M.T, p)[1] == k:
            return M


def planted(rng, nrows, ncols, pivot_cols, p, zero_cols=()):
    """(random invertible nrows x k) . (k x ncols echelon rows with pivots at `pivot_cols`, zero in `zero_cols`): rank k with exactly those pivots"""
    k = len(pivot_cols)
    E = random_matrix(rng, k, ncols, p)
    for i, c in enumerate(pivot_cols):
        E[i, :c] = 0
        E[:, c] = 0
        E[i, c] = 1
    E[:, list(zero_cols)] = 0
    return (random_invertible(rng, nrows, k, p).astype(object).dot(E.astype(object)) % p).astype(np.int64)


def example_system():
    """a consistent 3 x 5 system of Fractions, row 2 = row 0 + row 1: (A, b)"""
    F = Fraction
    A = [[F(1, 2), F(1, 3), 0, 1, 2], [0, F(2, 5), 1, F(1, 7), 0]]
    b = [F(3, 4), F(1, 2)]
    A.append([x + y for x, y in zip(A[0], A[1])])
    b.append(b[0] + b[1])
    return A, b

"""Shared by tests/test_dixon_cpu.py and tests/test_dixon_gpu.py: the restatement of Dixon's p-adic lifting in Python integers (`r = (r - A x) // p`, the
inverse mod p from tests/modp_util.rref_mod_p), an exact Gauss solve in Fractions, the bound and the reconstruction restated, the limb arithmetic of
csrc/clrs_modp_lift_arith.h compiled for the host (tests/mw_host/lift_host.cpp), and the systems of the tests."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction
from math import gcd, isqrt

import numpy as np

from clrs_amd import _lib
from tests import modp_util as mu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "lift_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "liblift_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
PMAX = 8388593                        # the largest prime below 2^23
HALF, BASE = 1 << 23, 1 << 24
SENTINEL = -7
BOUNDARY = [0, 1, -1, 2 ** 23 - 1, 2 ** 23, -2 ** 23, -2 ** 23 - 1, 2 ** 47 + 2 ** 23, -(2 ** 47 + 2 ** 23), 10 ** 40, -10 ** 40]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------
def objects(M):
    """a matrix or vector of Python integers as an object array"""
    a = np.asarray(M, dtype=object)
    out = np.empty(a.shape, dtype=object)
    out.flat = [int(v) for v in a.flat]
    return out


def inverse_mod_p(A, p):
    """(C, rank): C = A^-1 mod p as an object array from the reduced row-echelon form of [A mod p | I]; None when the rank of A mod p is below n"""
    A = objects(A)
    n = A.shape[0]
    res = np.array([[int(v) % p for v in row] for row in A], dtype=np.int64).reshape(n, n)
    piv, _, R = mu.rref_mod_p(np.concatenate([res, np.eye(n, dtype=np.int64)], axis=1), p)
    rank = int(sum(1 for c in piv if c < n))
    return (objects(R[:, n:]) if rank == n else None), rank


def lift(A, b, p, steps, device=0):
    """Plain Dixon lifting: (X, r, rank), X int32 (steps, n), r a list of Python integers; (None, None, rank) when A is singular mod p.  Also the `lift`
    stand-in of rounding.solve_dixon."""
    A, r = objects(A), objects(np.asarray(b, dtype=object).reshape(-1))
    n = A.shape[0]
    Cinv, rank = inverse_mod_p(A, p)
    if rank < n:
        return None, None, rank
    # the same formulas in numpy int64 where every intermediate fits: |r_k| <= max |b| + 2 n max |A|, |A x| < n max |A| p, C rbar < n p^2
    amax, bmax = max([abs(int(v)) for v in A.flat] + [1]), max([abs(int(v)) for v in r] + [1])
    if max(n * p * p, bmax + (2 + p) * n * amax) < 2 ** 62:
        A, r, Cinv = (a.astype(np.int64) for a in (A, r, Cinv))
    X = np.zeros((steps, n), np.int32)
    for k in range(steps):
        x = Cinv.dot(r % p) % p
        X[k] = [int(v) for v in x]
        t = r - A.dot(x)
        assert not any(int(v) % p for v in t)
        r = t // p
    return X, [int(v) for v in r], rank


def steps_and_bounds(A, b, p):
    """(K, N, D) restated: D2 = prod_c max(sum_r A[r, c]^2, 1), N2 = D2 max(sum b^2, 1), K the smallest integer with p^(2K) > 4 N2 D2"""
    A, b = objects(A), objects(np.asarray(b, dtype=object).reshape(-1))
    D2 = 1
    for c in range(A.shape[1]):
        D2 *= max(sum(int(v) ** 2 for v in A[:, c]), 1)
    N2 = D2 * max(sum(int(v) ** 2 for v in b), 1)
    K = 0
    while p ** (2 * K) <= 4 * N2 * D2:
        K += 1
    return K, isqrt(N2) + 1, isqrt(D2) + 1


def reconstruct(a, m, N, D):
    """the half-extended Euclid on (m, a mod m), stopped at the first remainder <= N"""
    r0, r1, t0, t1 = m, a % m, 0, 1
    while r1 > N:
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    if t1 == 0 or abs(t1) > D or gcd(r1, abs(t1)) != 1:
        return None
    return Fraction(r1, t1) if t1 > 0 else Fraction(-r1, -t1)


def horner(X, p):
    """sum_k X[k] p^k per column, Python integers"""
    x = [0] * X.shape[1]
    for k in range(X.shape[0] - 1, -1, -1):
        x = [v * p + int(w) for v, w in zip(x, X[k])]
    return x


def gauss_solve(A, b):
    """the exact solution of a square system in Fractions by Gauss-Jordan; None when singular"""
    n = len(A)
    M = [[Fraction(v) for v in A[i]] + [Fraction(b[i])] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [v - f * w for v, w in zip(M[r], M[c])]
    return [M[i][n] for i in range(n)]


def matvec(A, x):
    return [sum((Fraction(v) * w for v, w in zip(row, x)), Fraction(0)) for row in A]


# ---- the host build of clrs_modp_lift_arith.h --------------------------------------------------------------------------------------------------------------
p_ll = C.POINTER(C.c_longlong)


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC, os.path.join(_CSRC, "clrs_modp_lift_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.lift_split_host.argtypes = [C.c_int, C.c_int, p_ll, _lib.p_i32, p_ll]
    L.lift_div_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_i32, _lib.p_i32]
    L.lift_renorm_host.argtypes = [C.c_int, C.c_int, _lib.p_i32, p_ll]
    L.lift_residue_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_i32, _lib.p_i32]
    L.lift_power_table_host.argtypes = [C.c_int, C.c_int, _lib.p_i32]
    for f in (L.lift_split_host, L.lift_div_host, L.lift_renorm_host, L.lift_residue_host, L.lift_power_table_host):
        f.restype = C.c_int
    return L


_pi = lambda a: a.ctypes.data_as(_lib.p_i32)


def balanced(v, nl):
    """the nl balanced digits of the Python integer v (which must fit), restated"""
    out = []
    for _ in range(nl):
        d = ((v + HALF) % BASE) - HALF
        out.append(d)
        v = (v - d) // BASE
    assert v == 0
    return out


def value(limbs):
    return sum(int(d) << (24 * l) for l, d in enumerate(limbs))


def host_split(values, nl):
    vals = np.array(values, dtype=np.int64)
    digits, carry = np.zeros((len(values), nl), np.int32), np.zeros(len(values), np.int64)
    assert host_lib().lift_split_host(len(values), nl, vals.ctypes.data_as(p_ll), _pi(digits), carry.ctypes.data_as(p_ll)) == 0
    return digits, [int(c) for c in carry]


def host_div(p, limbs):
    limbs = np.ascontiguousarray(limbs, dtype=np.int32).copy()
    rem = np.zeros(limbs.shape[0], np.int32)
    assert host_lib().lift_div_host(p, limbs.shape[0], limbs.shape[1], _pi(limbs), _pi(rem)) == 0
    return limbs, rem


def host_renorm(limbs):
    limbs = np.ascontiguousarray(limbs, dtype=np.int32).copy()
    carry = np.zeros(limbs.shape[0], np.int64)
    assert host_lib().lift_renorm_host(limbs.shape[0], limbs.shape[1], _pi(limbs), carry.ctypes.data_as(p_ll)) == 0
    return limbs, [int(c) for c in carry]


def host_residue(p, limbs):
    limbs = np.ascontiguousarray(limbs, dtype=np.int32)
    out = np.zeros(limbs.shape[0], np.int32)
    assert host_lib().lift_residue_host(p, limbs.shape[0], limbs.shape[1], _pi(limbs), _pi(out)) == 0
    return [int(v) for v in out]


def host_lift(A, b, p, steps):
    """the lifting by the host build of the kernels' pieces (lift_step_host): (X, r as Python integers, counters)"""
    from clrs_amd import rounding
    A, b = objects(A), objects(np.asarray(b, dtype=object).reshape(-1))
    n = A.shape[0]
    Cinv, rank = inverse_mod_p(A, p)
    assert rank == n
    Cinv = np.ascontiguousarray(Cinv.astype(np.int64), dtype=np.int32)
    Ad, bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(b)
    nd, nbl = Ad.shape[0], bl.shape[0]
    nrl = max(nbl, nd + 1) + 1
    r = np.zeros((nrl + 1, n), np.int32)
    r[:nbl] = bl
    rbar = np.array([int(v) % p for v in b], dtype=np.int32)
    x, cnt, X = np.zeros(n, np.int32), np.zeros(2, np.int32), np.zeros((steps, n), np.int32)
    L = host_lib()
    L.lift_step_host.argtypes = [C.c_int] * 4 + [_lib.p_i32] * 6
    for k in range(steps):
        assert L.lift_step_host(n, nd, nrl, p, _pi(Cinv), _pi(Ad), _pi(r), _pi(rbar), _pi(x), _pi(cnt)) == 0
        X[k] = x
    assert not r[nrl].any()
    return X, [int(v) for v in rounding.from_balanced_digits(r[:nrl])], cnt.tolist()


# ---- systems ----------------------------------------------------------------------------------------------------------------------------------------------
def random_system(seed, n, bits, p, bbits=None, lo_entries=None):
    """(A, b) object arrays: entries uniform in (-2^bits, 2^bits) (or in [0, lo_entries)), drawn from a fixed seed and redrawn until A is invertible mod p"""
    rng = np.random.default_rng(seed)
    bbits = bits if bbits is None else bbits

    def draw(shape, nbits):
        words = (nbits + 29) // 30
        out = np.zeros(shape, dtype=object)
        for _ in range(words):
            out = out * (1 << 30) + rng.integers(0, 1 << 30, size=shape).astype(object)
        out = out % (1 << (nbits + 1)) - (1 << nbits)
        return objects(out)
    while True:
        A = objects(rng.integers(0, lo_entries, size=(n, n))) if lo_entries else draw((n, n), bits)
        if inverse_mod_p(A, p)[1] == n:
            break
    b = objects(rng.integers(0, lo_entries, size=n)) if lo_entries else draw((n,), bbits)
    return A, b


def extreme_system(n=65):
    """every entry -2^47 - 2^23, plus 3 on the diagonal: both digits of an off-diagonal entry are -2^23, the digit of largest magnitude, so the row sums are
    the largest two digits allow; b all ones"""
    A = np.full((n, n), -2 ** 47 - 2 ** 23, dtype=object)
    for i in range(n):
        A[i, i] += 3
    return objects(A), objects([1] * n)


def boundary_system(p):
    """16 x 16 with entries exactly at the digit boundaries, the diagonal shifted until A is invertible mod p"""
    n = 16
    A = objects([[BOUNDARY[(3 * i + 5 * j) % len(BOUNDARY)] for j in range(n)] for i in range(n)])
    shift = 0
    while inverse_mod_p(A, p)[1] < n:
        shift += 1
        for i in range(n):
            A[i, i] += 1
    b = objects([BOUNDARY[(i + 3) % len(BOUNDARY)] for i in range(n)])
    return A, b

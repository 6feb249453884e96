"""Shared by tests/test_dixon_multi_cpu.py and tests/test_dixon_multi_gpu.py: the per-entry residual update of csrc/clrs_modp_lift_arith.h (liftm_entry)
compiled for the host (tests/mw_host/liftm_host.cpp) and its restatement in Python integers, a host step loop built on it, the column-by-column stand-in
for the device lifting, counting stand-ins for the hooks, and a greedy exact-rank completion in Fractions."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

from clrs_amd import _lib, rounding
from tests import dixon_util as du

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "liftm_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libliftm_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
SENTINEL = du.SENTINEL
_pi = lambda a: a.ctypes.data_as(_lib.p_i32)


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC, os.path.join(_CSRC, "clrs_modp_lift_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.liftm_entry_host.argtypes = [C.c_int] * 4 + [_lib.p_d] + [_lib.p_i32] * 3
    L.liftm_step_host.argtypes = [C.c_int] * 5 + [_lib.p_i32] * 5 + [_lib.p_d, _lib.p_i32]
    L.liftm_entry_host.restype = L.liftm_step_host.restype = C.c_int
    return L


def host_entries(lo, hi, r, p):
    """liftm_entry on `count` entries: lo, hi (nd, count) integers, r (nrl + 1, count) int32 limbs -> (limbs after, residues, flags)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    nd, count = lo.shape
    P = np.ascontiguousarray(np.stack([lo, hi], axis=2))                  # [nd][count][2]
    r = np.ascontiguousarray(r, dtype=np.int32).copy()
    rbar, flags = np.zeros(count, np.int32), np.zeros(count, np.int32)
    assert host_lib().liftm_entry_host(count, nd, r.shape[0] - 1, int(p), P.ctypes.data_as(_lib.p_d), _pi(r), _pi(rbar), _pi(flags)) == 0
    return r, rbar, flags


def fits(v, nl):
    """whether the Python integer v has nl balanced digits"""
    for _ in range(nl):
        d = ((v + du.HALF) % du.BASE) - du.HALF
        v = (v - d) // du.BASE
    return v == 0


def entry_restated(lo, hi, limbs, p):
    """One entry in Python integers: t = value(limbs) - sum_l (lo_l + hi_l 2^24) 2^(24 l), q = floor(t / p).  Returns (balanced limbs of q or None when it
    overflows, q mod p, flags): bit 0 when p does not divide t, bit 1 when t does not fit in the nrl + 1 limbs or q does not fit in nrl."""
    nt = len(limbs)
    t = du.value(limbs) - sum((int(a) + (int(b) << 24)) << (24 * l) for l, (a, b) in enumerate(zip(lo, hi)))
    q = t // p
    over = not fits(t, nt) or not fits(q, nt - 1)
    flags = (1 if t % p else 0) | (2 if over else 0)
    return (None if over else du.balanced(q, nt - 1) + [0]), q % p, flags


def host_lift_multi(A, B, p, steps):
    """the lifting of all columns by the host build (liftm_step_host): (X (steps, n, m), R object (n, m), counters)"""
    A, B = du.objects(A), du.objects(B)
    n, m = B.shape
    Cinv, rank = du.inverse_mod_p(A, p)
    assert rank == n
    Cinv = np.ascontiguousarray(Cinv.astype(np.int64), dtype=np.int32)
    Ad, Bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(B)
    nd, nbl = Ad.shape[0], Bl.shape[0]
    nrl = max(nbl, nd + 1) + 1
    r = np.zeros((nrl + 1, n, m), np.int32)
    r[:nbl] = Bl
    rbar = np.ascontiguousarray(np.array([int(v) % p for v in B.flat], dtype=np.int32).reshape(n, m))
    x, cnt, X = np.zeros((n, m), np.int32), np.zeros(2, np.int32), np.zeros((steps, n, m), np.int32)
    P = np.zeros((nd, n * m, 2))
    for k in range(steps):
        assert host_lib().liftm_step_host(n, m, nd, nrl, p, _pi(Cinv), _pi(Ad), _pi(r), _pi(rbar), _pi(x), P.ctypes.data_as(_lib.p_d), _pi(cnt)) == 0
        X[k] = x
    assert not r[nrl].any()
    return X, rounding.from_balanced_digits(r[:nrl]), cnt.tolist()


def lift_columns(A, B, p, steps, device=0):
    """`dixon_util.lift` column by column: (X (steps, n, m), R object (n, m), rank); the `lift` stand-in of rounding.solve_dixon_multi"""
    A, B = du.objects(A), du.objects(B)
    n, m = B.shape
    cols = [du.lift(A, B[:, j], p, steps) for j in range(m)]
    if cols[0][0] is None:
        return None, None, cols[0][2]
    R = np.zeros((n, m), dtype=object)
    for j, c in enumerate(cols):
        R[:, j] = c[1]
    return np.ascontiguousarray(np.stack([c[0] for c in cols], axis=2)), R, cols[0][2]


class Counting:
    """a hook that counts its calls and remembers the shapes of its first two arguments"""

    def __init__(self, fn):
        self.fn, self.calls, self.shapes = fn, 0, []

    def __call__(self, *args, **kw):
        self.calls += 1
        self.shapes.append(tuple(np.asarray(a).shape for a in args[:2]))
        return self.fn(*args, **kw)


def host_matmul(A, B, device=0):
    return du.objects(np.asarray(A, dtype=object)).dot(du.objects(np.asarray(B, dtype=object)))


def host_reconstruct(X, p, N, D, device=0, want_x=False):
    """stand-in for rounding.dixon_reconstruct: Horner and the Euclid of dixon_util"""
    X = np.asarray(X)
    x = du.horner(X, p)
    sol = [du.reconstruct(v, p ** X.shape[0], N, D) for v in x]
    return (sol, x) if want_x else sol


def frac_rank(cols):
    """the rank over QQ of a list of vectors, by elimination in Fractions"""
    rows = [[Fraction(v) for v in c] for c in cols]
    rank = 0
    for c in range(len(rows[0]) if rows else 0):
        piv = next((r for r in range(rank, len(rows)) if rows[r][c] != 0), None)
        if piv is None:
            continue
        rows[rank], rows[piv] = rows[piv], rows[rank]
        for r in range(len(rows)):
            if r != rank and rows[r][c] != 0:
                f = rows[r][c] / rows[rank][c]
                rows[r] = [a - f * b for a, b in zip(rows[r], rows[rank])]
        rank += 1
    return rank


def greedy_completion(V):
    """the e_i, in ascending order, that are independent of the columns of V ((N, s)) and the e_j kept so far: the reference's loop, with exact ranks"""
    V = np.asarray(V, dtype=object)
    N, s = V.shape
    have = [list(V[:, c]) for c in range(s)]
    out = []
    for i in range(N):
        e = [Fraction(int(r == i)) for r in range(N)]
        if frac_rank(have + [e]) > len(have):
            have.append(e)
            out.append(i)
    return out


def frac_matmul(A, B):
    A, B = np.asarray(A, dtype=object), np.asarray(B, dtype=object)
    return [[sum((Fraction(A[i, k]) * Fraction(B[k, j]) for k in range(A.shape[1])), Fraction(0)) for j in range(B.shape[1])] for i in range(A.shape[0])]


def identity(n):
    return [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]


def random_rhs(seed, n, m, bits):
    rng = np.random.default_rng(seed)
    return du.objects(rng.integers(-(1 << bits) + 1, 1 << bits, size=(n, m)))

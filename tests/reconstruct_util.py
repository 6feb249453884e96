"""Shared by tests/test_reconstruct_cpu.py and tests/test_reconstruct_gpu.py: the limb arithmetic of csrc/clrs_modp_rec_arith.h compiled for the host
(tests/mw_host/reconstruct_host.cpp) behind Python wrappers, digits to and from Python integers restated, and the cases of the tests.  The oracle
everywhere is rounding.rational_reconstruction on Python integers."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction
from math import isqrt

import numpy as np

from clrs_amd import _lib, rounding

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "reconstruct_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libreconstruct_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
PMAX = 8388593
BASE = 1 << 24
SENTINEL = -7
p_ll = C.POINTER(C.c_longlong)
p_int = C.POINTER(C.c_int)
_pi = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32)


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC, os.path.join(_CSRC, "clrs_modp_rec_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    i, pi = C.c_int, _lib.p_i32
    L.rec_horner_host.argtypes = [i, i, i, pi, p_ll]
    L.rec_horner_lazy_host.argtypes = [i, i, i, pi, pi, pi, p_ll]
    L.rec_length_host.argtypes = [pi, i]
    L.rec_compare_host.argtypes = [pi, i, pi, i]
    L.rec_top_bits_host.argtypes = [pi, i, i, p_ll, p_int]
    L.rec_estimate_host.argtypes = [i, pi, i, pi, i, pi, p_int]
    L.rec_submul_host.argtypes = [pi, i, i, i, pi, i]
    L.rec_addmul_host.argtypes = [pi, i, i, i, i, pi, i]
    L.rec_residue_host.argtypes = [pi, i, i]
    L.rec_power_bound_host.argtypes = [i, i]
    L.rec_power_host.argtypes = [i, i, pi]
    L.rec_euclid_host.argtypes = [i, i, pi, pi, i, pi, i, pi, i, i, pi, pi, pi]
    for name in ("rec_horner_host", "rec_horner_lazy_host", "rec_length_host", "rec_compare_host", "rec_top_bits_host", "rec_estimate_host", "rec_submul_host",
                 "rec_addmul_host", "rec_residue_host", "rec_power_bound_host", "rec_power_host", "rec_euclid_host"):
        getattr(L, name).restype = C.c_int
    return L


# ---- digits, restated digit by digit -------------------------------------------------------------------------------------------------------------------------
def digits(v, count=None):
    """the little-endian digits in [0, 2^24) of the Python integer v >= 0 as int32: as many as v needs (at least one), or `count` (v must fit)"""
    out = []
    while v or not out:
        out.append(v % BASE)
        v //= BASE
    if count is not None:
        assert len(out) <= count
        out += [0] * (count - len(out))
    return np.array(out, dtype=np.int32)


def value(limbs):
    return sum(int(d) << (24 * l) for l, d in enumerate(limbs))


def length(v):
    """the number of limbs of v: 0 for 0"""
    return (int(v).bit_length() + 23) // 24


# ---- the host build, on Python integers ---------------------------------------------------------------------------------------------------------------------------
def host_estimate(r0, r1, window=False):
    """(c, s) of rec_quotient_estimate (or rec_quotient_window) for the Python integers r0 >= 0, r1 > 0"""
    a, b = digits(r0), digits(r1)
    c, s = np.zeros(1, np.int32), C.c_int(0)
    assert host_lib().rec_estimate_host(1 if window else 0, _pi(a), length(r0), _pi(b), length(r1), _pi(c), C.byref(s)) == 0
    return int(c[0]), s.value


def host_submul(r0, c, s, r1):
    """r0 - c 2^(24 s) r1 by rec_submul: (value, returned length); the value is None when the function reports a negative result"""
    a, b = digits(r0), digits(r1)
    n = host_lib().rec_submul_host(_pi(a), length(r0), c, s, _pi(b), length(r1))
    return (None if n < 0 else value(a)), n


def host_addmul(u0, c, s, u1, cap, junk=0):
    """u0 + c 2^(24 s) u1 by rec_addmul in a row of cap limbs whose limbs above u0 hold `junk`: (value of the first `returned length` limbs, that length)"""
    a = np.full(cap, junk, np.int32)
    a[:length(u0)] = digits(u0)[:length(u0)]
    b = digits(u1)
    n = host_lib().rec_addmul_host(_pi(a), length(u0), cap, c, s, _pi(b), length(u1))
    return (None if n < 0 else value(a[:n])), n


def host_euclid(a, p, K, N, D):
    """the host Euclid built from the pieces on (p^K, a): (Fraction or None, out) with out = [status, neg, steps, impossibilities, largest shift]"""
    m = p ** K
    Lm = length(m)
    nl = max(length(N), length(D), 1)
    md, xd, Nd, Dd = digits(m), digits(a), digits(N), digits(D)
    num, den, out = np.zeros(nl, np.int32), np.zeros(nl, np.int32), np.zeros(5, np.int32)
    assert host_lib().rec_euclid_host(p, Lm, _pi(md), _pi(xd), length(a), _pi(Nd), length(N), _pi(Dd), length(D), nl, _pi(num), _pi(den), _pi(out)) == 0
    if out[0]:
        assert not num.any() and not den.any()
        return None, out.tolist()
    return Fraction(-value(num) if out[1] else value(num), value(den)), out.tolist()


# ---- the device call ----------------------------------------------------------------------------------------------------------------------------------------------
def device_reconstruct(X, p, N, D, nl=None, nx=None, want_x=True):
    """one raw call of clrs_modp_dixon_reconstruct on sentinel-filled outputs: (code, num, den, neg, status, x_limbs, info)"""
    X = np.ascontiguousarray(X, dtype=np.int32)
    steps, n = X.shape
    Nd, Dd = digits(N), digits(D)
    nl = max(len(Nd), len(Dd)) if nl is None else nl
    nx = length(p ** steps) if nx is None else nx
    num, den = (np.full((n, nl), SENTINEL, np.int32) for _ in range(2))
    neg, status = (np.full(n, SENTINEL, np.int32) for _ in range(2))
    xl = np.full((n, nx), SENTINEL, np.int32) if want_x else None
    info = np.full(4, SENTINEL, np.int32)
    code = _lib.load().clrs_modp_dixon_reconstruct(0, n, int(p), steps, _pi(X), len(Nd), _pi(Nd), len(Dd), _pi(Dd), nl, _pi(num), _pi(den), _pi(neg), _pi(status),
                                                   nx, _pi(xl), _pi(info))
    return code, num, den, neg, status, xl, info


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------------
def padic_digits(a, p, K):
    """the K base-p digits of 0 <= a < p^K, lowest first, as a column (K, 1)"""
    out = np.zeros((K, 1), np.int32)
    for k in range(K):
        out[k, 0] = a % p
        a //= p
    assert a == 0
    return out


def horner(X, p):
    x = [0] * X.shape[1]
    for k in range(X.shape[0] - 1, -1, -1):
        x = [v * p + int(w) for v, w in zip(x, X[k])]
    return x


def big_random(rng, bound):
    """a Python integer uniform in [0, bound)"""
    words = (bound.bit_length() + 29) // 30 + 1
    v = 0
    for w in rng.integers(0, 1 << 30, size=words):
        v = (v << 30) | int(w)
    return v % bound


@functools.lru_cache(maxsize=None)
def mixed_case(p, K, n, seed=0):
    """(X (K, n) int32, kinds, N, D): entries alternately random residues (`kinds[i] = "random"`) and `num / den mod p^K` for a random fraction within the
    bounds N = D = isqrt(p^K // 2) - 1 (`"fraction"`: it reconstructs, m > 2 N D, unless D = 0 as for m = 2); n = 1 has one constructed entry."""
    rng = np.random.default_rng([p, K, n, seed])
    m = p ** K
    N = D = max(isqrt(m // 2) - 1, 0)
    X = np.zeros((K, n), np.int32)
    kinds = []
    for i in range(n):
        if i % 2 == 1:
            kinds.append("random")
            a = big_random(rng, m)
        else:
            kinds.append("fraction")
            while True:
                den = big_random(rng, D) + 1 if D > 0 else 1
                if den % p:
                    break
            num = big_random(rng, 2 * N + 1) - N
            a = num * pow(den, -1, m) % m
        X[:, i] = padic_digits(a, p, K)[:, 0]
    return X, tuple(kinds), N, D


def oracle(x, m, N, D):
    """(status, neg, |num|, den) per entry from rounding.rational_reconstruction"""
    out = []
    for v in x:
        f = rounding.rational_reconstruction(v, m, N, D)
        out.append((1, 0, 0, 0) if f is None else (0, 1 if f.numerator < 0 else 0, abs(f.numerator), f.denominator))
    return out


P67 = PMAX ** 67


def named_cases():
    """name -> (a, N, D, expected Fraction or None) at m = 8388593^67"""
    m, p = P67, PMAX
    B = isqrt(m // 2) - 1
    return {
        "a=0": (0, B, B, Fraction(0)),
        "a=1": (1, B, B, Fraction(1)),
        "a=m-1": (m - 1, B, B, Fraction(-1)),
        "1/3": (pow(3, -1, m), B, B, Fraction(1, 3)),
        "-22/7": (-22 * pow(7, -1, m) % m, B, B, Fraction(-22, 7)),
        "a=3, N=1": (3, 1, m, rounding.rational_reconstruction(3, m, 1, m)),
        "a=2^30+12345, N=2^20": (2 ** 30 + 12345, 2 ** 20, m, rounding.rational_reconstruction(2 ** 30 + 12345, m, 2 ** 20, m)),
        "a=p": (p, p - 1, m, None),
        "D one below": (-22 * pow(7, -1, m) % m, B, 6, None),
    }

"""Shared by tests/test_find_field_cpu.py and tests/test_find_field_gpu.py: csrc/clrs_minpoly_arith.h compiled for the host (tests/mw_host/minpoly_host.cpp,
g++ -ffp-contract=off), the planted numbers, an independent restatement of the reference's min_poly -> clindep (every rung from scratch, the `Fraction` LLL of
tests/lll_util.py, acceptance in mpmath) that shares no text with the header, and the mixed batch the device is compared with the host build on."""
import ctypes as C
import functools
import os
import subprocess

import mpmath as mp
import numpy as np

from clrs_amd import _lib, rounding
from clrs_amd.mw import from_limbs, to_limbs
from tests.lll_util import fraction_lll

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "minpoly_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libminpoly_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_minpoly_arith.h", "clrs_mw_field_round_arith.h", "clrs_zz_lll_arith.h", "clrs_modp_zz_arith.h",
                                                    "clrs_mw_arith.h")]
SENTINEL = -7
MP_PREC = 700
LAUNCH_RUNGS = 16                                        # FR_LAUNCH_RUNGS
TOTAL, PAD, ND = 193, 3, 6
_pi = lambda a: a.ctypes.data_as(_lib.p_i32)
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in _DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.minpoly_plan_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _lib.p_i32]
    L.minpoly_plan_host.restype = C.c_int
    L.minpoly_open_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_d, C.c_int, C.c_int, C.c_double, C.c_int]
    L.minpoly_open_host.restype = C.c_void_p
    L.minpoly_launch_host.argtypes = [C.c_void_p, C.c_int]
    L.minpoly_launch_host.restype = C.c_int
    L.minpoly_close_host.argtypes = [C.c_void_p, C.c_int, _lib.p_i32, _lib.p_i32, _lib.p_i32, _lib.p_d, _lib.p_i32]
    L.minpoly_close_host.restype = C.c_int
    return L


def host_plan(bits, limbs, deg, nd):
    out = np.zeros(7, np.int32)
    host_lib().minpoly_plan_host(bits, limbs, deg, nd, _pi(out))
    return dict(zip(("hdr", "launch_rungs", "max_nd", "P", "rungs", "nw", "elems"), (int(x) for x in out)))


def _pools(deg, plane, nd):
    """sentinel-filled outputs of a call"""
    p = max(plane, 1)
    return (np.full((nd, deg + 1, p), SENTINEL, np.int32), np.full(p, SENTINEL, np.int32), np.full(p, SENTINEL, np.int32), np.full(p, float(SENTINEL)),
            np.full((2, p), SENTINEL, np.int32))


def host_call(limbs, deg, count, v, plane, bits, errbound, nd, device=0, launch_rungs=LAUNCH_RUNGS):
    """the `call=` hook of rounding.minimal_polynomials on the host build; outputs pre-filled with sentinels"""
    v = np.ascontiguousarray(v, np.float64)
    rel, status, rung, err, info = _pools(deg, plane, nd)
    if count == 0:
        return rel, status, rung, err, info
    L, plan = host_lib(), host_plan(bits, limbs, deg, nd)
    h = L.minpoly_open_host(limbs, deg, count, _pd(v), plane, bits, errbound, nd)
    for _ in range(plan["rungs"] // launch_rungs + 2):
        running = L.minpoly_launch_host(h, launch_rungs)
        if not running:
            break
    assert running == 0
    L.minpoly_close_host(h, plane, _pi(rel), _pi(status), _pi(rung), _pd(err), _pi(info))
    return rel, status, rung, err, info


def device_call(limbs, deg, count, v, plane, bits, errbound, nd, device=0):
    """clrs_mw_minpoly with sentinel-filled outputs, the same shape of result as `host_call`"""
    v = np.ascontiguousarray(v, np.float64)
    rel, status, rung, err, info = _pools(deg, plane, nd)
    code = _lib.load().clrs_mw_minpoly(device, limbs, deg, count, _pd(v), plane, bits, errbound, nd, _pi(rel), _pi(status), _pi(rung), _pd(err), _pi(info))
    assert code == 0, (code, _lib.load().clrs_last_error())
    return rel, status, rung, err, info


def relation_of(out, i):
    """the relation of number i of a call's result as Python ints, low to high"""
    return [int(x) for x in rounding.planes_to_ints(out[0][:, :, i:i + 1])[:, 0]]


# ---- the planted numbers -------------------------------------------------------------------------------------------------------------------------------------
def _numbers():
    with mp.workprec(MP_PREC):
        return {"sqrt2": (mp.sqrt(2), [-2, 0, 1]), "golden": ((1 + mp.sqrt(5)) / 2, [-1, -1, 1]), "cbrt2": (mp.cbrt(2), [-2, 0, 0, 1]),
                "x4-x-1": (mp.findroot(lambda x: x ** 4 - x - 1, 1.2), [-1, -1, 0, 0, 1]), "sqrt2+sqrt3": (mp.sqrt(2) + mp.sqrt(3), [1, 0, -10, 0, 1]),
                "3/7": (mp.mpf(3) / 7, [-3, 7])}


PLANTED = _numbers()


def planes(xs, limbs):
    with mp.workprec(MP_PREC):
        return to_limbs([x() if callable(x) else x for x in xs], limbs)


def up_to_sign(a):
    a = [int(x) for x in a]
    return a if (a[-1] > 0 or (a[-1] == 0 and next((x for x in reversed(a) if x), 1) > 0)) else [-x for x in a]


def generic_bits(deg, h):
    """the ladder's cut that keeps d + 1 generic reals short of a spurious relation of coefficient height h (tests/test_field_round_gpu._mixed)"""
    return (deg + 1) * (h + 8) - 6


# ---- the reference's formulation, independently ------------------------------------------------------------------------------------------------------------
def restated(values, deg, limbs, errbound, bits):
    """per number (relation low to high or None, rung): lindep on (1, v, .., v^deg) at 1, 6, 11, .. bits from scratch -- the lattice [I | floor(2^p u)], a
    `Fraction` LLL with the same (delta, eta), the first row -- accepted when |sum a_k u_k| < errbound in mpmath; the ladder ends at min(bits, 53 limbs - 16).
    The powers are those of the exact sum of the limbs."""
    out = []
    with mp.workprec(MP_PREC):
        for v in from_limbs(np.atleast_2d(values)):
            u, D, found = [mp.mpf(v) ** k for k in range(deg + 1)], deg + 1, (None, 0)
            for p in range(1, min(bits, 53 * limbs - 16) + 1, 5):
                A = [[int(i == j) for j in range(D)] + [int(mp.floor(mp.ldexp(u[i], p)))] for i in range(D)]
                a = [int(x) for x in fraction_lll(A)[0][:D]]
                if abs(mp.fsum(x * y for x, y in zip(a, u))) < errbound:
                    found = (a, p)
                    break
            out.append(found)
    return out


# ---- the mixed batch of the device comparison ------------------------------------------------------------------------------------------------------------------
def _planted_roots(deg, h, count, seed):
    """`count` numbers with a minimal polynomial of degree `deg` and coefficient height about 2^h: r + q s with s a fixed algebraic number of that degree and
    small rationals r, q (deg 1: rationals with numerator and denominator below 2^h)"""
    rng = np.random.default_rng([seed, deg, h])
    with mp.workprec(MP_PREC):
        s = {1: mp.mpf(1), 2: mp.sqrt(2), 3: mp.cbrt(2), 4: PLANTED["x4-x-1"][0]}[deg]
        out = []
        for _ in range(count):
            m = int(rng.integers(1, 2 ** h))
            out.append(mp.mpf(int(rng.integers(-2 ** h + 1, 2 ** h))) / m + (mp.mpf(int(rng.integers(1, 4))) / int(rng.integers(1, 4)) * s if deg > 1 else 0))
        return out


@functools.lru_cache(maxsize=None)
def mixed(deg, limbs):
    """193 numbers (and 3 of padding) whose first wave holds, side by side: 0, 1 and small integers (relations at the first rungs), numbers of degree `deg` of
    two heights (the taller accepted late), pi and e (no relation before the ladder, cut by `bits`, ends: status 1), NaN and Inf (2) and a number whose powers
    leave 2^22 (4).  Returns (values (limbs, 196), bits, errbound)."""
    heights = (2, 6)
    h = 4 * max(heights) + 8                                                      # (the minimal polynomial of r + q s has coefficients near r^deg)
    bits, eb = generic_bits(deg, h), 2.0 ** -(deg * (h + 8))                      # (d + 1 generic reals: a relation below 2^(-p d / (d + 1)) near p bits)
    vals = np.zeros((limbs, TOTAL + PAD))
    special = {0: 0.0, 1: 1.0, 2: -3.0, 5: np.nan, 9: np.inf, 13: 2.0 ** 23, 62: -np.inf, 64: 7.0, 100: np.nan}
    with mp.workprec(MP_PREC):
        pis = {3: mp.pi, 40: mp.e, 130: -mp.pi / 7}
        pools = [_planted_roots(deg, hh, TOTAL, seed=7) for hh in heights]
        for i in range(TOTAL):
            if i in special:
                vals[0, i] = special[i]
            elif i in pis:
                vals[:, i] = to_limbs([pis[i]], limbs)[:, 0]
            else:
                vals[:, i] = to_limbs([pools[i % len(heights)][i]], limbs)[:, 0]
    vals[:, TOTAL:] = 0.5                                                        # behind every count: must never be read into a result
    return vals, bits, eb


@functools.lru_cache(maxsize=None)
def mixed_host(deg, limbs):
    vals, bits, eb = mixed(deg, limbs)
    return host_call(limbs, deg, TOTAL, vals, TOTAL + PAD, bits, eb, ND)


def same(dev, host, count):
    """bit for bit on the first `count` entries of every row; sentinels behind them"""
    for name, d, h in zip(("rel", "status", "rung", "err", "info"), dev, host):
        assert d[..., :count].tobytes() == np.ascontiguousarray(h[..., :count]).tobytes(), name
        assert (d[..., count:] == SENTINEL).all(), name

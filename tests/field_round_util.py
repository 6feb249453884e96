"""Shared by tests/test_field_round_cpu.py and tests/test_field_round_gpu.py: csrc/clrs_mw_field_round_arith.h compiled for the host
(tests/mw_host/field_round_host.cpp, g++ -ffp-contract=off), the planted inputs (seeded), an independent restatement of the reference's clindep (every rung from
scratch, Nemo's rounding floor(2^p u + 1/2), the `Fraction` LLL of tests/lll_util.py, acceptance in mpmath) that shares no text with the header, and host
stand-ins for the device calls of `round_to_field` and `kernel_vectors(field=...)`."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction as F

import mpmath as mp
import numpy as np

from clrs_amd import _lib, rounding
from clrs_amd.mw import from_limbs, to_limbs
from tests.lll_util import fraction_lll

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "field_round_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libfield_round_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_mw_field_round_arith.h", "clrs_zz_lll_arith.h", "clrs_modp_zz_arith.h", "clrs_mw_arith.h")]
SENTINEL = -7
MP_PREC = 700                                            # every generator below is a root to this many bits: enough for 10 limbs
LAUNCH_RUNGS = 16                                        # FR_LAUNCH_RUNGS
_pi = lambda a: a.ctypes.data_as(_lib.p_i32)
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in _DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.field_round_plan_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _lib.p_i32]
    L.field_round_plan_host.restype = C.c_int
    L.field_round_open_host.argtypes = [C.c_int, C.c_int, _lib.p_d, C.c_int, _lib.p_d, C.c_int, C.c_int, C.c_double, C.c_int]
    L.field_round_open_host.restype = C.c_void_p
    L.field_round_launch_host.argtypes = [C.c_void_p, C.c_int]
    L.field_round_launch_host.restype = C.c_int
    L.field_round_state_host.argtypes = [C.c_void_p, _lib.p_i32, _lib.p_i32]
    L.field_round_state_host.restype = C.c_int
    L.field_round_close_host.argtypes = [C.c_void_p, C.c_int, _lib.p_i32, _lib.p_i32, _lib.p_i32, _lib.p_d, _lib.p_d, _lib.p_i32]
    L.field_round_close_host.restype = C.c_int
    return L


def host_plan(bits, limbs, deg, nd):
    """dict of the constants and the plan of a call: hdr, max_passes, max_exchanges, launch_rungs, max_nd, P, rungs, nw, elems"""
    out = np.zeros(9, np.int32)
    host_lib().field_round_plan_host(bits, limbs, deg, nd, _pi(out))
    return dict(zip(("hdr", "max_passes", "max_exchanges", "launch_rungs", "max_nd", "P", "rungs", "nw", "elems"), (int(x) for x in out)))


def _pools(limbs, deg, plane, nd):
    """sentinel-filled outputs of a call"""
    p = max(plane, 1)
    return (np.full((nd, deg + 1, p), SENTINEL, np.int32), np.full(p, SENTINEL, np.int32), np.full(p, SENTINEL, np.int32), np.full(p, float(SENTINEL)),
            np.full((limbs, p), float(SENTINEL)), np.full((2, p), SENTINEL, np.int32))


def host_call(limbs, deg, gpow, count, v, plane, bits, errbound, nd, device=0, launch_rungs=LAUNCH_RUNGS, trace=None):
    """the `call=` hook of rounding.round_to_field on the host build; outputs pre-filled with sentinels.  `trace(ws, gw, plan)` is called after every launch."""
    gpow, v = np.ascontiguousarray(gpow, np.float64), np.ascontiguousarray(v, np.float64)
    rel, status, rung, err, vq, info = _pools(limbs, deg, plane, nd)
    if count == 0:
        return rel, status, rung, err, vq, info
    L, plan = host_lib(), host_plan(bits, limbs, deg, nd)
    h = L.field_round_open_host(limbs, deg, _pd(gpow), count, _pd(v), plane, bits, errbound, nd)
    for _ in range(plan["rungs"] // launch_rungs + 2):
        running = L.field_round_launch_host(h, launch_rungs)
        if trace is not None:
            ws, gw = np.zeros((plan["elems"], count), np.int32), np.zeros((deg, plan["nw"]), np.int32)
            L.field_round_state_host(h, _pi(ws), _pi(gw))
            trace(ws, gw, plan)
        if not running:
            break
    assert running == 0
    L.field_round_close_host(h, plane, _pi(rel), _pi(status), _pi(rung), _pd(err), _pd(vq), _pi(info))
    return rel, status, rung, err, vq, info


def device_call(limbs, deg, gpow, count, v, plane, bits, errbound, nd, device=0):
    """clrs_mw_field_round with sentinel-filled outputs, the same shape of result as `host_call`"""
    gpow, v = np.ascontiguousarray(gpow, np.float64), np.ascontiguousarray(v, np.float64)
    rel, status, rung, err, vq, info = _pools(limbs, deg, plane, nd)
    code = _lib.load().clrs_mw_field_round(device, limbs, deg, _pd(gpow), count, _pd(v), plane, bits, errbound, nd, _pi(rel), _pi(status), _pi(rung), _pd(err),
                                           _pd(vq), _pi(info))
    assert code == 0, (code, _lib.load().clrs_last_error())
    return rel, status, rung, err, vq, info


def host_round(values, field, limbs, launch_rungs=LAUNCH_RUNGS, **kw):
    """rounding.round_to_field on the host build, no rescue"""
    return rounding.round_to_field(values, field, limbs, relations=False, call=functools.partial(host_call, launch_rungs=launch_rungs), **kw)


# ---- the fields and the planted inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field(name):
    """x2-5, x2-2, x3-2, x4-x-1 (its positive real root), x5-x-1 (its real root), and 3/2 passed off as a generator of degree 2"""
    with mp.workprec(MP_PREC):
        if name == "x2-5":
            return rounding.NumberField([-5, 0, 1], mp.sqrt(5))
        if name == "x2-2":
            return rounding.NumberField([-2, 0, 1], mp.sqrt(2))
        if name == "x3-2":
            return rounding.NumberField([-2, 0, 0, 1], mp.cbrt(2))
        if name == "x4-x-1":
            return rounding.NumberField([-1, -1, 0, 0, 1], mp.findroot(lambda x: x ** 4 - x - 1, 1.2))
        if name == "x5-x-1":
            return rounding.NumberField([-1, -1, 0, 0, 0, 1], mp.findroot(lambda x: x ** 5 - x - 1, 1.2))
        if name == "3/2":                                                      # bypasses NumberField's check: 3/2 is no root of x^2 - 5
            f = rounding.NumberField([-5, 0, 1], mp.sqrt(5))
            f.g = mp.mpf(3) / 2
            f.residual = lambda: mp.mpf(0)
            return f
    raise KeyError(name)


PLANTED = [("x2-5", 4), ("x2-5", 16), ("x2-5", 40), ("x2-2", 4), ("x2-2", 16), ("x2-2", 40), ("x3-2", 4), ("x3-2", 16), ("x4-x-1", 4), ("x4-x-1", 16)]


def planted_errbound(deg, h):
    return 2.0 ** -(deg * (h + 8))


def planted_limbs(deg, h):
    """the least limb count on offer with 53 limbs - 16 >= (deg + 1)(h + 8) + 16"""
    return next(K for K in rounding.LIMBS if 53 * K - 16 >= (deg + 1) * (h + 8) + 16)


def planted(name, h, count, limbs=None, seed=0):
    """`count` elements sum_k (n_k / m) g^k with |n_k|, m < 2^h: (coefficient tuples of Fractions, planar values (limbs, count))"""
    f = field(name)
    limbs = planted_limbs(f.degree, h) if limbs is None else limbs
    rng = np.random.default_rng([seed, h, f.degree, sum(map(ord, name))])
    elems = []
    for _ in range(count):
        m = int(rng.integers(1, 2 ** h))
        elems.append(tuple(F(int(rng.integers(-2 ** h + 1, 2 ** h)), m) for _ in range(f.degree)))
    return elems, element_values(elems, f, limbs)


def element_values(elems, f, limbs):
    with mp.workprec(MP_PREC):
        gp = f.power_values(prec=MP_PREC)
        vals = [mp.fsum(mp.mpf(x.numerator) * g / x.denominator for x, g in zip(e, gp)) for e in elems]
        return to_limbs(vals, limbs)


# ---- the reference's formulation, independently ------------------------------------------------------------------------------------------------------------
def restated(values, f, limbs, errbound, bits=1000):
    """per number (coefficient tuple or None, rung): lindep at 1, 6, 11, .. bits from scratch -- the lattice [I | floor(2^p u + 1/2)], a `Fraction` LLL, the
    first row -- accepted when |sum a_i u_i| < errbound in mpmath; the ladder ends at min(bits, 53 limbs - 16)"""
    out = []
    with mp.workprec(MP_PREC):
        gp = f.power_values(prec=MP_PREC)
        for v in from_limbs(np.atleast_2d(values)):
            u, D, found = [mp.mpf(v)] + gp, f.degree + 1, (None, 0)
            for p in range(1, min(bits, 53 * limbs - 16) + 1, 5):
                A = [[int(i == j) for j in range(D)] + [int(mp.floor(mp.ldexp(u[i], p) + mp.mpf(1) / 2))] for i in range(D)]
                a = [int(x) for x in fraction_lll(A)[0][:D]]
                if abs(mp.fsum(x * y for x, y in zip(a, u))) < errbound:
                    found = (tuple(F(-x, a[0]) for x in a[1:]) if a[0] else None, p)
                    break
            out.append(found)
    return out


def vq_error(vq, elems, f):
    """max over the numbers of |vq - element| / max(|element|, 1), vq the limbs a call returned"""
    with mp.workprec(MP_PREC):
        gp = f.power_values(prec=MP_PREC)
        worst = mp.mpf(0)
        for got, e in zip(from_limbs(vq), elems):
            want = mp.fsum(mp.mpf(x.numerator) * g / x.denominator for x, g in zip(e, gp))
            worst = max(worst, abs(mp.mpf(got) - want) / max(abs(want), 1))
        return worst


# ---- host stand-ins for kernel_vectors(field=...) -----------------------------------------------------------------------------------------------------------------
def host_gemm(jobs, limbs, device=0):
    """`gemm=` in mpmath: only op(A) op(B) with beta = 0 is needed"""
    out = []
    with mp.workprec(64 * limbs + 128):
        for A, B, Cm, ta, tb, alpha, beta in jobs:
            assert not ta and not tb and alpha == 1 and beta == 0
            a = np.array([from_limbs(A[:, i, :]) for i in range(A.shape[1])], dtype=object).reshape(A.shape[1], A.shape[2])
            b = np.array([from_limbs(B[:, i, :]) for i in range(B.shape[1])], dtype=object).reshape(B.shape[1], B.shape[2])
            c = a.dot(b)
            out.append(to_limbs(c, limbs).reshape(limbs, c.shape[0], c.shape[1]))
    return out


def host_field_batch(batch):
    """`round_batch=` of kernel_vectors: the elimination `batch` (e.g. kernel_vectors_util.host_batch), the host build of the rounding, the product in mpmath"""
    def run(block_n, X, Y, limbs, tau, use_dual, dual_max, round_errbound, field=None, bits=1000, device=0):
        return rounding.kernel_vectors_field_batch(block_n, X, Y, limbs, tau, use_dual, dual_max, round_errbound, field=field, bits=bits, device=device,
                                                   batch=batch, round=host_round, gemm=host_gemm)
    return run


# ---- the oracle's solutions of the two Delsarte problems over QQ(sqrt 5) ------------------------------------------------------------------------------------------
class Sol:
    def __init__(self, X, Y):
        self.X, self.Y = X, Y


DELSARTE = {"icosahedron": (3, 3, "1/mp.sqrt(5)", 12, [1] * 7 + [4, 3], {0: 1, 6: 1, 7: 3, 8: 1}, 11),
            "600-cell": (4, 9, "1/(mp.sqrt(5)-1)", 120, [1] * 19 + [10, 9], {0: 1, 12: 1, 19: 8, 20: 6}, 23)}


@functools.lru_cache(maxsize=None)
def delsarte_flat(name):
    import clrs_amd
    from clrs_amd import problems, sdp
    n, d, cos = DELSARTE[name][:3]
    with sdp.data_planes(6):
        return clrs_amd.flatten(problems.delsarte_exact(n, d, cos))


@functools.lru_cache(maxsize=None)
def oracle_iterate(name, gap):
    """(the 6-limb snapshot of the 320-bit oracle's last iterate at the gap threshold `gap`, the fp64 X, Y the same solve returns)"""
    from oracle.oracle import Oracle
    f = delsarte_flat(name)
    r = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=gap)
    assert r["error_code"] == 0 and abs(r["p_obj"] - DELSARTE[name][3]) <= 1e-9, (r["error_code"], r["p_obj"])
    r2 = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=gap, snapshots=[r["iterations"]], snapshot_limbs=6)
    assert r2["iterations"] == r["iterations"] and len(r2["snap"]["iters"]) == 1
    return Sol(r2["snap"]["X"][0], r2["snap"]["Y"][0]), Sol(r["X"], r["Y"])

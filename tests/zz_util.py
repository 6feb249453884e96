"""Shared by tests/test_zz_gemm_cpu.py and tests/test_zz_gemm_gpu.py: the oracle of the exact integer matrix product (Python integers), the digit operands of
the tests, the arithmetic of csrc/clrs_modp_zz_arith.h compiled for the host (tests/mw_host/zz_host.cpp), the stand-alone sanitizer build of the same file,
and a counting `matmul` stand-in for the front ends of clrs_amd.rounding."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from clrs_amd import _lib, rounding

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "zz_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libzz_host.so")
_MAIN = os.path.join(_HERE, "mw_host", "zz_host_san")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC, os.path.join(_CSRC, "clrs_modp_zz_arith.h")]
HALF, BASE = 1 << 23, 1 << 24
SENTINEL = -7
p_ll = C.POINTER(C.c_longlong)
_pi = lambda a: a.ctypes.data_as(_lib.p_i32) if a is not None else _lib.p_i32()
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------------------------
def digits_restated(values, count=None):
    """The definition of balanced base-2^24 digits, digit by digit on Python integers, independent of clrs_amd.rounding: d = ((v + 2^23) mod 2^24) - 2^23,
    v <- (v - d) / 2^24.  Any shape -> int32 (count, *shape); `count=None`: as many digits as the longest value needs (at least one); a value that does not
    fit in `count` digits is an AssertionError."""
    a = np.asarray(values, dtype=object)
    rows = []
    for v in a.flat:
        v, row = int(v), []
        while True:
            d = ((v + HALF) % BASE) - HALF
            row.append(d)
            v = (v - d) // BASE
            if v == 0 and (count is None or len(row) >= count):
                break
        rows.append(row)
    nd = max([len(r) for r in rows] + [1]) if count is None else count
    assert all(len(r) <= nd for r in rows), "a value does not fit"
    out = np.zeros((nd, len(rows)), np.int32)
    for e, row in enumerate(rows):
        out[:len(row), e] = row
    return out.reshape((nd,) + a.shape)


def values_of(planes):
    """digit planes (nd, *shape), digits anywhere in [-2^23, 2^23] -> the object array of the Python integers sum_l planes[l] 2^(24 l), by Horner: like
    `digits_restated` independent of clrs_amd.rounding"""
    planes = np.asarray(planes)
    out = np.zeros(planes.shape[1:], dtype=object)
    for l in range(planes.shape[0] - 1, -1, -1):
        out = out * BASE + planes[l].astype(object)
    return out


def exact_product(Ad, Bd):
    """the exact product of the matrices two stacks of digit planes stand for, as an object matrix"""
    return values_of(Ad).dot(values_of(Bd))


def digits_needed(exact):
    return digits_restated(exact).shape[0]


def expected_planes(exact, ndc):
    return digits_restated(exact, count=ndc)


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------------
def random_digits(seed, nd, rows, cols):
    """uniform digits in [-2^23, 2^23), with the four extremes planted"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-HALF, HALF, size=(nd, rows, cols)).astype(np.int32)
    flat = d.reshape(-1)
    for pos, v in zip(rng.integers(0, flat.size, size=min(8, flat.size)), [HALF, -HALF, HALF - 1, 1 - HALF] * 2):
        flat[pos] = v
    return d


def extreme_digits(seed, nd, rows, cols, mode):
    """every digit of magnitude 2^23 - 1: "random" signs, "equal" signs (all positive), or "mix": a third of the digits +-2^23 instead"""
    rng = np.random.default_rng(seed)
    shape = (nd, rows, cols)
    d = np.full(shape, HALF - 1, np.int64)
    if mode == "mix":
        d = np.where(rng.integers(0, 3, size=shape) == 0, HALF, d)
    if mode != "equal":
        d = d * rng.choice(np.array([-1, 1]), size=shape)
    return d.astype(np.int32)


# ---- the device call ---------------------------------------------------------------------------------------------------------------------------------------
def device_gemm(Ad, Bd, ndc, device=0):
    """(code, C, info): clrs_zz_gemm on digit planes, C and info filled with sentinels before the call"""
    Ad, Bd = np.ascontiguousarray(Ad, dtype=np.int32), np.ascontiguousarray(Bd, dtype=np.int32)
    (nda, m, k), (ndb, k2, n) = Ad.shape, Bd.shape
    assert k == k2
    Cd, info = np.full((ndc, m, n), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    code = _lib.load().clrs_zz_gemm(device, m, k, n, nda, _pi(Ad), ndb, _pi(Bd), ndc, _pi(Cd), _pi(info))
    return code, Cd, info


def device_times():
    t = np.zeros(3)
    assert _lib.load().clrs_zz_gemm_times(_pd(t[0:]), _pd(t[1:]), _pd(t[2:])) == 0
    return [float(v) for v in t]


def chunks_expected(nda, m, n, ndb, bound):
    """the ranges of digits of B clrs_zz_gemm takes under a bound of `bound` bytes: 16 nda m n bytes per digit, at least one digit per range"""
    dc = min(ndb, max(bound // (16 * nda * m * n), 1))
    return -(-ndb // dc)


# ---- the host build of clrs_modp_zz_arith.h -------------------------------------------------------------------------------------------------------------------
def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in _DEPS)


@functools.lru_cache(maxsize=None)
def host_lib():
    if _stale(_LIB):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.zz_constants_host.argtypes = [_lib.p_i32]
    L.zz_split_host.argtypes = [C.c_int, _lib.p_d, _lib.p_d, _lib.p_d, _lib.p_i32]
    L.zz_flush_cycle_host.argtypes = [C.c_int, _lib.p_i32, _lib.p_i32, C.c_double, C.c_double, _lib.p_d]
    L.zz_carry_host.argtypes = [C.c_int, C.c_int, p_ll, C.c_int, _lib.p_i32]
    L.zz_gemm_host.argtypes = [C.c_int] * 4 + [_lib.p_i32, C.c_int, _lib.p_i32, C.c_int, _lib.p_i32, C.c_int, _lib.p_i32]
    for f in (L.zz_constants_host, L.zz_split_host, L.zz_flush_cycle_host, L.zz_carry_host, L.zz_gemm_host):
        f.restype = C.c_int
    return L


def host_constants():
    out = np.zeros(4, np.int32)
    host_lib().zz_constants_host(_pi(out))
    return [int(v) for v in out]                    # [the most MFMAs between flushes, what the kernel takes, steps between flushes, digit bits]


def host_split(values):
    acc = np.array(values, dtype=np.float64)
    lo, c, bad = np.zeros_like(acc), np.zeros_like(acc), np.zeros(acc.size, np.int32)
    host_lib().zz_split_host(acc.size, _pd(acc), _pd(lo), _pd(c), _pi(bad))
    return lo, c, bad


def host_flush_cycle(a, b, rem=0.0, hi0=0.0):
    """(bad, accumulator before the flush, lo, hi) for len(a) / 4 MFMAs of the digit products a[i] b[i]"""
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    assert a.size == b.size and a.size % 4 == 0
    out = np.zeros(3)
    bad = host_lib().zz_flush_cycle_host(a.size // 4, _pi(a), _pi(b), float(rem), float(hi0), _pd(out))
    return bad, float(out[0]), float(out[1]), float(out[2])


def host_carry(S, ndc):
    """(digits (count, ndc), entries that do not fit) for the int64 sums S (count, ns)"""
    S = np.ascontiguousarray(S, dtype=np.int64)
    out = np.full((S.shape[0], ndc), SENTINEL, np.int32)
    over = host_lib().zz_carry_host(S.shape[0], S.shape[1], S.ctypes.data_as(p_ll), ndc, _pi(out))
    return out, over


def host_gemm(Ad, Bd, ndc, dc=None):
    """(code, C, info): the whole product by the host build of the kernels' pieces, `dc` digits of B per range (default: all)"""
    Ad, Bd = np.ascontiguousarray(Ad, dtype=np.int32), np.ascontiguousarray(Bd, dtype=np.int32)
    (nda, m, k), (ndb, _, n) = Ad.shape, Bd.shape
    Cd, info = np.full((ndc, m, n), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    code = host_lib().zz_gemm_host(m, k, n, nda, _pi(Ad), ndb, _pi(Bd), ndc, _pi(Cd), ndb if dc is None else dc, _pi(info))
    return code, Cd, info


def sanitizer_program():
    """the stand-alone program over zz_host.cpp (its own main), built with AddressSanitizer and UndefinedBehaviorSanitizer; returns its path.  The
    sanitizers' runtimes are linked into the program, so it runs the same whatever else the environment loads into a process"""
    if _stale(_MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DZZ_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-o", _MAIN, _SRC], check=True)
    return _MAIN


# ---- the cases of the GPU file (the CPU file runs the host build on the same ones) ----------------------------------------------------------------------------
EDGE_SIZES = (1, 15, 16, 17, 63, 64, 65)
K_SIZES = (1, 3, 4, 5, 16, 111, 112, 113, 123, 124, 125, 128, 129, 500)         # 112 = 7 x 16: where k_zz_gemm flushes; 124 = 31 x 4: the most it could wait
DIGIT_COUNTS = ((1, 1), (2, 3), (3, 2), (1, 40), (40, 1), (5, 5))


def shape_cases():
    """(name, Ad, Bd) for the shapes at the tile edges: m, n in EDGE_SIZES with k = 17, one and two digits"""
    out = []
    for nd in (1, 2):
        for i, m in enumerate(EDGE_SIZES):
            for j, n in enumerate(EDGE_SIZES):
                seed = 1000 * nd + 10 * i + j
                out.append((f"m{m}-n{n}-d{nd}", random_digits(seed, nd, m, 17), random_digits(seed + 500, nd, 17, n)))
    return out


def k_cases():
    """(name, Ad, Bd) across the flush boundary: m = n = 17, every digit of magnitude 2^23 - 1 with random or equal signs, and a mix with +-2^23"""
    out = []
    for k in K_SIZES:
        for mode in ("random", "equal", "mix"):
            out.append((f"k{k}-{mode}", extreme_digits(k, 1, 17, k, mode), extreme_digits(k + 7, 1, k, 17, mode)))
    return out


def digit_cases():
    return [(f"d{nda}x{ndb}", random_digits(nda, nda, 9, 21), random_digits(100 + ndb, ndb, 21, 7)) for nda, ndb in DIGIT_COUNTS]


def vector_case():
    """33 x 33 times a 33 x 1 vector of 300 digits: the shape of the check product of solve_dixon"""
    return "check-shape", random_digits(5, 2, 33, 33), random_digits(6, 300, 33, 1)


# ---- a stand-in for `matmul=` ----------------------------------------------------------------------------------------------------------------------------------
class CountingMatmul:
    """`matmul(A, B, device=...)` in Python integers; keeps the shapes of every call; `corrupt`: the number of the call (0-based) whose first entry is raised by 1"""

    def __init__(self, corrupt=None, inner=None):
        self.calls, self.corrupt, self.inner = [], corrupt, inner

    def __call__(self, A, B, device=0):
        a, b = np.asarray(A, dtype=object), np.asarray(B, dtype=object)
        assert all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in list(a.flat) + list(b.flat)), "matmul is given integers only"
        out = np.asarray(a.dot(b) if self.inner is None else self.inner(A, B, device=device), dtype=object)
        if self.corrupt == len(self.calls) and out.size:
            out = out.copy()
            out.flat[0] = int(out.flat[0]) + 1
        self.calls.append((a.shape, b.shape))
        return out

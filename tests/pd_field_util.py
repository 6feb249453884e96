"""Exact oracles for the positive-definiteness check over a number field (clrs_modp_minors_field, rounding.checkpd_field): the
arithmetic of QQ(g) = QQ[x] / (f) on tuples of `Fraction`s, the leading principal minors by Bareiss' elimination in that ring, their signs at a real root in
mpmath, a Python evaluation of M(r) mod p that feeds tests/pd_util.minors_mod as the host stand-in for `rounding.leading_minors_field_mod`, a host Frobenius
by powers of the companion matrix, the host build of csrc/clrs_modp_field_arith.h, and the planted matrices.  Everything is compared with `==`."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction as F
from math import gcd

import mpmath as mp
import numpy as np

from clrs_amd import _lib, rounding
from tests import pd_util as pu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "modp_field_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmodp_field_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_modp_field_arith.h", "clrs_modp_arith.h")]
SENTINEL = -77
MP_PREC = 700
_pi = pu._pi
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in _DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.ff_digits_host.argtypes = [C.c_int, C.c_int, _lib.p_i32]
    L.ff_digits_host.restype = C.c_double
    L.ff_residue_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_d, _lib.p_d, _lib.p_d]
    L.ff_residue_host.restype = C.c_int
    L.ff_field_host.argtypes = [C.c_int, C.c_int, _lib.p_d, _lib.p_d, _lib.p_d, C.c_int, _lib.p_d, _lib.p_d, _lib.p_d, _lib.p_d]
    L.ff_field_host.restype = C.c_int
    return L


# ---- the fields ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field(name):
    """the fields of tests/field_round_util.py, x2-5 at its negative root as well, and the non-monic 2x2-5"""
    with mp.workprec(MP_PREC):
        if name == "x2-5":
            return rounding.NumberField([-5, 0, 1], mp.sqrt(5))
        if name == "x2-5 negative root":
            return rounding.NumberField([-5, 0, 1], -mp.sqrt(5))
        if name == "x2-2":
            return rounding.NumberField([-2, 0, 1], mp.sqrt(2))
        if name == "x3-2":
            return rounding.NumberField([-2, 0, 0, 1], mp.cbrt(2))
        if name == "x4-x-1":
            return rounding.NumberField([-1, -1, 0, 0, 1], mp.findroot(lambda x: x ** 4 - x - 1, 1.2))
        if name == "2x2-5":
            return rounding.NumberField([-5, 0, 2], mp.sqrt(mp.mpf(5) / 2))
    raise KeyError(name)


FIELDS = ("x2-5", "x2-2", "x3-2", "x4-x-1", "2x2-5")


# ---- QQ[x] / (f) on tuples of Fractions ------------------------------------------------------------------------------------------------------------------------------
def el(f, *c):
    """the element c_0 + c_1 g + .. of the field with minimal polynomial f"""
    d = len(f) - 1
    return tuple(F(v) for v in c) + (F(0),) * (d - len(c))


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def mul(f, a, b):
    d = len(f) - 1
    t = [F(0)] * (2 * d - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(2 * d - 2, d - 1, -1):                            # g^k = -g^(k-d) sum_j (f_j / f_d) g^j
        c = t[k] / f[d]
        if c:
            for j in range(d):
                t[k - d + j] -= c * f[j]
    return tuple(t[:d])


def inverse(f, a):
    """a^-1: the solution y of (multiplication by a) y = 1 by Gauss-Jordan on Fractions"""
    d = len(f) - 1
    cols, g = [], el(f, 0, 1)
    cur = el(f, 1)
    for _ in range(d):
        cols.append(mul(f, a, cur))
        cur = mul(f, cur, g)
    A = [[cols[j][i] for j in range(d)] + [F(int(i == 0))] for i in range(d)]
    for c in range(d):
        piv = next(r for r in range(c, d) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        A[c] = [v / A[c][c] for v in A[c]]
        for r in range(d):
            if r != c and A[r][c] != 0:
                A[r] = [v - A[r][c] * w for v, w in zip(A[r], A[c])]
    return tuple(A[i][d] for i in range(d))


def power(f, a, e):
    out = el(f, 1)
    for _ in range(e):
        out = mul(f, out, a)
    return out


def bareiss_minors_field(f, M):
    """the leading principal minors of a square matrix of field elements, up to and including the first that is zero: Bareiss' fraction-free elimination
    in QQ[x] / (f), the division by the previous pivot as a multiplication by its inverse.  For a matrix over Z[g], f monic, every entry stays in Z[g]."""
    n = len(M)
    a = [[tuple(F(x) for x in e) for e in row] for row in M]
    out, prev_inv = [], None
    for k in range(n):
        out.append(a[k][k])
        if not any(a[k][k]):
            return out
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                v = sub(mul(f, a[i][j], a[k][k]), mul(f, a[i][k], a[k][j]))
                a[i][j] = v if prev_inv is None else mul(f, v, prev_inv)
        prev_inv = inverse(f, a[k][k])
    return out


def value(fld, e):
    """the element at the real root of the field, in mpmath at MP_PREC bits"""
    with mp.workprec(MP_PREC):
        return mp.fsum(mp.mpf(x.numerator) / x.denominator * fld.g ** j for j, x in enumerate(e))


def sign_at(fld, e):
    """-1, 0, 1: 0 for the zero element only; a non-zero value must stand clear of zero at MP_PREC bits (the planted values do: the smallest is near 1e-13)"""
    if not any(e):
        return 0
    with mp.workprec(MP_PREC):
        v = value(fld, e)
        assert abs(v) > mp.ldexp(sum(abs(x) for x in e), -MP_PREC // 2), "a planted value too close to zero for this oracle"
        return 1 if v > 0 else -1


def normal_form(fld, A):
    """(scale, lc, M): what checkpd_field is documented to form -- scale = L lc^(d-1) with L the least common denominator and lc = |leading coefficient|,
    and scale A as a matrix of elements (still in powers of g)"""
    f = fld.minpoly
    d, lc = len(f) - 1, abs(f[-1])
    L = 1
    for row in A:
        for e in row:
            for x in e:
                L = L * F(x).denominator // gcd(L, F(x).denominator)
    scale = L * lc ** (d - 1)
    return scale, lc, [[tuple(F(x) * scale for x in e) for e in row] for row in A]


def to_h_coordinates(lc, e):
    """sum_j x_j g^j = sum_j (x_j / lc^j) h^j for h = lc g: the integer coefficients, asserted integral"""
    out = [x / lc ** j for j, x in enumerate(e)]
    assert all(x.denominator == 1 for x in out), out
    return [int(x) for x in out]


def exact_certificate(fld, A):
    """(scale, minors in h coordinates up to the first that is <= 0 at the root, pd, failed_order) by the oracles above"""
    scale, lc, M = normal_form(fld, A)
    minors = bareiss_minors_field(fld.minpoly, M)
    kept, failed = [], None
    for k, m in enumerate(minors):
        kept.append(to_h_coordinates(lc, m))
        if sign_at(fld, m) <= 0:
            failed = k + 1
            break
    assert failed is not None or len(minors) == len(A)
    return scale, kept, failed is None, failed


# ---- the stand-ins -----------------------------------------------------------------------------------------------------------------------------------------------------
def evaluate_mod(coeff_matrices, r, p):
    """M(r) mod p = sum_j M_j r^j mod p on Python integers"""
    mats = [np.asarray(M, dtype=object) for M in coeff_matrices]
    n = mats[0].shape[0]
    return [[sum(int(M[i, j]) * pow(r, k, p) for k, M in enumerate(mats)) % p for j in range(n)] for i in range(n)]


def host_field_minors(coeff_matrices, primes, roots, device=0):
    """the stand-in for rounding.leading_minors_field_mod: the same interface; per pair the per-prime restatement of tests/pd_util.py on M(r) mod p"""
    host_field_minors.calls.append(len(primes))
    rows, brk = [], []
    for p, rr in zip(primes, roots):
        got = [pu.minors_mod(evaluate_mod(coeff_matrices, int(r), int(p)), int(p)) for r in rr]
        rows.append([g[0] for g in got])
        brk.append([g[1] for g in got])
    return np.array(rows, np.int32), np.array(brk, np.int32)


host_field_minors.calls = []


def host_frobenius(minpoly, p):
    """x^p mod (f, p) as the first column of the p-th power of the companion matrix of f mod p (square and multiply on matrices of Python integers): another
    formulation than rounding's polynomial powers and the header's table.  -1 throughout where p divides the leading coefficient."""
    d = len(minpoly) - 1
    if minpoly[-1] % p == 0:
        return [-1] * d
    inv = pow(minpoly[-1], -1, p)
    Cm = [[0] * d for _ in range(d)]                                  # column j: the coordinates of x x^j
    for j in range(d - 1):
        Cm[j + 1][j] = 1
    for i in range(d):
        Cm[i][d - 1] = -minpoly[i] * inv % p
    matmul = lambda X, Y: [[sum(X[i][k] * Y[k][j] for k in range(d)) % p for j in range(d)] for i in range(d)]
    R, B, e = [[int(i == j) for j in range(d)] for i in range(d)], Cm, p
    while e:
        if e & 1:
            R = matmul(R, B)
        B = matmul(B, B)
        e >>= 1
    return [R[i][0] for i in range(d)]


def roots_by_trial(minpoly, p):
    return [r for r in range(p) if sum(c * pow(r, j, p) for j, c in enumerate(minpoly)) % p == 0]


def device_field_minors(coeff_matrices, primes, roots, chunk_bytes=0, digits=None):
    """one raw call of clrs_modp_minors_field on sentinel-filled outputs: (code, minors, breakdown, info); `digits` (d, nd, n, n): the planes to pass instead"""
    L = _lib.load()
    if digits is None:
        a = np.array([[[int(v) for v in row] for row in np.asarray(M, dtype=object)] for M in coeff_matrices], dtype=object)
        digits = np.ascontiguousarray(np.swapaxes(rounding.to_balanced_digits(a), 0, 1))
    digits = np.ascontiguousarray(digits, np.int32)
    d, nd, n = digits.shape[0], digits.shape[1], digits.shape[2]
    pr, rt = np.ascontiguousarray(primes, np.int32), np.ascontiguousarray(roots, np.int32)
    minors, brk, info = np.full((pr.size, d, n), SENTINEL, np.int32), np.full((pr.size, d), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    assert L.clrs_config_set(b"modp_minors_chunk_bytes", int(chunk_bytes)) == 0
    try:
        code = L.clrs_modp_minors_field(0, n, d, nd, _pi(digits), pr.size, _pi(pr), _pi(rt), _pi(minors), _pi(brk), _pi(info))
    finally:
        assert L.clrs_config_set(b"modp_minors_chunk_bytes", 0) == 0
    return code, minors, brk, info


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------------------------------------
def random_elements(seed, f, rows, cols, size=3):
    rng = np.random.default_rng(seed)
    d = len(f) - 1
    return [[tuple(F(int(v)) for v in rng.integers(-size, size + 1, size=d)) for _ in range(cols)] for _ in range(rows)]


def gram(f, B, shift):
    """B^T B + shift I over the field"""
    n, m = len(B[0]), len(B)
    out = [[el(f, shift if i == j else 0) for j in range(n)] for i in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = out[i][j]
            for k in range(m):
                s = add(s, mul(f, B[k][i], B[k][j]))
            out[i][j] = out[j][i] = s
    return out


def random_coefficient_matrices(seed, d, n, bits):
    """d random symmetric integer matrices with entries below 2^bits in size: no positive definiteness, for the raw call"""
    return [pu.random_symmetric(seed + 31 * j, n, bits) for j in range(d)]


def ldlt(f, L, D):
    """L diag(D) L^T for a unit lower triangular L of field elements: the leading minors are the running products of D"""
    n = len(L)
    return [[functools.reduce(add, (mul(f, mul(f, L[i][k], D[k]), L[j][k]) for k in range(min(i, j) + 1))) for j in range(n)] for i in range(n)]


def unit_lower(seed, f, n, size=2):
    rng = np.random.default_rng(seed)
    d = len(f) - 1
    rnd = lambda: tuple(F(int(v)) for v in rng.integers(-size, size + 1, size=d))
    return [[el(f, 1) if i == j else (rnd() if j < i else el(f, 0)) for j in range(n)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def first_split_prime(name):
    p, r = rounding.split_primes(field(name), 1)
    return p[0], r[0]


@functools.lru_cache(maxsize=None)
def planted(name):
    """the planted matrices: name -> (field, matrix of coefficient tuples, pd, failed_order or None)"""
    if name.startswith("gram "):                                     # B^T B + I with B over Z[g] (halves for the non-monic field: denominators to clear)
        fld = field(name[5:])
        f, n = fld.minpoly, 7
        B = random_elements(11, f, n, n)
        if name[5:] == "2x2-5":
            B = [[tuple(x / 2 for x in e) for e in row] for row in B]
        return fld, gram(f, B, 1), True, None
    f5 = [-5, 0, 1]
    if name in ("g-2 at 5 of 8", "g-2 at 5 of 8, negative root"):    # one matrix, two embeddings, opposite answers
        D = [el(f5, 3)] * 8
        D[4] = el(f5, -2, 1)
        fld = field("x2-5" if name == "g-2 at 5 of 8" else "x2-5 negative root")
        return fld, ldlt(f5, unit_lower(21, f5, 8), D), name == "g-2 at 5 of 8", None if name == "g-2 at 5 of 8" else 5
    if name == "(g-2)^20 at 5 of 8":                                 # positive, about 2.9e-13: the sign needs refinement
        D = [el(f5, 1)] * 8
        D[4] = power(f5, el(f5, -2, 1), 20)
        return field("x2-5"), ldlt(f5, unit_lower(22, f5, 8, size=1), D), True, None
    if name == "zero minor 17 of 33":
        D = [el(f5, 1 + (k % 3), k % 2) for k in range(33)]
        D[16] = el(f5, 0)
        return field("x2-5"), ldlt(f5, unit_lower(23, f5, 33, size=1), D), False, 17
    if name == "negative minor 9 of 20":
        D = [el(f5, 2)] * 20
        D[8] = el(f5, 1, -1)                                         # 1 - sqrt 5 < 0
        return field("x2-5"), ldlt(f5, unit_lower(24, f5, 20, size=1), D), False, 9
    if name == "one pair breaks down at 5 of 8":                     # r0 - g: zero at the pair (p, r0) of the first split prime, not at its other root
        p, roots = first_split_prime("x2-5")
        D = [el(f5, 1)] * 8
        D[4] = el(f5, roots[0], -1)
        return field("x2-5"), ldlt(f5, unit_lower(25, f5, 8, size=1), D), True, None
    if name == "singular psd gram":                                  # B^T B with B (n - 1) x n over Z[cbrt 2]: rank n - 1
        fld = field("x3-2")
        n = 7
        return fld, gram(fld.minpoly, random_elements(26, fld.minpoly, n - 1, n), 0), False, n
    raise KeyError(name)


PLANTED = tuple("gram " + f for f in FIELDS) + ("g-2 at 5 of 8", "g-2 at 5 of 8, negative root", "(g-2)^20 at 5 of 8", "zero minor 17 of 33",
                                                  "negative minor 9 of 20", "one pair breaks down at 5 of 8", "singular psd gram")


@functools.lru_cache(maxsize=None)
def planted_exact(name):
    fld, A, _, _ = planted(name)
    return exact_certificate(fld, A)


@functools.lru_cache(maxsize=None)
def planted_host_certificate(name):
    """checkpd_field through both host stand-ins, computed once: (certificate, calls of the stand-in)"""
    fld, A, _, _ = planted(name)
    host_field_minors.calls.clear()
    cert = rounding.checkpd_field(A, fld, minors=host_field_minors)
    return cert, list(host_field_minors.calls)


def host_frobenius_many(minpoly, primes):
    """`host_frobenius` for many primes at once, the same powers of the companion matrix in int64 (a sum of d <= 4 products of residues is below 2^48):
    int64 (len(primes), d)"""
    d = len(minpoly) - 1
    pr = np.asarray(primes, dtype=np.int64)
    lc = np.array([int(minpoly[-1]) % int(p) for p in pr], dtype=np.int64)
    inv = np.array([pow(int(v), -1, int(p)) if v else 0 for v, p in zip(lc, pr)], dtype=np.int64)
    Cm = np.zeros((pr.size, d, d), np.int64)
    for j in range(d - 1):
        Cm[:, j + 1, j] = 1
    for i in range(d):
        Cm[:, i, d - 1] = (-(np.array([int(minpoly[i]) % int(p) for p in pr], dtype=np.int64) * inv) % pr) % pr
    mm = lambda X, Y: np.einsum("qik,qkj->qij", X, Y) % pr[:, None, None]
    R = np.broadcast_to(np.eye(d, dtype=np.int64), (pr.size, d, d)).copy()
    for b in range(22, -1, -1):
        R = mm(R, R)
        R = np.where(((pr >> b) & 1)[:, None, None] == 1, mm(R, Cm), R)
    out = R[:, :, 0].copy()
    out[lc == 0] = -1
    return out

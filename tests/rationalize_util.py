"""Shared by tests/test_rationalize_cpu.py and tests/test_rationalize_gpu.py: the rational rounding compiled for the host (tests/mw_host/mw_rational_host.cpp,
the same mw_cf_round / mw_from_ratio the kernel calls), its restatement with `fractions.Fraction` on the exact value of the limbs, the classes of inputs, a
host stand-in for the device call of `kernel_vectors(rationalize=True)`, and planted pairs that come with their exact integer matrices."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import mpmath as mp
import numpy as np

from clrs_amd import _lib
from clrs_amd.mw import to_limbs
from clrs_amd.rounding import vectors_to_fractions
from tests import kernel_vectors_util as ku

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_rational_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_rational_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
LIMBS = (4, 5, 6, 8, 10)
CAP = 2 ** 53
STEPS = 96
EPS = 1e-15


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_mw_rational.hip.h", "clrs_mw_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mw_rationalize_host.argtypes = [C.c_int, C.c_int, _lib.p_d, C.c_long, C.c_double, _lib.p_d, _lib.p_d, _lib.p_i32, _lib.p_d]
    L.mw_rationalize_host.restype = C.c_int
    return L


def host_rationalize(values, limbs, errbound=EPS):
    """mw_cf_round / mw_from_ratio of the host build over a planar pool (limbs, count): num, den, status, vq"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    assert v.ndim == 2 and v.shape[0] == limbs
    count = v.shape[1]
    num, den, status, vq = np.zeros(max(count, 1)), np.zeros(max(count, 1)), np.zeros(max(count, 1), np.int32), np.zeros((limbs, max(count, 1)))
    vp = v if count else np.zeros((limbs, 1))
    assert host_lib().mw_rationalize_host(limbs, count, vp.ctypes.data_as(_lib.p_d), max(count, 1), float(errbound), num.ctypes.data_as(_lib.p_d),
                                          den.ctypes.data_as(_lib.p_d), status.ctypes.data_as(_lib.p_i32), vq.ctypes.data_as(_lib.p_d)) == 0
    return num[:count], den[:count], status[:count], vq[:, :count]


def exact_value(limbs_of_one):
    """the exact sum of the limbs of one number as a Fraction (None where the head is not finite)"""
    if not np.isfinite(limbs_of_one[0]):
        return None
    return sum((Fraction(float(l)) for l in limbs_of_one), Fraction(0))


def cf_reference(x, errbound):
    """The rounding in the words of the issue, exact: the convergents p_k / q_k of |x|, the first with |q_k |x| - p_k| < errbound; status 1 where p or q
    reaches 2^53 or 96 steps pass first; status 2 for x = None.  Returns (num, den, status, [the |q |x| - p| examined])."""
    if x is None:
        return 0, 0, 2, []
    eps, negative, x = Fraction(errbound), x < 0, abs(x)
    p1, p2, q1, q2, r, seen = 1, 0, 0, 1, x, []
    for _ in range(STEPS):
        a = r.numerator // r.denominator
        p, q = a * p1 + p2, a * q1 + q2
        if p >= CAP or q >= CAP:
            return 0, 0, 1, seen
        e = abs(q * x - p)
        seen.append(e)
        if e < eps:
            return (-p if negative else p), q, 0, seen
        if r == a:
            return 0, 0, 1, seen
        r = 1 / (r - a)
        p1, p2, q1, q2 = p, p1, q, q1
    return 0, 0, 1, seen


def input_classes(K, seed, per_class=6):
    """[(class name, planar limbs (K, count))]: the classes of inputs of the issue (finite ones through `to_limbs`, so properly formed K-limb numbers)"""
    rng = np.random.default_rng(seed)
    out = []
    with mp.workprec(64 * K + 256):
        noise = lambda: mp.ldexp(mp.mpf(float(rng.uniform(-1, 1))), -100)

        def ratios(sign):
            vals = []
            for _ in range(per_class):
                q = int(rng.integers(1, 10 ** 6 + 1))
                p = int(rng.integers(0, 40 * q))
                vals.append(sign * mp.mpf(p) / q + noise())
            return vals
        out.append(("ratio plus noise", to_limbs(ratios(1) + [mp.mpf(1) / 10 ** 6 + noise(), mp.mpf(999999) / 10 ** 6 + noise(), mp.mpf(7) / 2 + noise()], K)))
        out.append(("zero", to_limbs([mp.mpf(0)], K)))
        out.append(("pure noise", to_limbs([noise() for _ in range(per_class)], K)))
        out.append(("negative", to_limbs(ratios(-1) + [mp.mpf(-3), mp.mpf(-1) / 3], K)))
        out.append(("integer", to_limbs([mp.mpf(int(v)) for v in rng.integers(1, 2 ** 52, per_class)] + [mp.mpf(2 ** 52), mp.mpf(1), mp.mpf(2 ** 53 - 1)], K)))
        out.append(("beyond the cap", to_limbs([mp.mpf(2 ** 53), mp.mpf(-2 ** 53), mp.mpf(2 ** 53) + mp.mpf(1) / 3, mp.mpf(3) * 2 ** 60, mp.mpf(10) ** 30], K)))
        out.append(("irrational", to_limbs([mp.sqrt(2), (1 + mp.sqrt(5)) / 2, -mp.sqrt(2)], K)))
    bad = np.zeros((K, 3))
    bad[0] = [np.nan, np.inf, -np.inf]
    out.append(("not finite", bad))
    return out


def drawn_pool(K, count, seed):
    """`count` numbers drawn from the classes, planar (K, count)"""
    allv = np.concatenate([v for _, v in input_classes(K, seed, per_class=12)], axis=1)
    rng = np.random.default_rng(seed + 1)
    return np.ascontiguousarray(allv[:, rng.integers(0, allv.shape[1], count)])


# ---- the host stand-in of the device call of kernel_vectors(rationalize=True) ----------------------------------------------------------------

def host_round_batch(block_n, X, Y, limbs, tau, use_dual, dual_max, round_errbound, device=0):
    """clrs_amd.rounding.kernel_vectors_rational_batch on the host: the mpmath elimination of tests/kernel_vectors_util.host_batch, the entries rounded by the
    host build of mw_cf_round, the second residual Y_b Vq_b as a plain product of the exact values."""
    out, off = ku.host_batch(block_n, X, Y, limbs, tau, use_dual, dual_max), 0
    for n, k in zip((int(v) for v in block_n), out):
        Yb = Y[:, off:off + n * n]
        off += n * n
        flat = np.ascontiguousarray(np.transpose(k.vectors, (0, 2, 1)).reshape(limbs, -1))           # column-major n x count
        num, den, status, vq = host_rationalize(flat, limbs, round_errbound)
        shape = lambda a: np.ascontiguousarray(a.reshape(k.count, n).T)
        k.num, k.den, k.round_status = shape(num), shape(den), shape(status)
        k.vectors_rounded = np.ascontiguousarray(np.transpose(vq.reshape(limbs, k.count, n), (0, 2, 1)))
        with mp.workprec(52 * limbs + 64):
            Ym = ku.block_mp(Yb, n)
            q = [[mp.mpf(int(k.num[i, v])) / int(k.den[i, v]) if k.den[i, v] else mp.mpf(0) for v in range(k.count)] for i in range(n)]
            k.round_resid_max = np.array([max(abs(float(mp.fsum(Ym[i][j] * q[j][v] for j in range(n)))) for i in range(n)) for v in range(k.count)],
                                         dtype=np.float64)
    return out


# ---- planted pairs with their exact integer matrices -----------------------------------------------------------------------------------------

def planted_pair_exact(n, r, K, seed):
    """`kernel_vectors_util.planted_pair` (the same draws in the same order, so the same pair) that also returns the exact integer matrices X0, Y0
    (sixteen times the rational blocks): X0 = M[:, :r] D M[:, :r]^T, Y0 = M^-T[:, r:] E M^-T[:, r:]^T, X0 Y0 = 0."""
    rng = np.random.default_rng(seed)
    L, Ut = ku._unit_triangular(rng, n, dense=min(r, 6) if r < n else 0), ku._unit_triangular(rng, n)
    U = [[Ut[j][i] for j in range(n)] for i in range(n)]
    M = [[sum(L[i][k] * U[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    Li, Uti = ku._int_inverse_unit_lower(L), ku._int_inverse_unit_lower(Ut)
    Mit = [[sum(Li[k][i] * Uti[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    d = [int(v) for v in rng.integers(8, 129, n)]
    X0 = [[sum(M[i][k] * d[k] * M[j][k] for k in range(r)) for j in range(n)] for i in range(n)]
    Y0 = [[sum(Mit[i][k] * d[k] * Mit[j][k] for k in range(r, n)) for j in range(n)] for i in range(n)]
    X, Y = ku.planted_pair(n, r, K, seed)
    return X, Y, X0, Y0


def exact_echelon_vectors(A0, branch, perm, rank):
    """The exact vectors of a block from the integer matrix that was eliminated (X0 in the dual branch, Y0 in the primal one) over the returned pivots
    perm[:rank]: W = A11^-1 A12 with Fractions, then the vectors as DESIGN.md section 12 places them.  n x count nested lists of Fractions."""
    n = len(A0)
    piv, rest = [int(p) for p in perm[:rank]], [int(p) for p in perm[rank:]]
    # solve A[piv, piv] W = A[piv, rest] by Gauss-Jordan over the rationals
    aug = [[Fraction(A0[i][j]) for j in piv] + [Fraction(A0[i][j]) for j in rest] for i in piv]
    for c in range(rank):
        s = next(i for i in range(c, rank) if aug[i][c] != 0)
        aug[c], aug[s] = aug[s], aug[c]
        d = aug[c][c]
        aug[c] = [v / d for v in aug[c]]
        for i in range(rank):
            if i != c and aug[i][c] != 0:
                f = aug[i][c]
                aug[i] = [a - f * b for a, b in zip(aug[i], aug[c])]
    W = [[aug[c][rank + a] for a in range(n - rank)] for c in range(rank)]
    count = rank if branch == "dual" else n - rank
    V = [[Fraction(0)] * count for _ in range(n)]
    if branch == "dual":
        for c in range(rank):
            V[piv[c]][c] = Fraction(1)
            for a in range(n - rank):
                V[rest[a]][c] = W[c][a]
    else:
        for a in range(n - rank):
            V[rest[a]][a] = Fraction(1)
            for c in range(rank):
                V[piv[c]][a] = -W[c][a]
    return V


# ---- delsarte_exact(8, 3, 1/2) ------------------------------------------------------------------------------------------------------------------

def check_delsarte_exact_kernel(blocks):
    """what the issue states for delsarte_exact(8, 3, 1/2): a_0, A (4 x 4) and B (3 x 3) have 1, 4 and 2 vectors, every entry rounds to 0 or +-1 with
    den = 1, the two vectors of B each sum to zero (the kernel is the complement of (1, 1, 1))"""
    assert [k.count for k in blocks] == [1, 0, 0, 0, 0, 0, 0, 4, 2]
    for k in blocks:
        assert np.all(k.round_status == 0) and np.all(k.den == 1) and np.all(np.isin(k.num, (-1.0, 0.0, 1.0)))
        assert np.all(k.round_resid_max <= 1e-10)
        assert (k.max_num, k.max_den) == ((1, 1) if k.count else (0, 0))
    a0, A, B = blocks[0], blocks[7], blocks[8]
    assert vectors_to_fractions(a0) == [[Fraction(1)]]
    fa = vectors_to_fractions(A)
    assert sorted(map(tuple, fa)) == sorted(tuple(Fraction(int(i == j)) for i in range(4)) for j in range(4))
    fb = vectors_to_fractions(B)
    assert len(fb) == 2 and all(sum(v) == 0 and any(v) for v in fb) and fb[0] != fb[1] and fb[0] != [-x for x in fb[1]]

"""Shared by tests/test_lll_cpu.py and tests/test_lll_gpu.py: the arithmetic of csrc/clrs_zz_lll_arith.h and the whole reduction of clrs_zz_lll compiled for
the host (tests/mw_host/lll_host.cpp, g++ -ffp-contract=off), exact checks in `Fraction`s (LLL-reducedness, determinant, rank), a `Fraction` LLL as a
stand-in for `reduce=`, and the lattices and kernel blocks both files run."""
import ctypes as C
import functools
import json
import os
import subprocess
from fractions import Fraction as F

import numpy as np

from clrs_amd import _lib, rounding

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "lll_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "liblll_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_zz_lll_arith.h", "clrs_modp_zz_arith.h", "clrs_mw_arith.h")]
SENTINEL = -7
DELTA, ETA = 0.99, 0.51                                  # what the kernel runs (FLINT's defaults)
CHECK_DELTA, CHECK_ETA = F(98, 100), F(52, 100)          # what the tests assert, exactly
LAUNCH_SWAPS = 1024                                      # LLL_LAUNCH_SWAPS of clrs_zz_lll.hip
_pi = lambda a: a.ctypes.data_as(_lib.p_i32)
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in _DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.lll_constants_host.argtypes = [_lib.p_i32]
    L.lll_entry_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_i32, _lib.p_d]
    L.lll_split_host.argtypes = [C.c_int, _lib.p_d, _lib.p_d, _lib.p_i32, _lib.p_i32, _lib.p_i32]
    L.lll_update_host.argtypes = [C.c_int, C.c_int, C.c_int, _lib.p_i32, C.c_int, _lib.p_d]
    L.lll_reduce_host.argtypes = [C.c_int, _lib.p_i32, _lib.p_i32, _lib.p_i32, C.c_int, _lib.p_i32, _lib.p_i32, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                  _lib.p_i32]
    for f in (L.lll_constants_host, L.lll_entry_host, L.lll_split_host, L.lll_update_host, L.lll_reduce_host):
        f.restype = C.c_int
    return L


def host_constants():
    out = np.zeros(8, np.int32)
    host_lib().lll_constants_host(_pi(out))
    return [int(v) for v in out]


def host_entries(values, limbs, nd):
    """the K-limb images of Python integers: (limbs, count) fp64"""
    digits = np.ascontiguousarray(rounding.ints_to_planes(np.array(list(values), dtype=object), nd))
    out = np.zeros((limbs, digits.shape[1]))
    assert host_lib().lll_entry_host(limbs, nd, digits.shape[1], _pi(digits), _pd(out)) == 0
    return out


def host_split(mus):
    """(X, xd (count, 4), sh, bad) for the quotients rint(mu)"""
    mu = np.array(mus, dtype=np.float64)
    X, xd, sh, bad = np.zeros_like(mu), np.zeros((mu.size, 4), np.int32), np.zeros(mu.size, np.int32), np.zeros(mu.size, np.int32)
    host_lib().lll_split_host(mu.size, _pd(mu), _pd(X), _pi(xd), _pi(sh), _pi(bad))
    return X, xd, sh, bad


def host_update(rows, k, X, nd):
    """b_k <- b_k - sum_{j < k} X_j b_j on an object matrix: (the new matrix or None when a column overflowed, the overflow count, the digits as left)"""
    A = np.asarray(rows, dtype=object)
    digits = np.ascontiguousarray(rounding.ints_to_planes(A, nd))
    Xd = np.array(X, dtype=np.float64)
    over = host_lib().lll_update_host(A.shape[0], A.shape[1], nd, _pi(digits), k, _pd(Xd))
    return (rounding.planes_to_ints(digits) if over == 0 else None), over, digits


def _pack(rows, cols, cols_gram, digits):
    rows, cols, cols_gram = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (rows, cols, cols_gram))
    return rows, cols, cols_gram, np.ascontiguousarray(digits, np.int32).reshape(-1)


def host_call(rows, cols, cols_gram, nd, digits, delta, eta, limbs, max_swaps, device=0, launch_swaps=LAUNCH_SWAPS):
    """the `call=` hook of rounding.lll_batch on the host build: (out, info (nb, 8)), out filled with sentinels where nothing was written"""
    rows, cols, cols_gram, digits = _pack(rows, cols, cols_gram, digits)
    out, info = np.full(max(digits.size, 1), SENTINEL, np.int32), np.full((max(rows.size, 1), 8), SENTINEL, np.int32)
    assert host_lib().lll_reduce_host(rows.size, _pi(rows), _pi(cols), _pi(cols_gram), nd, _pi(digits) if digits.size else _pi(out), _pi(out), delta, eta, limbs,
                                      max_swaps, launch_swaps, _pi(info)) == 0
    return out[:digits.size], info[:rows.size]


def device_call(rows, cols, cols_gram, nd, digits, delta, eta, limbs, max_swaps, device=0):
    """clrs_zz_lll with sentinel-filled outputs, the same shape of result as `host_call`"""
    rows, cols, cols_gram, digits = _pack(rows, cols, cols_gram, digits)
    out, info = np.full(max(digits.size, 1), SENTINEL, np.int32), np.full((max(rows.size, 1), 8), SENTINEL, np.int32)
    code = _lib.load().clrs_zz_lll(device, rows.size, _pi(rows), _pi(cols), _pi(cols_gram), nd, _pi(digits) if digits.size else _pi(out), _pi(out), delta, eta, limbs,
                                   max_swaps, _pi(info))
    assert code == 0, (code, _lib.load().clrs_last_error())
    return out[:digits.size], info[:rows.size]


def host_lll_batch(lattices, **kw):
    """rounding.lll_batch on the host build (a stand-in for `lll=` of reduce_kernel_vectors); keeps `last_info` like the original"""
    out = rounding.lll_batch(lattices, call=host_call, **kw)
    host_lll_batch.last_info = rounding.lll_batch.last_info
    return out


host_lll_batch.last_info = None


def host_reduce(blocks, settings=None, device=0, matmul=None):
    """`reduce=` on the host build"""
    return rounding.reduce_kernel_vectors(blocks, settings, device=device, matmul=matmul, lll=host_lll_batch)


# ---- exact checks ------------------------------------------------------------------------------------------------------------------------------------------
def gram_schmidt(rows, cols_gram=None):
    """(mu, r) of the rows over the first cols_gram columns, one Cholesky in Fractions: mu[i][j] for j < i, r[i] = |b_i*|^2"""
    A = [[int(v) for v in row] for row in np.asarray(rows, dtype=object)]
    g = len(A[0]) if cols_gram is None and A else cols_gram
    d = len(A)
    G = [[sum(A[i][c] * A[j][c] for c in range(g)) for j in range(i + 1)] for i in range(d)]
    mu, r = [[F(0)] * d for _ in range(d)], [F(0)] * d
    for i in range(d):
        rr = [F(0)] * (i + 1)
        for j in range(i + 1):
            rr[j] = F(G[i][j]) - sum((mu[j][t] * rr[t] for t in range(j)), F(0))
            if j < i:
                mu[i][j] = rr[j] / r[j] if r[j] != 0 else None
        r[i] = rr[i]
        if r[i] <= 0:
            return mu, r
    return mu, r


def is_lll_reduced(rows, delta=CHECK_DELTA, eta=CHECK_ETA, cols_gram=None):
    """exactly: every r_i > 0, every |mu_ij| <= eta, and delta r_{i-1} <= r_i + mu_{i,i-1}^2 r_{i-1}"""
    rows = np.asarray(rows, dtype=object)
    if rows.shape[0] == 0:
        return True
    mu, r = gram_schmidt(rows, cols_gram)
    d = len(r)
    if any(v <= 0 for v in r):
        return False
    if any(abs(mu[i][j]) > eta for i in range(d) for j in range(i)):
        return False
    return all(F(delta) * r[i - 1] <= r[i] + mu[i][i - 1] ** 2 * r[i - 1] for i in range(1, d))


def _eliminate(M):
    """(rank, determinant when square else None) by elimination in Fractions"""
    A = [[F(int(v)) if not isinstance(v, F) else v for v in row] for row in np.asarray(M, dtype=object)]
    n, m = len(A), len(A[0]) if A else 0
    det, rank = F(1), 0
    for c in range(m):
        piv = next((i for i in range(rank, n) if A[i][c] != 0), None)
        if piv is None:
            det = F(0)
            continue
        if piv != rank:
            A[piv], A[rank] = A[rank], A[piv]
            det = -det
        det *= A[rank][c]
        for i in range(rank + 1, n):
            if A[i][c] != 0:
                f = A[i][c] / A[rank][c]
                A[i] = [a - f * b for a, b in zip(A[i], A[rank])]
        rank += 1
        if rank == n:
            break
    return rank, (det if n == m and rank == n else (F(0) if n == m else None))


def det_fraction(M):
    return _eliminate(M)[1] if np.asarray(M, dtype=object).size else F(1)


def rank_fraction(M):
    return _eliminate(M)[0]


def matmul_int(A, B):
    return np.asarray(A, dtype=object).dot(np.asarray(B, dtype=object))


def assert_properties(A, out, U=None, cols_gram=None):
    """what every reduced lattice must satisfy: with U, U integral, |det U| = 1 and U A == out; out (0.98, 0.52)-reduced, exactly"""
    A, out = np.asarray(A, dtype=object), np.asarray(out, dtype=object)
    assert out.shape == A.shape
    if U is not None:
        U = np.asarray(U, dtype=object)
        assert all(isinstance(v, int) for v in U.flat)
        assert abs(det_fraction(U)) == 1
        assert (matmul_int(U, A) == out).all()
    assert is_lll_reduced(out, cols_gram=cols_gram)


# ---- a Fraction LLL: the stand-in for `reduce=` that shares nothing with the kernel's arithmetic ------------------------------------------------------------------
def fraction_lll(rows, delta=F(99, 100)):
    """textbook LLL with eta = 1/2, every number a Python integer or a Fraction; returns the reduced rows (an object matrix)"""
    B = [[int(v) for v in row] for row in np.asarray(rows, dtype=object)]
    d = len(B)
    dot = lambda x, y: sum(a * b for a, b in zip(x, y))
    mu, r = [[F(0)] * d for _ in range(d)], [F(0)] * d

    def row(k):
        rr = [F(0)] * (k + 1)
        for j in range(k + 1):
            rr[j] = F(dot(B[k], B[j])) - sum((mu[j][t] * rr[t] for t in range(j)), F(0))
            if j < k:
                mu[k][j] = rr[j] / r[j]
        r[k] = rr[k]

    k = 0
    while k < d:
        row(k)
        changed = False
        for j in range(k - 1, -1, -1):
            X = round(mu[k][j])
            if X:
                B[k] = [a - X * b for a, b in zip(B[k], B[j])]
                for t in range(j):
                    mu[k][t] -= X * mu[j][t]
                mu[k][j] -= X
                changed = True
        if changed:
            row(k)
        if k > 0 and r[k] + mu[k][k - 1] ** 2 * r[k - 1] < delta * r[k - 1]:
            B[k - 1], B[k] = B[k], B[k - 1]
            k -= 1
        else:
            k += 1
    out = np.empty((d, len(B[0]) if B else 0), dtype=object)
    for i in range(d):
        out[i] = B[i]
    return out


def fraction_reduce(blocks, settings=None, device=0, matmul=None):
    """`reduce=` restated in Fractions: the embedding of DESIGN.md section 22 through `fraction_lll`; the same verifications as asserts"""
    out = []
    for N, s, M, R in blocks:
        lattice, _ = rounding.kernel_lattice(N, s, M, R)
        red = fraction_lll(lattice)
        left, U = red[:, :N - s], red[:, N - s:]
        assert all(v == 0 for v in left[:s].flat) and all(any(v != 0 for v in left[i]) for i in range(s, N))
        assert all(v == 0 for v in matmul_int(M, U[:s].T).flat)
        out.append(U)
    return out


class Recording:
    """wraps a `reduce=` and keeps the blocks it was given and the matrices it returned"""

    def __init__(self, inner):
        self.inner, self.blocks, self.U = inner, [], []

    def __call__(self, blocks, settings=None, device=0, matmul=None):
        out = self.inner(blocks, settings, device=device, matmul=matmul)
        self.blocks.extend(blocks)
        self.U.extend(out)
        return out


# ---- the lattices of the whole reductions -------------------------------------------------------------------------------------------------------------------
def _obj(rows):
    out = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, row in enumerate(rows):
        out[i] = [int(v) for v in row]
    return out


def identity(n):
    return _obj([[int(i == j) for j in range(n)] for i in range(n)])


def scrambled(seed, d, steps=None):
    """a small basis (the identity plus entries in [-2, 2] below the diagonal scaled rows) times a random unimodular matrix: elementary row operations
    with multipliers in [-3, 3]"""
    rng = np.random.default_rng(seed)
    A = [[int(v) for v in row] for row in (np.eye(d, dtype=np.int64) * rng.integers(1, 4, size=d) + np.tril(rng.integers(-2, 3, size=(d, d)), -1))]
    for _ in range(4 * d if steps is None else steps):
        i, j = (int(v) for v in rng.choice(d, size=2, replace=False)) if d > 1 else (0, 0)
        if i != j:
            m = int(rng.integers(-3, 4))
            A[i] = [a + m * b for a, b in zip(A[i], A[j])]
    return _obj(A)


def knapsack(seed=11, n=9, bits=40, weight=1 << 20):
    """[I_n | W a] with a planted relation x in {-1, 0, 1}^n, sum x_i a_i = 0; returns (lattice, x)"""
    rng = np.random.default_rng(seed)
    x = [1, -1, 0, 1, 1, -1, 0, -1, 1][:n]
    a = [(1 << (bits - 1)) + int.from_bytes(rng.bytes((bits + 6) // 8), "little") % (1 << (bits - 1)) for _ in range(n - 1)]
    last = -sum(xi * ai for xi, ai in zip(x, a)) * x[n - 1]
    a.append(last)
    assert sum(xi * ai for xi, ai in zip(x, a)) == 0
    return _obj([[int(i == j) for j in range(n)] + [weight * a[i]] for i in range(n)]), x


def ladder_input():
    """d = 16, a small basis times elementary operations with multipliers of 32 bits: entries of about 236 bits, far more than two words carry through the
    cancellation in r_kk"""
    rng = np.random.default_rng(7)
    A = [[int(v) for v in row] for row in scrambled(7, 16, steps=0)]
    for _ in range(48):
        i, j = (int(v) for v in rng.choice(16, size=2, replace=False))
        m = int.from_bytes(rng.bytes(4), "little") - (1 << 31)
        A[i] = [a + m * b for a, b in zip(A[i], A[j])]
    return _obj(A)


def whole_cases():
    """(name, lattice, cols_gram or None)"""
    rng = np.random.default_rng(5)
    wide = np.concatenate([_obj(rng.integers(-50, 51, size=(6, 8)).tolist()), identity(6)], axis=1)
    cases = [("d1", _obj([[7, -3, 2]]), None),
             ("big-quotient", _obj([[1, 0], [(1 << 100) + 3, 1]]), None),
             ("identity", identity(5), None),
             ("swaps-all-the-way-back", _obj([[int(i == j) << (6 - i) for j in range(6)] for i in range(6)]), None),
             ("knapsack", knapsack()[0], None),
             ("cols-gram", wide, 8)]
    cases += [(f"scrambled-{d}", scrambled(100 + d, d), None) for d in (3, 8, 17, 24)]
    return cases


def boundary_cases():
    """d = 4 at the lane and wave boundaries of the dot product: 63, 64, 65 and 255, 256 columns"""
    out = []
    for c in (63, 64, 65, 255, 256):
        rng = np.random.default_rng(c)
        A = rng.integers(-9, 10, size=(4, c)).astype(object)
        A[1] = A[1] + 5 * A[0]
        A[3] = A[3] - 7 * A[1] + 2 * A[2]
        out.append((f"cols-{c}", _obj(A.tolist()), None))
    return out


# ---- kernel blocks -----------------------------------------------------------------------------------------------------------------------------------------
HAND_MADE = {                        # (the blocks of tests/test_dixon_multi_cpu.py, copied)
    "fractions": (4, [[F(1, 2), F(1, 3), F(0), F(1)], [F(0), F(2, 5), F(1), F(-1, 7)]]),
    "zero rows": (5, [[F(0), F(3), F(0), F(1, 4), F(0)]]),
    "full": (2, [[F(1), F(1)], [F(1), F(-1)]]),
    "none": (3, []),
}
ECHELON_SIZES = ((8, 3), (12, 5), (16, 8), (24, 12))


def delsarte_kernels(branch="dual"):
    """the golden kernel of problems.delsarte_exact(8, 3, 1/2) (tests/golden/delsarte_exact_kernel.json): {block index: (N, vectors)}"""
    with open(os.path.join(_HERE, "golden", "delsarte_exact_kernel.json")) as fh:
        blocks = json.load(fh)[branch]
    return {i: (b["N"], [[F(n, d) for n, d in vec] for vec in b["vectors"]]) for i, b in enumerate(blocks)}


def echelon_kernels(seed, N, s, maxden=12):
    """s vectors of N entries in echelon form over the first s coordinates, the other entries random fractions with denominators <= maxden"""
    rng = np.random.default_rng(seed)
    return [[F(int(i == c)) for i in range(s)] + [F(int(rng.integers(-maxden, maxden + 1)), int(rng.integers(1, maxden + 1))) for _ in range(N - s)] for c in range(s)]


def echelon_block(seed, N, s):
    """(N, s, M, R) of echelon vectors [I_s ; W] without an inverse: the rows [-W^T row | e] cleared of denominators annihilate them"""
    vectors = echelon_kernels(seed, N, s)
    rows = [[-vectors[c][s + r] for c in range(s)] + [F(int(r == t)) for t in range(N - s)] for r in range(N - s)]
    M = rounding._rows_cleared_of_denominators(rows)
    return rounding._kernel_block(N, vectors, np.array([[F(0)] * N] * s + [[F(int(v)) for v in row] for row in M], dtype=object)), vectors


def kernel_sets():
    """(name, kernels) for basis_transformations"""
    sets = [("hand-made", HAND_MADE), ("delsarte-dual", delsarte_kernels("dual")), ("delsarte-primal", delsarte_kernels("primal"))]
    sets += [(f"echelon-{N}-{s}", {"e": (N, echelon_kernels(1000 + N, N, s))}) for N, s in ECHELON_SIZES]
    return sets

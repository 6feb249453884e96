"""Exact oracles for the basis change over a number field (clrs_modp_field_adjugate, rounding.inverse_field): Gauss-Jordan mod p on
numpy integers per (prime, root) pair after tests/pd_field_util.evaluate_mod -- the restatement of the device call and the host stand-in for
`rounding.field_adjugate_mod` --, a `Fraction` Gauss-Jordan and a greedy basis completion over QQ(g) on the arithmetic of tests/pd_field_util.py, host
stand-ins for `batch=` and `matmul=`, the golden kernels and the planted matrices.  The outputs of the device call are mathematically unique, so everything
is compared with `==`."""
import functools
import json
import os
from fractions import Fraction as F

import numpy as np

from clrs_amd import _lib, rounding
from tests import pd_field_util as fu

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(_HERE, "golden", "delsarte_field_kernel.json")
SENTINEL = fu.SENTINEL
_pi = fu._pi


# ---- mod p ------------------------------------------------------------------------------------------------------------------------------------------------------------
def adjugate_mod(A, p):
    """(adj, det, breakdown) of a square matrix of residues mod the prime p: Gauss-Jordan on [A | I] with the rows exchanged (the LAST candidate row is the
    pivot row, where the device takes the first: the outputs do not depend on it).  Singular: ([[-1] * n] * n, 0, c + 1), c the first column without a
    pivot.  int64 throughout: a product of residues is below 2^46."""
    a = np.array(A, dtype=np.int64) % p
    n = a.shape[0]
    a = np.concatenate([a, np.eye(n, dtype=np.int64)], axis=1)
    det = 1
    for c in range(n):
        cand = np.flatnonzero(a[c:, c]) + c
        if cand.size == 0:
            return np.full((n, n), -1, np.int64), 0, c + 1
        r = int(cand[-1])
        if r != c:
            a[[c, r]] = a[[r, c]]
            det = -det
        piv = int(a[c, c])
        det = det * piv % p
        a[c] = a[c] * pow(piv, -1, p) % p
        col = a[:, c].copy()
        col[c] = 0
        a = (a - col[:, None] * a[c][None, :]) % p
    det %= p
    return a[:, n:] * det % p, det, 0


def restate(mats, primes, roots):
    """per pair (adj, det, breakdown)"""
    return [[adjugate_mod(fu.evaluate_mod(mats, int(r), int(p)), int(p)) for r in rr] for p, rr in zip(primes, roots)]


def host_field_adjugate(coeff_matrices, primes, roots, device=0):
    """the stand-in for rounding.field_adjugate_mod: the same interface"""
    host_field_adjugate.calls.append(len(primes))
    got = restate(coeff_matrices, primes, roots)
    return (np.array([[g[0] for g in row] for row in got], np.int32), np.array([[g[1] for g in row] for row in got], np.int32),
            np.array([[g[2] for g in row] for row in got], np.int32))


host_field_adjugate.calls = []


def device_field_adjugate(mats, primes, roots, chunk_bytes=0, digits=None):
    """one raw call of clrs_modp_field_adjugate on sentinel-filled outputs: (code, adj, det, breakdown, info); `digits` (d, nd, n, n): the planes to pass"""
    L = _lib.load()
    if digits is None:
        a = np.array([[[int(v) for v in row] for row in np.asarray(M, dtype=object)] for M in mats], dtype=object)
        digits = np.ascontiguousarray(np.swapaxes(rounding.to_balanced_digits(a), 0, 1))
    digits = np.ascontiguousarray(digits, np.int32)
    d, nd, n = digits.shape[0], digits.shape[1], digits.shape[2]
    pr, rt = np.ascontiguousarray(primes, np.int32), np.ascontiguousarray(roots, np.int32)
    adj, det = np.full((pr.size, d, n, n), SENTINEL, np.int32), np.full((pr.size, d), SENTINEL, np.int32)
    brk, info = np.full((pr.size, d), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    assert L.clrs_config_set(b"modp_minors_chunk_bytes", int(chunk_bytes)) == 0
    try:
        code = L.clrs_modp_field_adjugate(0, n, d, nd, _pi(digits), pr.size, _pi(pr), _pi(rt), _pi(adj), _pi(det), _pi(brk), _pi(info))
    finally:
        assert L.clrs_config_set(b"modp_minors_chunk_bytes", 0) == 0
    return code, adj, det, brk, info


def points(seed, primes, d):
    """d distinct points in [0, p) per prime, 0 and p - 1 among them where they fit: the raw call takes any distinct points"""
    rng = np.random.default_rng(seed)
    out = []
    for p in primes:
        rr = {0, p - 1} if d >= 3 else {p - 1}
        while len(rr) < d:
            rr.add(int(rng.integers(0, p)))
        out.append(sorted(rr)[:d])
    return out


def lds_bytes(n):
    """what a workgroup of k_field_gj_adjugate takes: the padded matrix, the pivot row and the multiplier column, four masks, the permutation and its inverse"""
    npad = (n + 15) // 16 * 16
    return npad * (npad + 1 + 2) * 8 + 4 * 8 + 2 * npad * 4


def random_square_matrices(seed, d, n, bits):
    """d random square integer matrices, not symmetric, entries below 2^bits in size"""
    rng = np.random.default_rng(seed)
    return [[[int.from_bytes(rng.bytes((bits + 7) // 8), "little") % (1 << bits) * (1 if rng.integers(2) else -1) for _ in range(n)] for _ in range(n)]
            for _ in range(d)]


def host_rref(A, p, device=0):
    """the stand-in for rounding.rref_mod_p: (pivot columns, rank) by elimination on Python integers"""
    a = [[int(v) % p for v in row] for row in np.asarray(A, dtype=object)]
    pivots, r = [], 0
    for c in range(len(a[0]) if a else 0):
        piv = next((i for i in range(r, len(a)) if a[i][c]), None)
        if piv is None:
            continue
        a[r], a[piv] = a[piv], a[r]
        inv = pow(a[r][c], -1, p)
        a[r] = [v * inv % p for v in a[r]]
        for i in range(len(a)):
            if i != r and a[i][c]:
                f = a[i][c]
                a[i] = [(v - f * w) % p for v, w in zip(a[i], a[r])]
        pivots.append(c)
        r += 1
        if r == len(a):
            break
    return np.array(pivots, np.int32), r


def host_matmul(A, B, device=0):
    """the stand-in for rounding.zz_matmul: the product on Python integers"""
    host_matmul.calls += 1
    return np.asarray(A, dtype=object).dot(np.asarray(B, dtype=object))


host_matmul.calls = 0


# ---- over the field ---------------------------------------------------------------------------------------------------------------------------------------------------
def zero(f):
    return fu.el(f, 0)


def identity(f, n):
    return [[fu.el(f, int(i == j)) for j in range(n)] for i in range(n)]


def as_lists(M):
    """an object array (or nested lists) of coefficient tuples -> nested lists of tuples of Fractions"""
    return [[tuple(F(x) for x in e) for e in row] for row in M]


def matmul_exact(f, A, B):
    return [[functools.reduce(fu.add, (fu.mul(f, A[i][k], B[k][j]) for k in range(len(B))), zero(f)) for j in range(len(B[0]))] for i in range(len(A))]


def rref_exact(f, A):
    """(reduced rows, pivot columns) of a matrix of field elements by Gauss-Jordan on Fractions"""
    a = [list(row) for row in A]
    pivots, r = [], 0
    for c in range(len(a[0])):
        piv = next((i for i in range(r, len(a)) if any(a[i][c])), None)
        if piv is None:
            continue
        a[r], a[piv] = a[piv], a[r]
        inv = fu.inverse(f, a[r][c])
        a[r] = [fu.mul(f, v, inv) for v in a[r]]
        for i in range(len(a)):
            if i != r and any(a[i][c]):
                m = a[i][c]
                a[i] = [fu.sub(v, fu.mul(f, m, w)) for v, w in zip(a[i], a[r])]
        pivots.append(c)
        r += 1
        if r == len(a):
            break
    return a, pivots


def inverse_exact(f, B):
    """the inverse over the field, or None for a singular matrix"""
    n = len(B)
    a, pivots = rref_exact(f, [list(B[i]) + identity(f, n)[i] for i in range(n)])
    return [row[n:] for row in a] if pivots == list(range(n)) else None


def completion_exact(f, vectors, N):
    """the indices of the unit vectors the greedy completion takes: the pivot columns behind the first s of [V | I] over the field"""
    s = len(vectors)
    rows = [[vectors[c][i] for c in range(s)] + identity(f, N)[i] for i in range(N)]
    pivots = rref_exact(f, rows)[1]
    assert pivots[:s] == list(range(s)) and len(pivots) == N
    return [c - s for c in pivots[s:]]


def determinant_exact(f, B):
    """the determinant by elimination over the field"""
    a, n, det = [list(row) for row in B], len(B), fu.el(f, 1)
    for c in range(n):
        piv = next((i for i in range(c, n) if any(a[i][c])), None)
        if piv is None:
            return zero(f)
        if piv != c:
            a[c], a[piv] = a[piv], a[c]
            det = fu.sub(zero(f), det)
        det = fu.mul(f, det, a[c][c])
        inv = fu.inverse(f, a[c][c])
        for i in range(c + 1, n):
            if any(a[i][c]):
                m = fu.mul(f, a[i][c], inv)
                a[i] = [fu.sub(v, fu.mul(f, m, w)) for v, w in zip(a[i], a[c])]
    return det


def to_g(lc, e):
    """sum_j y_j h^j for h = lc g, as coefficients in g"""
    return tuple(F(y) * lc ** j for j, y in enumerate(e))


# ---- the golden kernels and the planted matrices ---------------------------------------------------------------------------------------------------------------------
GOLDEN_BLOCKS = (("600-cell", "19"), ("600-cell", "20"), ("icosahedron", "7"))
GOLDEN_COMPLETIONS = {("600-cell", "19"): [0, 1], ("600-cell", "20"): [0, 1, 2], ("icosahedron", "7"): [0]}
GOLDEN_PRIMES = {("600-cell", "19"): 2, ("600-cell", "20"): 3, ("icosahedron", "7"): 1}


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def golden_kernels(case):
    """{key: (N, vectors)} with the vectors as lists of coefficient tuples of Fractions, as rounding.vectors_to_field gives them"""
    data = golden()[case]
    assert data["field"] == [-5, 0, 1]
    return {key: (len(vecs[0]), [[tuple(F(x) for x in e) for e in v] for v in vecs]) for key, vecs in data["blocks"].items()}


@functools.lru_cache(maxsize=None)
def golden_basis(case, key):
    """(N, s, vectors, B = [V | E] with the exact greedy completion, its exact inverse)"""
    f = [-5, 0, 1]
    N, vectors = golden_kernels(case)[key]
    s = len(vectors)
    extra = completion_exact(f, vectors, N)
    B = [[vectors[c][i] for c in range(s)] + [fu.el(f, int(i == j)) for j in extra] for i in range(N)]
    return N, s, vectors, extra, B, inverse_exact(f, B)


@functools.lru_cache(maxsize=None)
def planted(name, n=6):
    """a random matrix over the field `name` of tests/pd_field_util.FIELDS (halves for the non-monic field: denominators to clear) and its exact inverse"""
    fld = fu.field(name)
    f = fld.minpoly
    B = fu.random_elements(41 + n, f, n, n)
    if name == "2x2-5":
        B = [[tuple(x / 2 for x in e) for e in row] for row in B]
    inv = inverse_exact(f, B)
    assert inv is not None
    return fld, B, inv


def first_primes_needed(fld, bound):
    """the least number of split primes, from 2^23 downwards, whose product exceeds twice the bound"""
    count = 1
    while True:
        primes, _ = rounding.split_primes(fld, count)
        if np.prod([int(p) for p in primes], dtype=object) > 2 * bound:
            return count
        count += 1


def integer_form(fld, B):
    """(scale, lc, the d integer coefficient matrices in h) as rounding.inverse_field is documented to form them, by tests/pd_field_util.normal_form"""
    scale, lc, M = fu.normal_form(fld, B)
    d = len(fld.minpoly) - 1
    return scale, lc, [[[fu.to_h_coordinates(lc, e)[c] for e in row] for row in M] for c in range(d)]


@functools.lru_cache(maxsize=None)
def host_hooks():
    return dict(adjugate=host_field_adjugate, batch=host_rref, matmul=host_matmul)

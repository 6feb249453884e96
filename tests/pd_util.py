"""Exact oracles for the positive-definiteness check (clrs_modp_minors, rounding.checkpd): the leading principal minors of an integer
matrix by Bareiss' fraction-free elimination on Python integers, a Python restatement of what the device does per prime (the elimination L D L^T mod p
without exchanges, the minors as running products of the pivots), the host stand-in for `rounding.leading_minors_mod` built on it, and the matrices of the
tests.  Everything is compared with `==`."""
from fractions import Fraction as F

import numpy as np

from clrs_amd import _lib, rounding

PMAX = 8388593
SENTINEL = -77


def _pi(a):
    return None if a is None else a.ctypes.data_as(_lib.p_i32)


def bareiss_minors(M):
    """the n leading principal minors of a square matrix of Python integers, exactly: Bareiss' elimination with a row exchange where a pivot is zero (the
    leading minor of that order and every later one through that pivot position are then taken from the definition instead)"""
    n = len(M)
    a = [[int(v) for v in row] for row in M]
    out, prev = [], 1
    for k in range(n):
        out.append(a[k][k])
        if a[k][k] == 0:                                             # a zero leading minor: the rest by the definition on fresh copies
            for m in range(k + 2, n + 1):
                out.append(det([[int(v) for v in row[:m]] for row in M[:m]]))
            return out
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                a[i][j] = (a[i][j] * a[k][k] - a[i][k] * a[k][j]) // prev
        prev = a[k][k]
    return out


def det(M):
    """the determinant of a square matrix of Python integers by Bareiss' elimination with row exchanges"""
    n = len(M)
    a = [list(row) for row in M]
    sign, prev = 1, 1
    for k in range(n):
        piv = next((i for i in range(k, n) if a[i][k] != 0), None)
        if piv is None:
            return 0
        if piv != k:
            a[k], a[piv] = a[piv], a[k]
            sign = -sign
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                a[i][j] = (a[i][j] * a[k][k] - a[i][k] * a[k][j]) // prev
        prev = a[k][k]
    return sign * a[n - 1][n - 1] if n else 1


def minors_mod(M, p):
    """what one workgroup of k_minors_ldl computes: (row, breakdown) for the prime p -- the elimination without exchanges on the residues, the minors as
    running products of the pivots, 0 at the first zero pivot and -1 behind it"""
    n = len(M)
    a = [[int(v) % p for v in row] for row in M]
    row, prod = [], 1
    for j in range(n):
        d = a[j][j]
        prod = prod * d % p
        row.append(prod)
        if d == 0:
            return row + [-1] * (n - j - 1), j + 1
        inv = pow(d, -1, p)
        for i in range(j + 1, n):
            f = a[i][j] * inv % p
            if f:
                for c in range(j + 1, n):
                    a[i][c] = (a[i][c] - f * a[j][c]) % p
    return row, 0


def minors_mod_np(M, p):
    """minors_mod with the rows of a step taken together in int64 (a residue times a residue is below 2^46): the same answer, fast enough for hundreds of
    primes"""
    n = len(M)
    a = np.array([[int(v) % p for v in row] for row in M], dtype=np.int64).reshape(n, n)
    row, prod = [], 1
    for j in range(n):
        d = int(a[j, j])
        prod = prod * d % p
        row.append(prod)
        if d == 0:
            return row + [-1] * (n - j - 1), j + 1
        f = a[j + 1:, j] * pow(d, -1, p) % p
        a[j + 1:, j + 1:] = (a[j + 1:, j + 1:] - f[:, None] * a[j, j + 1:][None, :]) % p
    return row, 0


def host_minors(M, primes, device=0):
    """the stand-in for rounding.leading_minors_mod: the same interface, Python integers"""
    host_minors.calls.append(len(primes))
    M = [[int(v) for v in row] for row in np.asarray(M, dtype=object)]
    rows, brk = zip(*(minors_mod(M, int(p)) for p in primes))
    return np.array(rows, np.int32), np.array(brk, np.int32)


host_minors.calls = []


def minors_from_exact(exact, p):
    """(row, breakdown) for the prime p from the exact minors: the same answer as minors_mod as long as no minor before the breakdown is 0 mod p"""
    row, n = [], len(exact)
    for k, v in enumerate(exact):
        row.append(v % p)
        if v % p == 0:
            return row + [-1] * (n - k - 1), k + 1
    return row, 0


def device_minors(M, primes, chunk_bytes=0, digits=None):
    """one raw call of clrs_modp_minors on sentinel-filled outputs: (code, minors, breakdown, info); `digits`: the planes to pass instead of those of M"""
    L = _lib.load()
    digits = rounding.to_balanced_digits(np.asarray(M, dtype=object)) if digits is None else np.ascontiguousarray(digits, np.int32)
    n = digits.shape[1]
    pr = np.ascontiguousarray(primes, np.int32)
    minors, brk, info = np.full((pr.size, n), SENTINEL, np.int32), np.full(pr.size, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    assert L.clrs_config_set(b"modp_minors_chunk_bytes", int(chunk_bytes)) == 0
    try:
        code = L.clrs_modp_minors(0, n, digits.shape[0], _pi(digits), pr.size, _pi(pr), _pi(minors), _pi(brk), _pi(info))
    finally:
        assert L.clrs_config_set(b"modp_minors_chunk_bytes", 0) == 0
    return code, minors, brk, info


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------------------------------
def random_spd(seed, n, bits):
    """B^T B + I for a random integer B with entries of about `bits` / 2 bits: positive definite, entries of about `bits` bits"""
    rng = np.random.default_rng(seed)
    half = max(bits // 2, 1)
    B = [[int.from_bytes(rng.bytes((half + 7) // 8), "little") % (1 << half) - (1 << (half - 1)) for _ in range(n)] for _ in range(n)]
    return [[sum(B[k][i] * B[k][j] for k in range(n)) + (1 if i == j else 0) for j in range(n)] for i in range(n)]


def random_symmetric(seed, n, bits):
    """a random symmetric integer matrix (indefinite in general) with entries below 2^bits in size"""
    rng = np.random.default_rng(seed)
    M = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            v = int.from_bytes(rng.bytes((bits + 7) // 8), "little") % (1 << (bits + 1)) - (1 << bits)
            M[i][j] = M[j][i] = v
    return M


def unit_lower(seed, n, size=3):
    rng = np.random.default_rng(seed)
    return [[1 if i == j else (int(rng.integers(-size, size + 1)) if j < i else 0) for j in range(n)] for i in range(n)]


def ldlt(L, d):
    """L diag(d) L^T for a unit lower triangular L: the leading minors are the running products of d"""
    n = len(L)
    return [[sum(L[i][k] * d[k] * L[j][k] for k in range(min(i, j) + 1)) for j in range(n)] for i in range(n)]


def hilbert(n):
    return [[F(1, i + j + 1) for j in range(n)] for i in range(n)]


def planted(name):
    """the planted matrices of the tests: name -> (matrix, pd, failed_order)"""
    if name == "hilbert20":
        return hilbert(20), True, None
    if name in ("hilbert20 minus 1e-40", "hilbert20 minus 1e-28"):   # the smallest eigenvalue of the Hilbert matrix of order 20 is about 7.8e-29: between the two shifts
        H = hilbert(20)
        for i in range(20):
            H[i][i] -= F(1, 10 ** (40 if name.endswith("40") else 28))
        return H, name.endswith("40"), None                         # (the order comes from the exact minors)
    if name == "singular psd":                                      # rank n - 1: B^T B with B (n - 1) x n; every minor below the last is positive
        n = 12
        B = np.random.default_rng(3).integers(-5, 6, size=(n - 1, n)).astype(object)
        return [[int(v) for v in row] for row in B.T.dot(B)], False, n
    if name == "zero minor 17 of 33":
        d = [1 + (k % 3) for k in range(33)]
        d[16] = 0
        return ldlt(unit_lower(4, 33), d), False, 17
    if name == "negative minor 9 of 20":
        d = [2] * 20
        d[8] = -3
        return ldlt(unit_lower(5, 20), d), False, 9
    if name == "first prime planted at 5 of 12":
        d = [1] * 12
        d[4] = PMAX
        return ldlt(unit_lower(6, 12, size=2), d), True, None
    raise KeyError(name)


PLANTED = ("hilbert20", "hilbert20 minus 1e-40", "hilbert20 minus 1e-28", "singular psd", "zero minor 17 of 33", "negative minor 9 of 20", "first prime planted at 5 of 12")

"""Shared by tests/test_kernel_vectors_cpu.py and tests/test_kernel_vectors_gpu.py: the five problems with the ranks of their solution blocks, the Python
restatement of the scatter's index map, an mpmath stand-in for the device call of clrs_amd.rounding (the elimination of tests/preprocess_host.py plus a
plain product), the index map compiled for the host (tests/mw_host/mw_kv_host.cpp) and the planted blocks of the device tests."""
import ctypes as C
import functools
import os
import subprocess

import mpmath as mp
import numpy as np

from clrs_amd import _lib
from clrs_amd.mw import to_limbs
from clrs_amd.rounding import BlockKernel
from tests.preprocess_host import limbs_to_mp, pivoted_cholesky

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_kv_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_kv_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
LIMBS = (4, 5, 6, 8, 10)

# ranks of the X blocks of the solutions at gap 1e-30, in block order (eigenvalues of X above 1e-10 = eigenvalues of Y below 1e-10)
RANKS = {
    "theta_c5": [2],
    "povm_2x2": [2, 2],
    "min_f_2": [1, 1],
    "cohnelkies_8_3": [1, 1, 1, 2],
    "delsarte_3_6": [0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 5, 3, 1],
}


@functools.lru_cache(maxsize=None)
def problem(name):
    import clrs_amd
    from clrs_amd import problems as P
    sdp = {"theta_c5": P.theta_c5, "povm_2x2": P.povm_2x2, "min_f_2": lambda: P.min_f(2), "cohnelkies_8_3": lambda: P.cohnelkies(8, 3),
           "delsarte_3_6": lambda: P.delsarte(3, 6, 0.5)}[name]()
    return clrs_amd.flatten(sdp)


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_mw_kernel_vectors.hip.h", "clrs_mw_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mw_kv_entry.argtypes = [C.c_int, _lib.p_i32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    L.mw_kv_max.argtypes, L.mw_kv_max.restype = [C.c_double, C.c_double], C.c_double
    L.mw_kv_scatter_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _lib.p_i32, _lib.p_d, C.c_long, _lib.p_d]
    L.mw_kv_scatter_host.restype = C.c_long
    return L


def restate_vectors(branch, perm, r, W):
    """The vectors from (perm, r, W), W of shape (planes, r, n - r) (or (r, n - r) of any dtype): shape (planes, n, count), in the words of the issue --
    dual: vector c has v[perm[c]] = 1, v[perm[r + a]] = W[c, a], 0 at the other pivots; primal: vector a has v[perm[r + a]] = 1, v[perm[c]] = -W[c, a],
    0 at the other non-pivots."""
    W = np.asarray(W)
    flat2 = W.ndim == 2
    W = W[None] if flat2 else W
    n = len(perm)
    V = np.zeros((W.shape[0], n, r if branch == "dual" else n - r), dtype=W.dtype)
    if branch == "dual":
        for c in range(r):
            V[0, perm[c], c] = 1
            for a in range(n - r):
                V[:, perm[r + a], c] = W[:, c, a]
    else:
        for a in range(n - r):
            V[0, perm[r + a], a] = 1
            for c in range(r):
                V[:, perm[c], a] = -W[:, c, a]
    return V[0] if flat2 else V


def w_of_vectors(branch, perm, r, V):
    """the relations W (planes, r, n - r) read back out of the vectors (planes, n, count)"""
    n = len(perm)
    piv, rest = list(perm[:r]), list(perm[r:])
    if r == 0 or r == n:
        return np.zeros((V.shape[0], r, n - r))
    return V[:, rest, :].transpose(0, 2, 1) if branch == "dual" else -V[:, piv, :]


def block_mp(planes, n):
    """planar (K, n * n) column-major -> n x n list of lists of mpmath numbers (call under the working precision wanted)"""
    g = limbs_to_mp(planes)
    return [[g[i + j * n] for j in range(n)] for i in range(n)]


def host_batch(block_n, X, Y, limbs, tau, use_dual, dual_max, device=0):
    """clrs_amd.rounding.kernel_vectors_batch in mpmath at 52 * limbs bits: the branch from limb plane 0, the elimination of tests/preprocess_host.py, the
    vectors by `restate_vectors`, the residual by a plain product."""
    out, off = [], 0
    bits = 52 * int(limbs)
    for n in (int(v) for v in block_n):
        Xb, Yb = X[:, off:off + n * n], Y[:, off:off + n * n]
        off += n * n
        branch = "dual" if use_dual and (n == 0 or float(np.max(np.abs(Xb[0]))) <= dual_max) else "primal"
        with mp.workprec(bits + 64):
            G, Ym = block_mp(Xb if branch == "dual" else Yb, n), block_mp(Yb, n)
        perm, r, W, resid, _ = pivoted_cholesky(G, None, tau, bits)
        with mp.workprec(bits):
            Wm = np.array(W, dtype=object).reshape(r, n - r)
            Vm = restate_vectors(branch, perm, r, Wm + mp.mpf(0))
            count = Vm.shape[1]
            R = [[mp.fsum(Ym[i][k] * Vm[k, v] for k in range(n)) for v in range(count)] for i in range(n)]
            rmax = np.array([max(abs(float(R[i][v])) for i in range(n)) for v in range(count)], dtype=np.float64)
            vmax = np.array([max(abs(float(Vm[i, v])) for i in range(n)) for v in range(count)], dtype=np.float64)
            vec = to_limbs([Vm[i, v] for i in range(n) for v in range(count)], limbs).reshape(limbs, n, count) if n * count else np.zeros((limbs, n, count))
            piv = to_limbs(resid, limbs) if n - r else np.zeros((limbs, 0))
        out.append(BlockKernel(branch, r, count, np.array(perm, dtype=np.int32), vec, rmax, vmax, piv))
    return out


# ---- planted blocks of the device tests ------------------------------------------------------------------------------------------------------

def _unit_triangular(rng, n, dense=0):
    """unit lower triangular of small integers: two entries +-1 per row left of the diagonal, and the first `dense` columns filled with -5 .. 5 without 0 (the
    rows of M[:, :r] then differ and the pivots of X rarely tie; the inverse is an integer matrix whatever the entries)"""
    L = [[int(i == j) for j in range(n)] for i in range(n)]
    for i in range(1, n):
        for j in rng.choice(i, size=min(2, i), replace=False):
            L[i][int(j)] = int(rng.choice([-1, 1]))
        for j in range(min(dense, i)):
            L[i][j] = int(rng.choice([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5]))
    return L


def _int_inverse_unit_lower(L):
    n = len(L)
    inv = [[int(i == j) for j in range(n)] for i in range(n)]
    for i in range(n):
        for k in range(i):
            if L[i][k]:
                for j in range(n):
                    inv[i][j] -= L[i][k] * inv[k][j]
    return inv


def planted_pair(n, r, K, seed):
    """(X, Y) planar (K, n * n): X = M[:, :r] D M[:, :r]^T, Y = M^-T[:, r:] E M^-T[:, r:]^T with M = L U (unit triangular, small integers: M^-1 is an
    integer matrix) and positive rational diagonals D, E (sixteenths), so X Y = 0 exactly, rank X = r, rank Y = n - r; plus 2^-100 times a random PSD
    matrix each, rounded to K limbs."""
    rng = np.random.default_rng(seed)
    L, Ut = _unit_triangular(rng, n, dense=min(r, 6) if r < n else 0), _unit_triangular(rng, n)      # (dense: no zero rows in M[:, :r]; full rank: M stays well conditioned)
    U = [[Ut[j][i] for j in range(n)] for i in range(n)]
    M = [[sum(L[i][k] * U[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    Li, Uti = _int_inverse_unit_lower(L), _int_inverse_unit_lower(Ut)          # M^-T = L^-T U^-T = Li^T Uti
    Mit = [[sum(Li[k][i] * Uti[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    d = [int(v) for v in rng.integers(8, 129, n)]                              # sixteenths: 1/2 .. 8
    X0 = [[sum(M[i][k] * d[k] * M[j][k] for k in range(r)) for j in range(n)] for i in range(n)]
    Y0 = [[sum(Mit[i][k] * d[k] * Mit[j][k] for k in range(r, n)) for j in range(n)] for i in range(n)]
    assert all(sum(X0[i][k] * Y0[k][j] for k in range(n)) == 0 for i in range(n) for j in range(n))
    out = []
    with mp.workprec(64 * K + 128):
        for A0 in (X0, Y0):
            G = rng.standard_normal((n, n))
            P = G @ G.T / n
            P = (P + P.T) / 2
            out.append(to_limbs([mp.mpf(A0[i][j]) / 16 + mp.ldexp(mp.mpf(float(P[i, j])), -100) for j in range(n) for i in range(n)], K))
    return out[0], out[1]

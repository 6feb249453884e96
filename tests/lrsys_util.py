"""Shared by tests/test_linear_system_cpu.py and tests/test_linear_system_gpu.py: the index arithmetic of csrc/clrs_modp_lrsys_arith.h compiled for the host
(tests/mw_host/lrsys_host.cpp), the oracle of clrs_zz_lowrank_system in Python integers, the raw device call, the operands of the tests, a hand-made
`ExactProblem` with its dense restatement, the host stand-ins of every hook of `rounding.exact_solution`, and the assertions on the exact solution of
delsarte_exact(8, 3, 1/2)."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction as F

import numpy as np

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import modp_util as mu
from tests import pd_util
from tests import rationalize_util as ru
from tests import zz_util as zu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "lrsys_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "liblrsys_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
_DEPS = [_SRC, os.path.join(_CSRC, "clrs_modp_lrsys_arith.h"), os.path.join(_CSRC, "clrs_modp_zz_arith.h")]
HALF, SENTINEL, INVALID = 1 << 23, -7, -1
_pi = lambda a: a.ctypes.data_as(_lib.p_i32) if a is not None else _lib.p_i32()
_pd = lambda a: a.ctypes.data_as(_lib.p_d)


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in _DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.lrsys_constants_host.argtypes = [_lib.p_i32]
    L.lrsys_panels_host.argtypes = [C.c_int] * 3 + [_lib.p_i32]
    L.lrsys_stride_host.argtypes = [C.c_int]
    L.lrsys_p_range_host.argtypes = [C.c_int] * 5 + [_lib.p_i32]
    L.lrsys_slots_host.argtypes = [C.c_int] * 3 + [_lib.p_i32]
    L.lrsys_host.argtypes = [C.c_int] * 3 + [_lib.p_i32, C.c_int, _lib.p_i32, C.c_int, _lib.p_i32, C.c_int, _lib.p_i32, _lib.p_i32, C.c_int, _lib.p_i32] + [C.c_int] * 3 + [_lib.p_i32]
    for f in (L.lrsys_constants_host, L.lrsys_panels_host, L.lrsys_stride_host, L.lrsys_p_range_host, L.lrsys_slots_host, L.lrsys_host):
        f.restype = C.c_int
    return L


def host_constants():
    out = np.zeros(5, np.int32)
    host_lib().lrsys_constants_host(_pi(out))
    return [int(v) for v in out]                    # [tile, row capacity, MFMAs between flushes, the most allowed, the bound on K]


def host_panels(rmax, ndu, ndw):
    out = np.zeros(5, np.int32)
    host_lib().lrsys_panels_host(rmax, ndu, ndw, _pi(out))
    return [int(v) for v in out]                    # [tp, dp, dq, stride of U, stride of W]


def host_p_range(s, p0, dp, q0, dq):
    out = np.zeros(3, np.int32)
    host_lib().lrsys_p_range_host(s, p0, dp, q0, dq, _pi(out))
    return [int(v) for v in out]                    # [np, plo, phi]


def host_slots(lane4, np_, count):
    out = np.zeros((count, 2), np.int32)
    host_lib().lrsys_slots_host(lane4, np_, count, _pi(out))
    return [tuple(int(v) for v in row) for row in out]


def _args(Ud, Wd, rowptr, pairs):
    Ud, Wd = np.ascontiguousarray(Ud, dtype=np.int32), np.ascontiguousarray(Wd, dtype=np.int32)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    pairs = np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2)
    return Ud, Wd, rowptr, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def host_system(Ud, Wd, rowptr, pairs, ndc, panels=(0, 0, 0)):
    """(code, C, info): the whole call by the host build of the kernel's pieces; `panels` = (tp, dp, dq) forces the panels (default: lrsys_panels)"""
    Ud, Wd, rowptr, ca, cb = _args(Ud, Wd, rowptr, pairs)
    (ndu, n, T), ndw, R, nc = Ud.shape, Wd.shape[0], rowptr.size - 1, ca.size
    Cd, info = np.full((ndc, R, nc), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    code = host_lib().lrsys_host(n, T, R, _pi(rowptr), ndu, _pi(Ud), ndw, _pi(Wd), nc, _pi(ca), _pi(cb), ndc, _pi(Cd), *[int(v) for v in panels], _pi(info))
    return code, Cd, info


# ---- the device call -----------------------------------------------------------------------------------------------------------------------------------------
def device_system(Ud, Wd, rowptr, pairs, ndc, device=0):
    """(code, C, info): clrs_zz_lowrank_system on digit planes, C and info filled with sentinels before the call"""
    Ud, Wd, rowptr, ca, cb = _args(Ud, Wd, rowptr, pairs)
    (ndu, n, T), ndw, R, nc = Ud.shape, Wd.shape[0], rowptr.size - 1, ca.size
    Cd, info = np.full((ndc, R, nc), SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    code = _lib.load().clrs_zz_lowrank_system(device, n, T, R, _pi(rowptr), ndu, _pi(Ud), ndw, _pi(Wd), nc, _pi(ca), _pi(cb), ndc, _pi(Cd), _pi(info))
    return code, Cd, info


def device_times():
    t = np.zeros(3)
    assert _lib.load().clrs_zz_lowrank_system_times(_pd(t[0:]), _pd(t[1:]), _pd(t[2:])) == 0
    return [float(v) for v in t]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------------------------
def exact_system(Ud, Wd, rowptr, pairs):
    """C[i, c] = 2^(a != b) sum_{t in row i} U[a, t] W[b, t] in Python integers, from the digit planes"""
    U, W = zu.values_of(Ud), zu.values_of(Wd)
    out = np.zeros((len(rowptr) - 1, len(pairs)), dtype=object)
    for i in range(len(rowptr) - 1):
        for c, (a, b) in enumerate(pairs):
            out[i, c] = (1 if a == b else 2) * sum(int(U[a, t]) * int(W[b, t]) for t in range(rowptr[i], rowptr[i + 1]))
    return out


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a, n)]


def sparse_pairs(n):
    """a selection that leaves whole tiles of 16 x 16 empty: the first and the last row of the triangle, a few diagonal entries, one pair twice"""
    picks = [(0, b) for b in range(0, n, 3)] + [(a, n - 1) for a in range(0, n, 5)] + [(a, a) for a in range(1, n, 7)]
    return picks + picks[:1]


def row_pointer(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def extreme_digits(seed, nd, n, T):
    """every digit +-2^23"""
    rng = np.random.default_rng(seed)
    return (rng.choice(np.array([-HALF, HALF]), size=(nd, n, T))).astype(np.int32)


def mixed_case(seed, n, ndu, ndw, counts=(0, 1, 2, 5, 0, 2)):
    """(Ud, Wd, rowptr): rows of 0, 1, 2 and 5 terms in one call"""
    rowptr = row_pointer(counts)
    T = int(rowptr[-1])
    return zu.random_digits(seed, ndu, n, T), zu.random_digits(seed + 1000, ndw, n, T), rowptr


# ---- the hooks of rounding.exact_solution on the host -----------------------------------------------------------------------------------------------------------
def host_assemble(U, W, rowptr, pairs, device=0):
    """the `assemble` stand-in of rounding.linear_system: Python integers"""
    U, W = du.objects(np.asarray(U, dtype=object)), du.objects(np.asarray(W, dtype=object))
    out = np.zeros((len(rowptr) - 1, len(pairs)), dtype=object)
    for i in range(len(rowptr) - 1):
        for c, (a, b) in enumerate(pairs):
            out[i, c] = (1 if a == b else 2) * sum(int(U[a, t]) * int(W[b, t]) for t in range(rowptr[i], rowptr[i + 1]))
    return out


class Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *args, **kw):
        self.calls.append(tuple(np.asarray(a, dtype=object).shape for a in args[:2]))
        return self.fn(*args, **kw)


def host_hooks():
    from tests import dixon_multi_util as dm
    return dict(batch=mu.host_batch, lift=du.lift, reconstruct=dm.host_reconstruct, matmul=dm.host_matmul, minors=pd_util.host_minors,
                round_batch=ru.host_round_batch, assemble=host_assemble)


# ---- a hand-made problem: two clusters, a low-rank block of 2 x 2 sub-blocks with rank-2 terms, a dense block, free variables ---------------------------------------
def handmade_problem():
    rng = np.random.default_rng(2024)
    fr = lambda shape: np.array([F(int(a), int(b)) for a, b in zip(rng.integers(-9, 10, size=int(np.prod(shape))), rng.integers(1, 7, size=int(np.prod(shape))))],
                                dtype=object).reshape(shape)
    delta, P0, P1, N = 2, 3, 2, 2

    def sym_rank2():                                   # lam (v w^T + w v^T): vs != ws, symmetric
        lam, v, w = fr((1,))[0], fr((delta,)), fr((delta,))
        return rounding.ExactLowRank([lam, lam], [v, w], [w, v])

    def lowrank_entries(P):
        ent = {(0, 0): {}, (0, 1): {}, (1, 0): {}, (1, 1): {}}
        for p in range(P):
            ent[(0, 0)][p], ent[(1, 1)][p] = sym_rank2(), sym_rank2()
            off = rounding.ExactLowRank(fr((2,)), fr((2, delta)), fr((2, delta)))
            ent[(0, 1)][p] = off
            ent[(1, 0)][p] = rounding.ExactLowRank(off.lam, off.ws, off.vs)          # the transposed partner
        return ent

    def dense_entries(P, n):
        out = {}
        for p in range(P):
            M = fr((n, n))
            out[p] = M + M.T
        return {(0, 0): out}
    lr0, dn0 = rounding.ExactBlock(2, delta, lowrank_entries(P0), "L0"), rounding.ExactBlock(1, 3, dense_entries(P0, 3), "D0")
    lr1 = rounding.ExactBlock(2, delta, lowrank_entries(P1), "L1")
    symm = lambda n: (lambda M: M + M.T)(fr((n, n)))
    return rounding.ExactProblem(True, F(1, 3), [[lr0, dn0], [lr1]], [fr((P0, N)), fr((P1, N))], [fr((P0,)), fr((P1,))], [[symm(4), symm(3)], [symm(4)]], fr((N,)))


def handmade_Bs(problem):
    """hand-made transformations (B^T, Binv, s): block 0 loses one dimension, block 1 keeps all under a rational change of basis, block 2 has none"""
    B0 = np.array([[1, 0, 0, 0], [F(1, 2), 1, 0, 0], [-1, F(2, 3), 1, 0], [2, 0, F(1, 5), 1]], dtype=object)
    B1 = np.array([[2, 1, 0], [0, 1, F(1, 3)], [0, 0, 1]], dtype=object)
    out = {}
    for key, (B, s) in {0: (B0, 1), 1: (B1, 0)}.items():
        Bf = rounding._object_matrix(B, "test", F)
        out[key] = (Bf.T.copy(), _inverse(Bf), s)
    return out


def _inverse(B):
    """the inverse of a small matrix of Fractions by Gauss-Jordan"""
    n = B.shape[0]
    M = [[F(v) for v in B[i]] + [F(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    out = np.empty((n, n), dtype=object)
    for i in range(n):
        out[i] = M[i][n:]
    return out


def dense_constraint(bl, p):
    """the constraint matrix of constraint p in block `bl` as a dense (n, n) matrix of Fractions, entry by entry"""
    n, d = bl.n, bl.delta
    M = np.empty((n, n), dtype=object)
    M.fill(F(0))
    for (r, s), ent in bl.entries.items():
        e = ent.get(p)
        if e is None:
            continue
        if isinstance(e, rounding.ExactLowRank):
            for k in range(e.rank):
                for i in range(d):
                    for j in range(d):
                        M[r * d + i, s * d + j] += e.lam[k] * e.vs[k][i] * e.ws[k][j]
        else:
            for i in range(n):
                for j in range(n):
                    M[i, j] += e[i][j]
    return M


def restated_system(problem, Bs=None):
    """(A, b, index) by triple loops on dense constraint matrices: P M P^T entry by entry, the factor 2 off the diagonal"""
    rows, index = [], []
    kept = []
    for bi, (j, bl) in enumerate(problem.flat_blocks()):
        if Bs is not None and bi in Bs:
            Binv, s = Bs[bi][1], Bs[bi][2]
            kept.append([[F(v) for v in Binv[r]] for r in range(s, bl.n)])
        else:
            kept.append([[F(int(r == c)) for c in range(bl.n)] for r in range(bl.n)])
        index += [(bi, a, b) for a in range(len(kept[-1])) for b in range(a, len(kept[-1]))]
    index += [("free", k) for k in range(problem.b.size)]
    for j, cl in enumerate(problem.blocks):
        for p in range(len(problem.c[j])):
            row = []
            for bi, (jj, bl) in enumerate(problem.flat_blocks()):
                P, n = kept[bi], bl.n
                M = dense_constraint(bl, p) if jj == j else None
                for a in range(len(P)):
                    for b in range(a, len(P)):
                        v = F(0)
                        if M is not None:
                            for x in range(n):
                                for y in range(n):
                                    v += P[a][x] * M[x, y] * P[b][y]
                        row.append(v if a == b else 2 * v)
            row += [problem.B[j][p, k] for k in range(problem.b.size)]
            rows.append(row)
    return rows, [F(v) for cj in problem.c for v in cj], index


# ---- delsarte_exact(8, 3, 1/2) -----------------------------------------------------------------------------------------------------------------------------------
EXPECTED_A = (F(0), F(8), F(25), F(52), F(133, 2), F(60), F(55, 2))


def check_delsarte_exact_solution(problem, sol):
    """what the exact solution of delsarte_exact(8, 3, 1/2) must be: the bound 240 with a = (0, 8, 25, 52, 133/2, 60, 55/2), A = 0, every constraint exact
    at every sample for the untransformed blocks, every certificate positive"""
    assert sol.success and sol.correct_slacks
    assert sol.objective == 240 and type(sol.objective) is F
    assert tuple(sol.Y[k][0, 0] for k in range(7)) == EXPECTED_A
    assert sol.Y[7].shape == (4, 4) and all(v == 0 for v in sol.Y[7].flat)
    assert sol.Y[8].shape == (3, 3) and any(v != 0 for v in sol.Y[8].flat)
    assert sol.certificates and all(cert.pd for cert in sol.certificates)
    blocks = [bl for _, bl in problem.flat_blocks()]
    for p in range(len(problem.c[0])):
        total = F(0)
        for bl, Y in zip(blocks, sol.Y):
            M = dense_constraint(bl, p)
            total += sum((M[i, j] * Y[i, j] for i in range(bl.n) for j in range(bl.n)), F(0))
        assert total == problem.c[0][p], p

"""Shared by tests/test_mw_gemm_cpu.py and tests/test_mw_gemm_gpu.py: the host restatement of the batched multi-word product
(tests/mw_host/mw_gemm_host.cpp, the kernel's own entry functions compiled with g++), the job list of the issue, its mpmath reference
and the bound

    |C_ij - exact| <= (k + 2) 2^-(52 K - 2) (sum_r |a_ir b_rj| + |c_ij|)

(the accumulator bound of tests/test_mw_arith_cpu.py::test_mw_dot_accumulator plus the one add of beta C); `exact` in mpmath at 53 K + 200 bits
from the limb sums of the inputs."""
import ctypes as C
import functools
import os
import subprocess

import mpmath as mp
import numpy as np

from clrs_amd import _lib
from tests.test_mw_arith_cpu import rand_values, to_limbs

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_gemm_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_gemm_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
LIMBS = (4, 5, 6, 8, 10)
PAD = 3                         # lda, ldb, ldc exceed the row counts by this
SENTINEL = -7.25                # in the padding rows of C; the padding rows of A and B hold NaN (nothing may read them)
# (m, n, k, transa, transb, alpha, beta): the four op combinations, both alpha and all three beta spread over the shapes
JOBS = ((1, 1, 1, 0, 0, 1, 0), (17, 15, 1, 1, 0, -1, 1), (16, 16, 16, 0, 1, 1, -1), (33, 18, 19, 1, 1, -1, 0), (5, 40, 35, 0, 0, -1, -1),
        (20, 20, 0, 1, 0, 1, 1))


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("clrs_mw_gemm.hip.h", "clrs_mw_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mw_gemm_host.argtypes = [C.c_int, C.c_int, C.POINTER(_lib.MwGemmJob), _lib.p_d, C.c_long, _lib.p_d, C.c_long, _lib.p_d, C.c_long]
    return L


def limb_sums(planes):
    """planar (K, n) -> list of mpmath numbers (exact at the current precision)"""
    return [mp.fsum(mp.mpf(float(planes[l, i])) for l in range(planes.shape[0])) for i in range(planes.shape[1])]


class Batch:
    """Pools and job table of a list of (m, n, k, transa, transb, alpha, beta) with random full-limb operands, and the mpmath reference."""

    def __init__(self, K, shapes, seed, operands=None):
        self.K, self.shapes = K, shapes
        rng = np.random.default_rng(seed)
        mp.mp.prec = 53 * K + 200
        self.where, a_len, b_len, c_len = [], 0, 0, 0
        for m, n, k, ta, tb, al, be in shapes:
            ra, ca, rb, cb = (k, m, n, k) if ta and tb else (k, m, k, n) if ta else (m, k, n, k) if tb else (m, k, k, n)
            self.where.append((a_len, ra, ca, b_len, rb, cb, c_len))
            a_len, b_len, c_len = a_len + (ra + PAD) * ca, b_len + (rb + PAD) * cb, c_len + (m + PAD) * n
        self.A, self.B = np.full((K, max(a_len, 1)), np.nan), np.full((K, max(b_len, 1)), np.nan)
        self.C = np.full((K, max(c_len, 1)), SENTINEL)
        self.table = (_lib.MwGemmJob * len(shapes))()
        self.exact, self.scale = [], []
        for t, ((m, n, k, ta, tb, al, be), (ao, ra, ca, bo, rb, cb, co)) in enumerate(zip(shapes, self.where)):
            self.table[t] = _lib.MwGemmJob(m, n, k, ta, tb, al, be, ra + PAD, rb + PAD, m + PAD, ao, bo, co)
            if operands is not None:
                av, bv, cv = operands[t]
            else:
                av, bv, cv = (rand_values(rng, ra * ca, K), rand_values(rng, rb * cb, K), rand_values(rng, m * n, K))
            a, b, c = (to_limbs(v, K) if len(v) else np.zeros((K, 0)) for v in (av, bv, cv))
            for pool, off, rows, cols, x in ((self.A, ao, ra, ca, a), (self.B, bo, rb, cb, b), (self.C, co, m, n, c)):
                for j in range(cols):
                    pool[:, off + j * (rows + PAD):off + j * (rows + PAD) + rows] = x[:, j * rows:(j + 1) * rows]
            am, bm, cm = limb_sums(a), limb_sums(b), limb_sums(c)             # the values the limbs really hold, column-major
            opa = (lambda i, r: am[r + i * ra]) if ta else (lambda i, r: am[i + r * ra])
            opb = (lambda r, j: bm[j + r * rb]) if tb else (lambda r, j: bm[r + j * rb])
            ex, sc = np.empty((m, n), dtype=object), np.empty((m, n), dtype=object)
            for i in range(m):
                for j in range(n):
                    terms = [opa(i, r) * opb(r, j) for r in range(k)]
                    ex[i, j] = al * mp.fsum(terms) + be * cm[i + j * m]
                    sc[i, j] = mp.fsum(abs(v) for v in terms) + (abs(cm[i + j * m]) if be else 0)
            self.exact.append(ex)
            self.scale.append(sc)

    def pools(self):
        """fresh copies of (A, B, C): C is overwritten by a run"""
        return self.A.copy(), self.B.copy(), self.C.copy()

    def entries(self, Cout, t):
        """planar (K, m * n) of job t, column-major, from a C pool"""
        m, n = self.shapes[t][:2]
        co = self.where[t][6]
        return np.concatenate([Cout[:, co + j * (m + PAD):co + j * (m + PAD) + m] for j in range(n)], axis=1) if n else np.zeros((self.K, 0))

    def check(self, Cout):
        """every entry within the bound of mpmath, padding rows untouched, nothing written that is not finite"""
        K = self.K
        mp.mp.prec = 53 * K + 200
        worst = 0.0
        for t, (m, n, k, ta, tb, al, be) in enumerate(self.shapes):
            got = limb_sums(self.entries(Cout, t))
            assert np.all(np.isfinite(self.entries(Cout, t)))
            co = self.where[t][6]
            for j in range(n):
                assert np.all(Cout[:, co + j * (m + PAD) + m:co + (j + 1) * (m + PAD)] == SENTINEL), ("padding rows of C written", t, j)
                for i in range(m):
                    err, bound = abs(got[i + j * m] - self.exact[t][i, j]), (k + 2) * mp.mpf(2) ** -(52 * K - 2) * self.scale[t][i, j]
                    assert err <= bound, (K, t, i, j, float(err / bound) if bound else float(err))
                    if bound:
                        worst = max(worst, float(err / bound))
        return worst


@functools.lru_cache(maxsize=None)
def issue_batch(K):
    return Batch(K, JOBS, seed=1000 + K)


@functools.lru_cache(maxsize=None)
def cancel_batch(K):
    """one job whose inner product cancels to 2^-80 of its terms (constructed as test_mw_dot_accumulator does), plus beta = +1"""
    mp.mp.prec = 53 * K + 200
    rng = np.random.default_rng(100 + K)
    n = 64
    av, bv = rand_values(rng, n, K), rand_values(rng, n, K)
    av, bv = limb_sums(to_limbs(av, K)), limb_sums(to_limbs(bv, K))
    partial = mp.fsum(x * y for x, y in zip(av[:-1], bv[:-1]))
    av[-1] = -partial / bv[-1] * (1 + mp.mpf(2) ** -80)
    cv = [partial * mp.mpf(2) ** -85]
    return Batch(K, ((1, 1, n, 1, 0, 1, 1),), seed=0, operands=[(av, bv, cv)])


def run_host(batch):
    A, B, Cp = batch.pools()
    assert host_lib().mw_gemm_host(batch.K, len(batch.shapes), batch.table, A.ctypes.data_as(_lib.p_d), A.shape[1], B.ctypes.data_as(_lib.p_d), B.shape[1],
                                   Cp.ctypes.data_as(_lib.p_d), Cp.shape[1]) == 0
    return Cp


def run_device(batch, device=0):
    A, B, Cp = batch.pools()
    _lib.check(_lib.load().clrs_mw_gemm(device, batch.K, len(batch.shapes), batch.table, A.ctypes.data_as(_lib.p_d), A.shape[1], B.ctypes.data_as(_lib.p_d),
                                        B.shape[1], Cp.ctypes.data_as(_lib.p_d), Cp.shape[1]))
    return Cp


# ---- preprocess: both substitutions side by side ---------------------------------------------------------------------------------------------

PLANTS_CE = [(0, {0: 0.5}), (0, {1: 0.25, 3: -0.5}), (0, {2: -0.125})]          # those of test_planted_dependencies_low_rank_instance


def replicate_clusters(sdp, times=2):
    """The ClusteredLowRankSDP with every cluster `times` times (the same free variables): sum_j P_j grows, N does not."""
    import copy
    from clrs_amd.sdp import ClusteredLowRankSDP
    out = ClusteredLowRankSDP(sdp.maximize, sdp.constant, [copy.deepcopy(cl) for _ in range(times) for cl in sdp.blocks], list(sdp.B) * times,
                              list(sdp.c) * times, list(sdp.C) * times, sdp.b, sdp.names)
    out.check()
    return out


def reduced_scales(flat, cs, vr):
    """sum |a b| + |c| of every entry of the reduced B and c (the layout of FlatSDP.B / .c of the reduced problem), from fp64 heads"""
    fv_zeros, fv_nonzeros, Rref, rhs, nf, ff = vr
    N = flat.n_free
    cols = [ff[a] for a in fv_nonzeros]
    R = np.array([[abs(float(Rref[k, pos])) for pos in fv_nonzeros] for k in range(len(nf))], dtype=np.float64).reshape(len(nf), len(cols))
    rh = np.array([abs(float(v)) for v in rhs], dtype=np.float64)
    gone = {(j, p) for _, j, p in cs}
    sB, sc = [np.zeros(0)], [np.zeros(0)]
    for j in range(flat.n_clusters):
        o, P = int(flat.cluster_off[j]), int(flat.cluster_P[j])
        keep = [p for p in range(P) if (j, p) not in gone]
        Bj = np.abs(flat.B[o * N:(o + P) * N].reshape(P, N, order="F"))[keep]
        sB.append((Bj[:, cols] + Bj[:, nf] @ R).reshape(-1, order="F"))
        sc.append(np.abs(flat.c[o:o + P])[keep] + Bj[:, nf] @ rh)
    return np.concatenate(sB), np.concatenate(sc)


def assert_same_reduction(flat, host, dev, D):
    """(reduced, cs, var_rels) of substitute="host" and of "device": the same index sets, reduced B, c, b planes entrywise within TWICE the bound
    (both round the same exact value), with k = N + 1, the contraction length of the device's product"""
    from tests.util import mw_diff
    (rh, ch, vh), (rd, cd, vd) = host, dev
    assert ch == cd
    assert vh[0] == vd[0] and vh[1] == vd[1] and vh[4] == vd[4] and vh[5] == vd[5]
    assert (rh is flat) == (rd is flat)
    if rh is flat:
        return 0.0
    assert rh.n_free == rd.n_free and np.array_equal(rh.cluster_P, rd.cluster_P)
    sB, sc = reduced_scales(flat, ch, vh)
    unit = 2 * (flat.n_free + 1 + 2) * 2.0 ** -(52 * D - 2) * (1 + 1e-9)
    worst = 0.0
    for name, scale in (("B", sB), ("c", sc), ("b", None)):
        a, b = rh.data_planes_of(name, D), rd.data_planes_of(name, D)
        assert a.shape == b.shape
        d = np.abs(mw_diff(a, b))
        if scale is None:                     # b is formed in mpmath by both
            assert np.all(d == 0.0)
            continue
        assert scale.shape == d.shape
        assert np.all(d <= unit * scale), (name, float(np.max(d / np.where(scale > 0, unit * scale, 1.0))))
        if d.size and np.any(scale > 0):
            worst = max(worst, float(np.max(d[scale > 0] / (unit * scale[scale > 0]))))
    return worst

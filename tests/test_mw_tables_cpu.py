"""CPU tests (no GPU) of what a multi-word context derives from a description before it touches a device: the host-only table builder
csrc/clrs_mw_tables.h::mw_build_tables (compiled with g++ through tests/mw_host/mw_tables_host.cpp) against a numpy restatement written
here from the FlatSDP alone -- the tables mean what MwDev (csrc/clrs_mw_kernels.hip.h) says they mean --, its validation messages, and the
digit cutter of the static operands of the exact-product kernels (mw_cut_digits) against mpmath."""
import copy
import ctypes as C
import functools
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib
from tests.util import duplicate_block, flat, permute_cluster_constraints

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_tables_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_tables_host.so")
_CSRC = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc")
ERR_INVALID = -1

i64 = C.c_longlong


class MwBlk(C.Structure):
    """struct MwBlk (csrc/clrs_mw_types.h)"""
    _fields_ = [(n, C.c_int) for n in ("j", "n", "kind", "delta", "U", "cnt", "P", "inv")] + \
               [(n, i64) for n in ("xyoff", "rd_off", "v_off", "vrow_off", "z_off", "g_off", "tptr_off", "a_off", "sd_off", "w_off", "dmap_off", "d0", "t0")] + \
               [("m", C.c_int), ("pad2", C.c_int)]


class MwClu(C.Structure):
    """struct MwClu"""
    _fields_ = [(n, C.c_int) for n in ("P", "b0", "b1", "lds")] + [("coff", i64), ("Soff", i64), ("one_term", C.c_int), ("pad", C.c_int)]


@functools.lru_cache(maxsize=None)
def host_lib():
    deps = [_SRC, os.path.join(_HERE, "..", "include", "clrs_hip.h")] + \
           [os.path.join(_CSRC, f) for f in ("clrs_mw_tables.h", "clrs_mw_types.h", "clrs_mw_slices.h", "clrs_mw_arith.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mwt_build.restype = C.c_void_p
    L.mwt_build.argtypes = [C.POINTER(_lib.SdpDesc), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.mwt_free.argtypes = [C.c_void_p]
    L.mwt_len.restype = C.c_long
    L.mwt_len.argtypes = [C.c_void_p, C.c_char_p]
    L.mwt_width.argtypes = [C.c_void_p, C.c_char_p]
    L.mwt_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    L.mwt_scalar.restype = C.c_double
    L.mwt_scalar.argtypes = [C.c_void_p, C.c_char_p]
    L.mwt_exponent.argtypes = [C.c_double]
    L.mwt_cut.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_float)]
    return L


def planes_of(f, name, DK):
    """(DK, len): the planes of a data array as clrs_amd.mw.MwSchurContext passes them"""
    if DK == 1:
        return np.ascontiguousarray(getattr(f, name), dtype=np.float64).reshape(1, -1)
    return f.data_planes_of(name, DK)


def desc_of(f, DK):
    """the clrs_sdp_desc of a FlatSDP, built as clrs_amd/mw.py builds it, and the arrays it points to"""
    keep = {}

    def hold(name, arr, dt):
        keep[name] = np.ascontiguousarray(arr, dtype=dt)
        return keep[name]

    d = _lib.SdpDesc()
    d.n_clusters, d.n_free, d.n_blocks = f.n_clusters, f.n_free, f.n_blocks
    d.cluster_P = hold("cluster_P", f.cluster_P, np.int32).ctypes.data_as(_lib.p_i32)
    for name in ("block_cluster", "block_m", "block_delta", "block_kind", "term_p", "term_r", "term_s", "term_rank", "dense_p"):
        setattr(d, name, hold(name, getattr(f, name), np.int32).ctypes.data_as(_lib.p_i32))
    for name in ("term_ptr", "term_vec_ptr", "dense_ptr", "dense_A_ptr"):
        setattr(d, name, hold(name, getattr(f, name), np.int64).ctypes.data_as(_lib.p_i64))
    for name in ("B", "term_lambda", "term_vs", "term_ws", "dense_A"):
        setattr(d, name, hold(name, planes_of(f, name, DK), np.float64).ctypes.data_as(_lib.p_d))
    return d, keep


class Tables:
    """Everything mw_build_tables made of (f, DK), copied out; raises nothing: `rc` and `err` say how it went."""
    DTYPES = {4: np.int32, 8: np.float64}

    def __init__(self, f, DK):
        L = host_lib()
        d, keep = desc_of(f, DK)
        rc, err = C.c_int(0), C.create_string_buffer(256)
        h = L.mwt_build(C.byref(d), DK, C.byref(rc), err, 256)
        self.rc, self.err = rc.value, err.value.decode()
        if not h:
            return
        try:
            for name, rec in (("blk", MwBlk), ("clu", MwClu)):
                n = L.mwt_len(h, name.encode())
                assert L.mwt_width(h, name.encode()) == C.sizeof(rec)
                buf = (rec * max(n, 1))()
                assert L.mwt_copy(h, name.encode(), buf) == 0
                setattr(self, name, list(buf)[:n])
            for name in ("lr_list", "dn_list", "V", "dA", "st_lam", "B", "vrow", "tptr", "st_a", "st_b", "st_orig", "st_p", "st_war", "st_wac", "st_trl",
                         "st_trd", "st_flag", "ay_a", "ay_b", "ay_blk", "dmap", "dense_p", "drow_ptr", "drow_blk", "drow_en"):
                n = L.mwt_len(h, name.encode())
                assert n >= 0
                a = np.zeros(n, dtype=self.DTYPES[L.mwt_width(h, name.encode())])
                assert L.mwt_copy(h, name.encode(), a.ctypes.data_as(C.c_void_p)) == 0
                setattr(self, name, a)
            for name in ("J", "N", "NB", "DK", "T", "D", "xlen", "Slen", "xylen", "xrdlen", "zlen", "glen", "sdlen", "wlen", "Vp", "dAp", "lamp", "Bp", "maxU",
                         "maxP", "maxn", "maxn_dense", "maxTb", "maxcnt", "dn_big", "sa_lanes", "n_one_term", "n_many_term"):
                v = L.mwt_scalar(h, name.encode())
                assert v == int(v) and v > -1e299
                setattr(self, name, int(v))
        finally:
            L.mwt_free(h)


# ---- the tables against a restatement from the FlatSDP -------------------------------------------------------------------------------------------

INSTANCES = ("x2p1", "polyopt8", "delsarte_8_3", "ce_8_3", "ns_8_3_2", "sdpa_small", "threepoint_4", "ns_8_3_2_permuted", "polyopt8_dup0")


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "ns_8_3_2_permuted":
        return permute_cluster_constraints(flat("ns_8_3_2"))
    if name == "polyopt8_dup0":
        return duplicate_block(flat("polyopt8"), 0)
    return flat(name)


def check_tables(f, DK, t):
    J, N, NB = f.n_clusters, f.n_free, f.n_blocks
    T, D = int(f.term_ptr[NB]), int(f.dense_ptr[NB])
    vs, ws, lam, dA_in, B_in = (planes_of(f, nm, DK) for nm in ("term_vs", "term_ws", "term_lambda", "dense_A", "B"))
    coff = np.concatenate([[0], np.cumsum(f.cluster_P.astype(np.int64))])
    xlen = int(coff[-1])
    assert (t.J, t.N, t.NB, t.DK, t.T, t.D) == (J, N, NB, DK, T, D)
    assert t.xlen == xlen and t.Slen == int(np.sum(f.cluster_P.astype(np.int64) ** 2)) and t.xylen == f.xy_len and t.xrdlen == int(np.sum(f.block_n))
    assert t.lamp == max(T, 1) and t.Bp == max(xlen * N, 1) and len(t.V) == t.Vp * DK and len(t.dA) == t.dAp * DK
    V, dA, st_lam = t.V.reshape(DK, t.Vp), t.dA.reshape(DK, t.dAp), t.st_lam.reshape(DK, t.lamp)
    # clusters: offsets and block ranges
    for j, cl in enumerate(t.clu):
        mine = [b for b in range(NB) if int(f.block_cluster[b]) == j]
        assert (cl.P, cl.coff, cl.Soff, cl.lds, cl.pad) == (int(f.cluster_P[j]), int(coff[j]), int(np.sum(f.cluster_P[:j].astype(np.int64) ** 2)), 0, 0)
        assert (cl.b0, cl.b1) == ((mine[0], mine[-1] + 1) if mine else (0, 0))
    assert t.maxP == int(np.max(f.cluster_P))
    U_of, zoff, goff, sdoff, woff, rdoff = {}, 0, 0, 0, 0, 0
    drows, most_terms = [], 0
    assert list(t.lr_list) == [b for b in range(NB) if f.block_kind[b] == 0] and list(t.dn_list) == [b for b in range(NB) if f.block_kind[b] != 0]
    for b, k in enumerate(t.blk):
        j, m, dl = int(f.block_cluster[b]), int(f.block_m[b]), int(f.block_delta[b])
        n, P = m * dl, int(f.cluster_P[j])
        assert (k.j, k.n, k.kind, k.delta, k.P, k.m, k.inv, k.pad2) == (j, n, int(f.block_kind[b]), dl, P, m, 0, 0)
        assert (k.xyoff, k.rd_off) == (int(f.block_off[b]), rdoff)
        rdoff += n
        if k.kind == 0:
            t0, t1 = int(f.term_ptr[b]), int(f.term_ptr[b + 1])
            most_terms = max(most_terms, t1 - t0)
            vptr = f.term_vec_ptr

            def vec(arr, tt):
                return arr[:, int(vptr[tt]):int(vptr[tt]) + dl]

            def key(r, x):
                return (r, tuple(x.reshape(-1).tolist()))          # floats compare by ==, every plane

            # distinct (sub-block, vector) pairs in the order of their first occurrence: per term vs at r, ws at r, ws at s, vs at s
            first, partner = {}, {}
            for tt in range(t0, t1):
                r, s = int(f.term_r[tt]), int(f.term_s[tt])
                for kk in (key(r, vec(vs, tt)), key(r, vec(ws, tt)), key(s, vec(ws, tt)), key(s, vec(vs, tt))):
                    first.setdefault(kk, len(first))
                partner[(int(f.term_p[tt]), r, s, int(f.term_rank[tt]))] = tt
            U = len(first)
            U_of[b] = U
            assert k.U == U
            assert (k.t0, k.z_off, k.g_off, k.cnt) == (t0, zoff, goff, 0)
            zoff, goff = zoff + n * U, goff + U * U
            Vb = V[:, k.v_off:k.v_off + n * U].reshape(DK, U, n)               # [plane][column u][row]
            vrow = t.vrow[k.vrow_off:k.vrow_off + U]

            def expanded(r, x):
                e = np.zeros((DK, n))
                e[:, r * dl:(r + 1) * dl] = x
                return e

            for (r, x), u in first.items():
                assert vrow[u] == r * dl
                assert np.array_equal(Vb[:, u, :], expanded(r, np.array(x).reshape(DK, dl)))
            # CSR of the stably p-sorted terms
            order = sorted(range(t0, t1), key=lambda tt: int(f.term_p[tt]))
            tp = t.tptr[k.tptr_off:k.tptr_off + P + 1]
            assert tp[0] == t0
            assert np.array_equal(tp[1:] - t0, np.cumsum(np.bincount(f.term_p[t0:t1], minlength=P)))
            for i, tt in enumerate(order, start=t0):
                r, s = int(f.term_r[tt]), int(f.term_s[tt])
                pt = partner[(int(f.term_p[tt]), s, r, int(f.term_rank[tt]))]
                assert t.st_orig[i] == tt and t.st_p[i] == f.term_p[tt] and tp[t.st_p[i]] <= i < tp[t.st_p[i] + 1]
                assert np.array_equal(st_lam[:, i], lam[:, tt])
                assert t.st_flag[i] == (1 if s <= r else 0) | (2 if s != r else 0)
                for idx, want in ((t.st_b[i], expanded(r, vec(vs, tt))), (t.st_war[i], expanded(r, vec(vs, tt))), (t.st_a[i], expanded(s, vec(ws, pt))),
                                  (t.st_wac[i], expanded(s, vec(ws, tt))), (t.st_trl[i], expanded(r, vec(ws, tt))), (t.st_trd[i], expanded(s, vec(vs, tt)))):
                    assert 0 <= idx < U and np.array_equal(Vb[:, idx, :], want)
            for tt in range(t0, t1):
                r, s = int(f.term_r[tt]), int(f.term_s[tt])
                pt = partner[(int(f.term_p[tt]), s, r, int(f.term_rank[tt]))]
                assert t.ay_blk[tt] == b
                assert np.array_equal(Vb[:, t.ay_a[tt], :], expanded(r, vec(ws, tt)))
                assert np.array_equal(Vb[:, t.ay_b[tt], :], expanded(int(f.term_r[pt]), vec(vs, pt)))
        else:
            d0, d1 = int(f.dense_ptr[b]), int(f.dense_ptr[b + 1])
            assert (k.d0, k.cnt, k.sd_off, k.w_off, k.U) == (d0, d1 - d0, sdoff, woff, 0)
            sdoff, woff = sdoff + (d1 - d0) ** 2, woff + (d1 - d0) * n * n
            want_map = np.full(P, -1)
            for e in range(d0, d1):
                want_map[int(f.dense_p[e])] = e - d0
                drows.append((int(coff[j]) + int(f.dense_p[e]), b, e - d0))
                a0 = int(f.dense_A_ptr[e])
                assert np.array_equal(dA[:, k.a_off + (e - d0) * n * n:k.a_off + (e - d0 + 1) * n * n], dA_in[:, a0:a0 + n * n])
            assert np.array_equal(t.dmap[k.dmap_off:k.dmap_off + P], want_map)
    assert (t.zlen, t.glen, t.sdlen, t.wlen) == (zoff, goff, sdoff, woff)
    assert t.maxU == max(U_of.values(), default=0) and t.maxn == int(np.max(f.block_n)) and t.maxTb == most_terms
    dense = [k for k in t.blk if k.kind != 0]
    assert t.maxn_dense == max((k.n for k in dense), default=0) and t.maxcnt == max((k.cnt for k in dense), default=0)
    assert t.dn_big == (1 if any(k.n > 1 for k in dense) else 0)
    assert np.array_equal(t.dense_p, f.dense_p[:D])
    # the dense entries per stacked constraint row
    drows.sort()
    assert np.array_equal(t.drow_ptr, np.concatenate([[0], np.cumsum(np.bincount([g for g, _, _ in drows], minlength=xlen))]))
    assert list(t.drow_blk) == [bb for _, bb, _ in drows] and list(t.drow_en) == [e for _, _, e in drows]
    # the stacked B
    want_B = np.zeros((DK, max(xlen * N, 1)))
    for j in range(J):
        P, o = int(f.cluster_P[j]), int(coff[j])
        for a in range(N):
            want_B[:, o + a * xlen:o + a * xlen + P] = B_in[:, o * N + a * P:o * N + (a + 1) * P]
    assert np.array_equal(t.B.reshape(DK, t.Bp), want_B)
    # S_j through k_mw_saccum_one: 32 clusters or more, one to four blocks, at most one low-rank term per (constraint, block)
    widest = max((cl.b1 - cl.b0 for cl in t.clu), default=1)
    assert t.sa_lanes == (4 if widest >= 3 else max(widest, 1))
    for j, cl in enumerate(t.clu):
        one = J >= 32 and 1 <= cl.b1 - cl.b0 <= 4 and all(
            np.max(np.bincount(f.term_p[int(f.term_ptr[b]):int(f.term_ptr[b + 1])], minlength=1)) <= 1 for b in range(cl.b0, cl.b1) if f.block_kind[b] == 0)
        assert cl.one_term == int(one)
    assert t.n_one_term == sum(cl.one_term for cl in t.clu) and t.n_one_term + t.n_many_term == J
    return U_of


@pytest.mark.parametrize("DK", [1, 2])
@pytest.mark.parametrize("name", INSTANCES)
def test_tables_mean_what_mwdev_says(name, DK, oracle_built):
    """Every table of mw_build_tables against the restatement above; the unique-vector count of a block against the oracle's per sub-block counts
    (oracle_unique_counts: unique vs / unique ws of the terms with r = the sub-block, fp64 heads) -- the table merges the two sets of a sub-block, so
    U = their sum over the sub-blocks where vs == ws in every term, and lies between the larger sum and both sums otherwise."""
    from oracle.oracle import Oracle
    f = problem(name)
    t = Tables(f, DK)
    assert t.rc == 0, t.err
    U_of = check_tables(f, DK, t)
    if DK == 1:
        o = Oracle(f, use_lo=False)
        for b, U in U_of.items():
            UR, UL = o.unique_counts(b)
            v0, v1 = int(f.term_vec_ptr[f.term_ptr[b]]), int(f.term_vec_ptr[f.term_ptr[b + 1]])
            if np.array_equal(f.term_vs[v0:v1], f.term_ws[v0:v1]):
                assert U == int(np.sum(UR)) == int(np.sum(UL))
            else:
                assert max(int(np.sum(UR)), int(np.sum(UL))) <= U <= int(np.sum(UR)) + int(np.sum(UL))


def test_tables_have_subblock_terms_and_dense_blocks():
    """the instances above do reach the cases they are there for: r != s terms with partners, dense blocks of more than one row, duplicates removed"""
    f = problem("ns_8_3_2")
    assert np.any(f.term_r != f.term_s) and np.max(f.block_m) >= 2
    t = Tables(f, 1)
    assert np.any(t.st_flag & 2) and np.any((t.st_flag & 1) == 0)
    assert any(k.kind == 0 and k.U < 2 * (int(f.term_ptr[b + 1]) - int(f.term_ptr[b])) for b, k in enumerate(t.blk))
    assert Tables(problem("sdpa_small"), 1).dn_big == 1


# ---- validation without a GPU ------------------------------------------------------------------------------------------------------------------

def _modified(name, **arrays):
    g = copy.copy(flat(name))
    for k, fn in arrays.items():
        a = getattr(g, k).copy()
        fn(a)
        setattr(g, k, a)
    return g


def _no_partner():
    from tests.test_hip_parity import _mini_sdp
    sdp = _mini_sdp(m=2, drop_partner=True)
    sdp.check = lambda: None                      # (the host-side check would refuse it first)
    return clrs_amd.flatten(sdp)


def _set(i, v):
    def fn(a):
        a[i] = v
    return fn


def _add(i, v):
    def fn(a):
        a[i] += v
    return fn


def _dense_block(name):
    f = flat(name)
    return next(b for b in range(f.n_blocks) if f.block_kind[b] != 0)


MALFORMED = {
    "partner": (_no_partner, 1, "term without transposed partner: A[r,s][p] must equal A[s,r][p]^T"),
    "block_cluster": (lambda: _modified("ns_8_3_2", block_cluster=_set(-1, 0)), 1, "block_cluster must be non-decreasing and within range"),
    "term_index": (lambda: _modified("polyopt8", term_p=_set(0, int(flat("polyopt8").cluster_P[0]))), 1, "term index out of range"),
    "term_sub_block": (lambda: _modified("polyopt8", term_s=_set(0, 1)), 1, "term index out of range"),
    "vector_length": (lambda: _modified("polyopt8", term_vec_ptr=_add(slice(1, None), 1)), 1, "term vectors must have delta entries"),
    "dense_size": (lambda: _modified("sdpa_small", dense_A_ptr=_add(slice(1, None), 1)), 1, "dense matrix must have n*n entries"),
    "asymmetric": (lambda: _modified("sdpa_small", dense_A=_add(1, 0.5)), 1, "dense constraint matrices must be symmetric"),
    "asymmetric_plane_1": (lambda: _modified("sdpa_small", dense_A_lo=_add(1, 2.0 ** -60)), 2, "dense constraint matrices must be symmetric"),
    "dense_m": (lambda: _modified("sdpa_small", block_m=_set(_dense_block("sdpa_small"), 2)), 1, "bad block shape"),
    "empty_cluster": (lambda: _modified("ns_8_3_2", cluster_P=_set(1, 0)), 1, "cluster without constraints"),
    # two at once: the clusters are looked at before any block
    "first_wins": (lambda: _modified("polyopt8", term_p=_set(0, -1), cluster_P=_set(-1, -3)), 1, "cluster without constraints"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_descriptions_are_refused_without_a_device(case):
    make, DK, message = MALFORMED[case]
    g = make()
    if case == "block_cluster":
        assert g.block_cluster[-1] < g.block_cluster[-2]
    if case.startswith("asymmetric"):
        assert flat("sdpa_small").block_n[0] > 1 and flat("sdpa_small").block_kind[0] != 0
    t = Tables(g, DK)
    assert (t.rc, t.err) == (ERR_INVALID, message)


def test_asymmetry_in_the_second_plane_needs_the_second_plane():
    """... the same description is fine when only the fp64 heads are passed"""
    make, _, _ = MALFORMED["asymmetric_plane_1"]
    assert Tables(make(), 1).rc == 0


# ---- the digit cutter ----------------------------------------------------------------------------------------------------------------------------

def _double_doubles():
    """400 (x0, x1) with x0 = fl(x0 + x1) over 40 binades: zeros, both signs, tails of either sign, tails far below the head, short values"""
    rng = np.random.default_rng(2024)
    out = []
    for i in range(400):
        if i % 50 == 0:
            out.append((0.0, 0.0))
            continue
        binade = i % 40 - 20
        h = float(np.ldexp(rng.uniform(0.5, 1.0), binade)) * (-1.0 if i % 3 == 0 else 1.0)
        if i % 7 == 0:                                   # a few bits only: nothing below the last slice
            h = float(np.ldexp(float(rng.integers(1, 1 << 20)), binade - 20))
            out.append((h, 0.0))
            continue
        gap = (0, 0, 30, 300)[i % 4]                     # tails right below the head, and far below it (2^-356 of the head: below the last slice, 2^-345 at 6 limbs)
        tail = float(np.ldexp(rng.uniform(0.5, 1.0), binade - 54 - gap)) * (-1.0 if i % 2 == 0 else 1.0)
        s = h + tail
        out.append((s, tail - (s - h)))
    assert sum(1 for a, b in out if a * b < 0) > 50 and sum(1 for a, b in out if a < 0) > 50
    return out


@pytest.mark.parametrize("K", [4, 5, 6])
def test_digit_cutter(K):
    """mw_cut_digits at S = mws_slices(K): every digit an integer that fp32 holds (|d| <= 2^(beta - 1) + 1), and 2^e sum_s d[s] 2^-(s+1) beta is x0 + x1
    exactly where the value has no bits below the last slice, within 2^(e - S beta) of it otherwise (every slice rounds the head of the remainder to
    nearest: what is left after S of them is at most half a step of the last grid, plus a tail below that)."""
    L = host_lib()
    beta, S = L.mwt_beta(), L.mwt_slices(K)
    assert beta == 23 and S == (52 * K + 16 + beta - 1) // beta
    exact = inexact = 0
    with mp.workprec(2200):
        for i, (x0, x1) in enumerate(_double_doubles()):
            e = L.mwt_exponent(x0) + i % 4               # (the callers cut at the exponent of a column's largest entry: never below the value's own)
            d = (C.c_float * S)()
            L.mwt_cut(x0, x1, e, S, d)
            d = [float(v) for v in d]
            assert all(v == int(v) and abs(v) <= 2 ** (beta - 1) + 1 for v in d), (x0, x1, d)
            x = mp.mpf(x0) + mp.mpf(x1)
            got = mp.ldexp(mp.fsum(mp.ldexp(mp.mpf(v), -(s + 1) * beta) for s, v in enumerate(d)), e)
            if mp.isint(mp.ldexp(x, S * beta - e)):
                assert got == x, (x0, x1, e)
                exact += 1
            else:
                assert abs(got - x) < mp.ldexp(mp.mpf(1), e - S * beta), (x0, x1, e)
                inexact += 1
    assert exact > 100 and inexact > 20, (exact, inexact)

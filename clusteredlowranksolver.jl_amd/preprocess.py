"""Detect and remove linear dependencies before solving: the reference's `preprocess!` / `postprocess` (src/pre_postprocessing.jl).

The reference factors the dense matrix (all PSD entries) x (all constraints) by a column-pivoted QR.  Here the same information comes
from the Gram matrices of the constraint matrices, cluster by cluster: G_j[p, q] = sum_l <A_p, A_q> = S_j(X = I, Y = I), which the
assembly kernels produce at any limb count, and R_ii^2 of the reference's QR is pivot i of the diagonally pivoted Cholesky of G_j
(`clrs_mw_constraint_dependencies`, csrc/clrs_mw_rank.hip.h).  Dependencies cannot cross clusters (clusters share no PSD block).

    flat = flatten(sdp)
    reduced, cs, var_rels = preprocess(flat, prec=256)         # `reduced is flat` when nothing was found
    res = solvesdp_mw(reduced, ...)
    x, y = postprocess(res.x, res.y, cs, var_rels)             # original numbering

`cs = [(i, j, p)]`: removed constraint p of cluster j, i its index in the x layout (0-based).  `var_rels = (fv_zeros, fv_nonzeros, Rref,
rhs_changed, nf_vars, ff_vars)` with the reference's meaning: `[I Rref] [y_nf; y_ff] = rhs_changed` fixes the variables `nf_vars` by
the free ones `ff_vars`; `fv_zeros` / `fv_nonzeros` are positions in `ff_vars` of the variables set to zero / kept.  `Rref` and
`rhs_changed` are mpmath numbers.

Precision and thresholds.  The reference decides at tol = sqrt(eps(BigFloat)) on |R_ii|, i.e. at eps = 2^-(prec - 1) on a Gram pivot.
A Gram pivot of an exact dependency is rounding noise of about 2^-(52 D) max G_ii, so detection runs at D limbs, the smallest of 4, 5,
6, 8, 10 with 52 D >= prec + 32 (6 for the default 256 bits), with the data planes zero padded, and

    tau = max(2^-(prec - 1), 2^-(52 D - 32) max_p G[p, p]).

The second term is a DEVIATION from the reference's absolute threshold: it keeps rounding noise from being read as independence when
the data are large.  For prec > 488 the limb count stays at D = 10 and the second term governs.
A second deviation: `FlatSDP.constant` is a Python float, so the constant of the reduced problem is rounded to fp64 there; the exact
value is `var_rels.constant`.

The rank-revealing steps are a parameter (`reveal`): None = the device primitives of libclrs_hip.so.  The package has no CPU
implementation of them; the tests drive the host-side steps with one of their own (tests/preprocess_host.py).

The substitution is a parameter too (`substitute`).  "host" (the default) forms every quantity entry by entry in mpmath at 52 D bits.  "device" forms
everything whose size grows with the number of constraints -- the conditions on the free variables, their Gram matrix, the Gram matrix of the
remaining free variables and the reduced B and c -- as batched multi-word products on limb planes (`reveal.gemm_batch`, `clrs_mw_gemm`); only
the r x (N + 1 - r) relation coefficients `var_rels` promises as mpmath numbers, the residual test, b and the constant stay in mpmath.  Both round
the same exact values to D limbs, so the reduced problems agree to the accuracy of D limbs, not bit for bit.
"""
from __future__ import annotations

import copy
from typing import List, Optional

import numpy as np

from .sdp import DATA_ARRAYS, FlatSDP, flatten

LINDEP_MESSAGE = "Linear dependent constraint(s) resulting in a constraint 0 = b_i with b_i nonzero."
DETECT_LIMBS = (4, 5, 6, 8, 10)


def detect_limbs(prec: int) -> int:
    """Limbs of the detection: the smallest of 4, 5, 6, 8, 10 with 52 D >= prec + 32 (10 beyond that)."""
    for D in DETECT_LIMBS:
        if 52 * D >= prec + 32:
            return D
    return DETECT_LIMBS[-1]


def threshold(prec: int, D: int, max_diag: float) -> float:
    """tau = max(2^-(prec - 1), 2^-(52 D - 32) max_diag): pivots at or below it count as zero."""
    return max(2.0 ** -(prec - 1), 2.0 ** -(52 * D - 32) * max(float(max_diag), 0.0))


class VarRels(tuple):
    """(fv_zeros, fv_nonzeros, Rref, rhs_changed, nf_vars, ff_vars) plus `.constant`: the exact constant of the reduced problem (mpmath)."""
    constant = None


class DeviceReveal:
    """The rank-revealing steps on the device, for one FlatSDP at D limbs (a temporary context of its own)."""

    def __init__(self, flat: FlatSDP, D: int, device: int = 0):
        from .mw import MwSchurContext
        self.D, self.device = D, device
        self.ctx = MwSchurContext(flat, limbs=D, device=device, data_limbs=D if flat.tails else 2) if flat.n_clusters else None

    def gram_diag(self) -> List[np.ndarray]:
        """fp64 heads of the diagonal of every G_j"""
        f = self.ctx.flat
        G = self.ctx.constraint_gram()
        return [G[0, int(f.S_off[j]):int(f.S_off[j + 1])].reshape(int(f.cluster_P[j]), -1).diagonal().copy() for j in range(f.n_clusters)]

    def dependencies(self, tau):
        """per cluster (perm, r, W planar (D, r (P - r)), resid planar (D, P - r))"""
        f = self.ctx.flat
        perm, rank, W, resid = self.ctx.constraint_dependencies(tau)
        out = []
        for j in range(f.n_clusters):
            P, r, o, so = int(f.cluster_P[j]), int(rank[j]), int(f.cluster_off[j]), int(f.S_off[j])
            out.append((perm[o:o + P].copy(), r, W[:, so:so + r * (P - r)].copy(), resid[:, o:o + P - r].copy()))
        return out

    def free_gram(self) -> np.ndarray:
        return self.ctx.free_gram()

    def rank_reveal(self, G, n: int, ncand: int, tau: float):
        from .mw import rank_reveal
        return rank_reveal(G, [n], [ncand], [tau], self.D, self.device)[0]

    def gemm_batch(self, jobs):
        """[(A, B, C or None, transa, transb, alpha, beta)] -> [C <- beta C + alpha op(A) op(B)] on planes (planes, rows, cols), D limbs, one call
        (needs no context: `preprocess` still calls it after `close`)"""
        from .mw import gemm_batch
        return gemm_batch(jobs, self.D, self.device)

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None


# ---- host helpers: planar limbs <-> mpmath -----------------------------------------------------------------------------------

def _mp():
    import mpmath as mp
    return mp


def _mp_sum(planes) -> np.ndarray:
    """planar (k, ...) floats -> object array (...) of mpmath numbers (exact sums at the current precision's worth of bits)"""
    mp = _mp()
    planes = np.asarray(planes, dtype=np.float64)
    out = np.empty(planes.shape[1:], dtype=object)
    for idx in np.ndindex(*planes.shape[1:]):
        out[idx] = mp.fsum(mp.mpf(float(planes[(l,) + idx])) for l in range(planes.shape[0]) if planes[(l,) + idx] != 0.0)
    return out


def _split(a, planes: int) -> np.ndarray:
    """object array of mpmath numbers -> planar (planes, ...) by successive roundings"""
    mp = _mp()
    a = np.asarray(a, dtype=object)
    out = np.zeros((planes,) + a.shape)
    for idx in np.ndindex(*a.shape):
        r = mp.mpf(a[idx])
        for l in range(planes):
            h = float(r)
            out[(l,) + idx] = h
            if h == 0.0:
                break
            r = r - mp.mpf(h)
    return out


def _dot(u, v):
    mp = _mp()
    return mp.fsum(a * b for a, b in zip(u, v))


def _n_planes(flat: FlatSDP) -> int:
    nt = 0
    for t in (flat.tails or {}).values():
        nt = max(nt, t.shape[0])
    return 2 + nt


def _has_blocks(flat: FlatSDP) -> np.ndarray:
    has = np.zeros(flat.n_clusters, dtype=bool)
    has[np.asarray(flat.block_cluster, dtype=np.int64)] = True
    return has


def select_constraints(flat: FlatSDP, keep: List[np.ndarray], drop_empty: bool = True, B_planes=None, c_planes=None, b_planes=None,
                       constant: Optional[float] = None) -> FlatSDP:
    """The FlatSDP with only the constraints keep[j] (increasing cluster-local indices) of every cluster, renumbered; clusters left with
    neither constraints nor blocks are dropped.  `B_planes` / `c_planes`: per cluster (planes, P'_j, N') / (planes, P'_j) arrays, `b_planes` (planes, N'): replacement data
    of the kept rows after the free-variable substitution."""
    J, N = flat.n_clusters, flat.n_free
    npl = _n_planes(flat)
    has = _has_blocks(flat)
    keep = [np.asarray(k, dtype=np.int64) for k in keep]
    alive = [j for j in range(J) if has[j] or len(keep[j]) or not drop_empty]
    newj = {j: i for i, j in enumerate(alive)}
    newp = []
    for j in range(J):
        m = -np.ones(int(flat.cluster_P[j]), dtype=np.int64)
        m[keep[j]] = np.arange(len(keep[j]))
        newp.append(m)
    stack = {name: flat.data_planes_of(name, npl) for name in DATA_ARRAYS}
    out_pl = {}
    # rows of B and c
    if B_planes is None:
        Bs = []
        for j in alive:
            o, P = int(flat.cluster_off[j]), int(flat.cluster_P[j])
            Bj = stack["B"][:, o * N:(o + P) * N].reshape(npl, N, P)          # column-major P x N per plane: [plane, column, row]
            Bs.append(Bj[:, :, keep[j]].reshape(npl, -1))
        out_pl["B"] = np.concatenate(Bs, axis=1) if Bs else np.zeros((npl, 0))
        Nn = N
    else:
        Nn = B_planes[0].shape[2] if B_planes else 0
        pl = max([npl] + [x.shape[0] for x in B_planes])
        Bs = [np.transpose(B_planes[j], (0, 2, 1)).reshape(B_planes[j].shape[0], -1) for j in alive]      # column-major P' x N' per plane
        Bs = [np.pad(x, ((0, pl - x.shape[0]), (0, 0))) for x in Bs]
        out_pl["B"] = np.concatenate(Bs, axis=1) if Bs else np.zeros((pl, 0))
    if c_planes is None:
        cs_ = [stack["c"][:, int(flat.cluster_off[j]) + keep[j]] for j in alive]
    else:
        cs_ = [c_planes[j] for j in alive]
    plc = max([npl] + [x.shape[0] for x in cs_])
    out_pl["c"] = np.concatenate([np.pad(x, ((0, plc - x.shape[0]), (0, 0))) for x in cs_], axis=1) if cs_ else np.zeros((plc, 0))
    out_pl["b"] = stack["b"] if b_planes is None else b_planes
    out_pl["C"] = stack["C"]
    # terms and dense entries of the kept constraints
    tsel, dsel, term_ptr, dense_ptr = [], [], [0], [0]
    for b in range(flat.n_blocks):
        j = int(flat.block_cluster[b])
        for t in range(int(flat.term_ptr[b]), int(flat.term_ptr[b + 1])):
            if newp[j][int(flat.term_p[t])] >= 0:
                tsel.append(t)
        for e in range(int(flat.dense_ptr[b]), int(flat.dense_ptr[b + 1])):
            if newp[j][int(flat.dense_p[e])] >= 0:
                dsel.append(e)
        term_ptr.append(len(tsel)); dense_ptr.append(len(dsel))
    tsel, dsel = np.array(tsel, dtype=np.int64), np.array(dsel, dtype=np.int64)
    tj = flat.block_cluster[np.searchsorted(flat.term_ptr, tsel, side="right") - 1] if len(tsel) else np.zeros(0, np.int64)
    dj = flat.block_cluster[np.searchsorted(flat.dense_ptr, dsel, side="right") - 1] if len(dsel) else np.zeros(0, np.int64)
    term_p = np.array([newp[int(j)][int(flat.term_p[t])] for j, t in zip(tj, tsel)], dtype=np.int32)
    dense_p = np.array([newp[int(j)][int(flat.dense_p[e])] for j, e in zip(dj, dsel)], dtype=np.int32)

    def gather(ptr, sel):
        idx = [np.arange(int(ptr[t]), int(ptr[t + 1])) for t in sel]
        lens = np.array([len(i) for i in idx], dtype=np.int64)
        return (np.concatenate(idx) if idx else np.zeros(0, np.int64)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    vidx, term_vec_ptr = gather(flat.term_vec_ptr, tsel)
    aidx, dense_A_ptr = gather(flat.dense_A_ptr, dsel)
    out_pl["term_lambda"] = stack["term_lambda"][:, tsel]
    out_pl["term_vs"], out_pl["term_ws"] = stack["term_vs"][:, vidx], stack["term_ws"][:, vidx]
    out_pl["dense_A"] = stack["dense_A"][:, aidx]
    cluster_P = np.array([len(keep[j]) for j in alive], dtype=np.int32)
    g = copy.copy(flat)
    g.n_clusters, g.n_free, g.cluster_P = len(alive), Nn, cluster_P
    g.block_cluster = np.array([newj[int(j)] for j in flat.block_cluster], dtype=np.int32)
    g.term_ptr, g.dense_ptr = np.array(term_ptr, dtype=np.int64), np.array(dense_ptr, dtype=np.int64)
    g.term_p, g.dense_p = term_p, dense_p
    for name in ("term_r", "term_s", "term_rank"):
        setattr(g, name, np.asarray(getattr(flat, name))[tsel].astype(np.int32))
    g.term_vec_ptr, g.dense_A_ptr = term_vec_ptr, dense_A_ptr
    tails = {}
    ntail = max(x.shape[0] for x in out_pl.values()) - 2
    for name in DATA_ARRAYS:
        pl = out_pl[name]
        pl = np.pad(pl, ((0, max(0, 2 - pl.shape[0])), (0, 0)))
        setattr(g, name, np.ascontiguousarray(pl[0]))
        setattr(g, name + "_lo", np.ascontiguousarray(pl[1]))
        if ntail > 0:
            tails[name] = np.ascontiguousarray(np.pad(pl[2:], ((0, ntail - (pl.shape[0] - 2)), (0, 0))))
    g.tails = tails if ntail > 0 and any(np.any(t != 0.0) for t in tails.values()) else {}
    g.cluster_off = np.concatenate([[0], np.cumsum(cluster_P.astype(np.int64))]).astype(np.int64)
    g.S_off = np.concatenate([[0], np.cumsum(cluster_P.astype(np.int64) ** 2)]).astype(np.int64)
    if constant is not None:
        g.constant = float(constant)
    return g


# ---- the reference's three functions ------------------------------------------------------------------------------------------

SUBSTITUTE = ("host", "device")


def find_linear_dependencies(flat: FlatSDP, prec: int = 256, reveal=None, device: int = 0, substitute: str = "host"):
    """Steps 1, 2 and 4 of src/pre_postprocessing.jl:4-137 on Gram matrices.  Returns (cs, var_rels, work): the removed constraints, the
    relations between the free variables, and `work` = what `preprocess` needs to substitute (kept sets, D).
    `reveal`: None = the device (`DeviceReveal`), or a callable (flat, D) -> an object with the same methods.
    `substitute`: "host" = every product in mpmath; "device" = the products over constraints through `reveal.gemm_batch` (module docstring)."""
    mp = _mp()
    if substitute not in SUBSTITUTE:
        raise ValueError(f"substitute must be one of {SUBSTITUTE}, got {substitute!r}")
    D = detect_limbs(prec)
    J, N = flat.n_clusters, flat.n_free
    has = _has_blocks(flat)
    dev_clusters = [j for j in range(J) if has[j]]
    # clusters without PSD blocks have a zero Gram matrix: every constraint of theirs is a pure condition on the free variables.  They are
    # kept away from the device context (a cluster without blocks has nothing to assemble) and treated as zero Gram rows here.
    fdev = flat if len(dev_clusters) == J else _only_clusters(flat, dev_clusters)
    rv = (DeviceReveal(fdev, D, device) if reveal is None else reveal(fdev, D))
    try:
        if substitute == "device":
            if not hasattr(rv, "gemm_batch"):
                raise ValueError('substitute="device" needs a `reveal` object with a gemm_batch method')
            if _n_planes(flat) > D:
                raise ValueError(f'substitute="device": the data carry {_n_planes(flat)} limb planes, the detection runs at {D}')
        with mp.workprec(52 * D):
            return _find(flat, fdev, dev_clusters, rv, prec, D, substitute == "device")
    finally:
        rv.close()


def _only_clusters(flat: FlatSDP, clusters: List[int]) -> FlatSDP:
    """`flat` restricted to `clusters` (all of which own blocks; the others own none), tails kept"""
    g = copy.copy(flat)
    N = flat.n_free
    newj = {j: i for i, j in enumerate(clusters)}
    rows = np.concatenate([np.arange(int(flat.cluster_off[j]), int(flat.cluster_off[j + 1])) for j in clusters]) if clusters else np.zeros(0, np.int64)
    bidx = np.concatenate([np.arange(int(flat.cluster_off[j]) * N, int(flat.cluster_off[j + 1]) * N) for j in clusters]) if clusters else np.zeros(0, np.int64)
    g.n_clusters = len(clusters)
    g.cluster_P = flat.cluster_P[clusters].astype(np.int32) if clusters else np.zeros(0, np.int32)
    g.B, g.B_lo, g.c, g.c_lo = flat.B[bidx], flat.B_lo[bidx], flat.c[rows], flat.c_lo[rows]
    g.block_cluster = np.array([newj[int(j)] for j in flat.block_cluster], dtype=np.int32)
    g.tails = dict(flat.tails) if flat.tails else {}
    if g.tails:
        g.tails["B"], g.tails["c"] = flat.tails["B"][:, bidx], flat.tails["c"][:, rows]
    g.cluster_off = np.concatenate([[0], np.cumsum(g.cluster_P.astype(np.int64))]).astype(np.int64)
    g.S_off = np.concatenate([[0], np.cumsum(g.cluster_P.astype(np.int64) ** 2)]).astype(np.int64)
    return g


def _find(flat, fdev, dev_clusters, rv, prec, D, on_device=False):
    mp = _mp()
    J, N = flat.n_clusters, flat.n_free
    npl = _n_planes(flat)
    Bpl, cpl = flat.data_planes_of("B", npl), flat.data_planes_of("c", npl)

    def B_rows(j, rows):
        """rows of B_j as an object array (len(rows), N) of mpmath numbers"""
        o, P = int(flat.cluster_off[j]), int(flat.cluster_P[j])
        Bj = Bpl[:, o * N:(o + P) * N].reshape(npl, N, P)
        return _mp_sum(np.transpose(Bj[:, :, rows], (0, 2, 1)))

    def c_rows(j, rows):
        return _mp_sum(cpl[:, int(flat.cluster_off[j]) + np.asarray(rows, dtype=np.int64)])

    def Bc_planes(j, rows):
        """rows of [B_j | c_j] as planes (npl, len(rows), N + 1): gathers are exact on planes"""
        o, P = int(flat.cluster_off[j]), int(flat.cluster_P[j])
        rows = np.asarray(rows, dtype=np.int64)
        out = np.empty((npl, len(rows), N + 1))
        out[:, :, :N] = np.transpose(Bpl[:, o * N:(o + P) * N].reshape(npl, N, P)[:, :, rows], (0, 2, 1))
        out[:, :, N] = cpl[:, o + rows]
        return out

    def padD(a):
        return np.pad(a, ((0, D - a.shape[0]),) + ((0, 0),) * (a.ndim - 1))

    # 1. constraints: per cluster the kept set, the removed set and the relations W_j
    kept = [np.zeros(0, np.int64) for _ in range(J)]
    removed = [np.arange(int(flat.cluster_P[j]), dtype=np.int64) for j in range(J)]
    rel = [None] * J
    if dev_clusters:
        tau = [threshold(prec, D, np.max(d) if len(d) else 0.0) for d in rv.gram_diag()]
        for jd, (perm, r, W, _res) in enumerate(rv.dependencies(np.array(tau))):
            j = dev_clusters[jd]
            kept[j], removed[j] = np.asarray(perm[:r], dtype=np.int64), np.asarray(perm[r:], dtype=np.int64)
            if not (r and len(removed[j])):
                rel[j] = None
            elif on_device:
                rel[j] = np.transpose(np.asarray(W).reshape(D, len(removed[j]), r), (0, 2, 1))        # the same as planes (D, r, removed)
            else:
                rel[j] = _mp_sum(W).reshape(len(removed[j]), r).T      # r x removed (column-major r x (P - r))
    cs = [(int(flat.cluster_off[j]) + int(p), j, int(p)) for j in range(J) for p in sorted(removed[j])]
    nrem = len(cs)
    # 2. conditions on the free variables: F y = g, one row per removed constraint
    Mpl = None
    if on_device:
        if nrem:
            # [F | g]_j = [B | c]_removed - W_j^T [B | c]_kept as one batch over the clusters (C preloaded with the removed rows), stacked into Mpl (D, nrem, N + 1)
            parts, jobs = [], []
            for j in range(J):
                if not len(removed[j]):
                    continue
                rs = np.sort(removed[j])
                Cr = Bc_planes(j, rs)
                if rel[j] is None:
                    parts.append(padD(Cr))
                    continue
                order = {int(p): i for i, p in enumerate(removed[j])}
                parts.append(len(jobs))
                jobs.append((rel[j][:, :, [order[int(p)] for p in rs]], Bc_planes(j, kept[j]), Cr, 1, 0, -1, 1))
            done = rv.gemm_batch(jobs) if jobs else []
            Mpl = np.concatenate([done[x] if isinstance(x, int) else x for x in parts], axis=1)
    else:
        F, g = np.empty((nrem, N), dtype=object), np.empty(nrem, dtype=object)
        row = 0
        removed_B = []
        for j in range(J):
            if not len(removed[j]):
                continue
            rs = np.sort(removed[j])
            order = {int(p): i for i, p in enumerate(removed[j])}
            Br, cr = B_rows(j, rs), c_rows(j, rs)
            removed_B.append(Br)
            Bk, ck = (B_rows(j, kept[j]), c_rows(j, kept[j])) if len(kept[j]) else (None, None)
            for i, p in enumerate(rs):
                w = rel[j][:, order[int(p)]] if rel[j] is not None else None
                for a in range(N):
                    F[row, a] = Br[i, a] - (_dot(w, Bk[:, a]) if w is not None else 0)
                g[row] = cr[i] - (_dot(w, ck) if w is not None else 0)
                row += 1
    nf, ff = [], list(range(N))
    Rref, rhs = np.empty((0, N), dtype=object), np.empty(0, dtype=object)
    Rref_pl, rhs_pl = np.zeros((D, 0, N)), np.zeros((D, 0))
    if nrem:
        n = N + 1
        if on_device:
            Gp = rv.gemm_batch([(Mpl, Mpl, None, 1, 0, 1, 0)])[0]                      # [F g]^T [F g], (D, n, n)
            tau2 = threshold(prec, D, max([float(v) for v in Gp[0].diagonal()[:N]] + [0.0]))
            perm, r, W, res = rv.rank_reveal(np.transpose(Gp, (0, 2, 1)).reshape(D, -1), n, N, tau2)
            Gnn = _mp_sum(Gp[:, N, N].reshape(D, 1))[0]
        else:
            M = np.concatenate([F, g.reshape(-1, 1)], axis=1)
            G = np.empty((n, n), dtype=object)
            for a in range(n):
                for b in range(a + 1):
                    G[a, b] = G[b, a] = _dot(M[:, a], M[:, b])
            tau2 = threshold(prec, D, max([float(G[a, a]) for a in range(N)] + [0.0]))
            perm, r, W, res = rv.rank_reveal(_split(G.reshape(-1, order="F"), D), n, N, tau2)
            Gnn = G[N, N]
        perm = [int(v) for v in perm]
        nf, rest = perm[:r], perm[r:]
        gi = rest.index(N)
        resid_g = _mp_sum(res)[gi]
        if resid_g > max(mp.mpf(2) ** -(prec - 1), mp.mpf(2) ** -(52 * D - 32) * max(mp.mpf(1), Gnn)):
            raise ValueError(LINDEP_MESSAGE)
        ff = [v for v in rest if v != N]
        Wm = _mp_sum(W).reshape(len(rest), r).T if r else np.empty((0, len(rest)), dtype=object)
        Rref = Wm[:, [rest.index(v) for v in ff]] if r else np.empty((0, len(ff)), dtype=object)
        rhs = Wm[:, gi] if r else np.empty(0, dtype=object)
        if on_device and r:                      # the same coefficients as the planes rank_reveal returned (never through mpmath and back)
            Wp = np.transpose(np.asarray(W).reshape(D, len(rest), r), (0, 2, 1))
            Rref_pl, rhs_pl = Wp[:, :, [rest.index(v) for v in ff]], Wp[:, :, gi]
        elif on_device:
            Rref_pl = np.zeros((D, 0, len(ff)))
    # 4. free variables that do the same job: rank of B[kept] changemat through its Gram matrix
    nff = len(ff)
    fv_nonzeros, fv_zeros = list(range(nff)), []
    if nff:
        if fdev.n_clusters and N:
            Q = rv.free_gram()
        else:
            Q = np.zeros((D, N * N))
        if on_device and (nrem or nf):
            Qp = np.transpose(np.asarray(Q).reshape(D, N, N), (0, 2, 1))
            rows = [Bc_planes(j, np.sort(removed[j]))[:, :, :N] for j in range(J) if len(removed[j]) and j in dev_clusters]
            if rows:                                # minus the removed rows' outer products, all clusters stacked: one product
                Br = np.concatenate(rows, axis=1)
                Qp = rv.gemm_batch([(Br, Br, Qp, 1, 0, -1, 1)])[0]
            # changemat^T Q changemat as two products; changemat is written as planes: unit rows for ff, the negated planes of Rref for nf
            T = np.zeros((D, N, nff))
            T[0, ff, np.arange(nff)] = 1.0
            if nf:
                T[:, nf, :] = -Rref_pl
            QT = rv.gemm_batch([(Qp, T, None, 0, 0, 1, 0)])[0]
            Gf = rv.gemm_batch([(T, QT, None, 1, 0, 1, 0)])[0]
            # T^T (Q T) is symmetric only up to the rounding of D limbs: the lower triangle is mirrored, as the host path builds it, so that the pivoting
            # cannot depend on which triangle an elimination reads
            Gf = np.stack([np.tril(P) + np.tril(P, -1).T for P in Gf])
            Gl = np.transpose(Gf, (0, 2, 1)).reshape(D, -1)
        elif nrem or nf:
            Qm = _mp_sum(Q).reshape(N, N, order="F") if np.any(Q != 0.0) else np.full((N, N), mp.mpf(0), dtype=object)
            for j in range(J):                      # minus the removed rows' outer products (clusters the device saw only)
                if not len(removed[j]) or j not in dev_clusters:
                    continue
                Br = B_rows(j, np.sort(removed[j]))
                for a in range(N):
                    for b in range(N):
                        Qm[a, b] = Qm[a, b] - _dot(Br[:, a], Br[:, b])
            # changemat^T Q changemat with changemat = [e_a for ff_a ; -Rref for nf]
            Gf = np.empty((nff, nff), dtype=object)
            for a in range(nff):
                for b in range(a + 1):
                    v = Qm[ff[a], ff[b]]
                    if nf:
                        v = v - _dot(Rref[:, a], [Qm[k, ff[b]] for k in nf]) - _dot([Qm[ff[a], k] for k in nf], Rref[:, b])
                        v = v + _dot(Rref[:, a], [_dot([Qm[k, k2] for k2 in nf], Rref[:, b]) for k in nf])
                    Gf[a, b] = Gf[b, a] = v
            Gl = _split(Gf.reshape(-1, order="F"), D)
        else:
            Gl = Q
        tau3 = threshold(prec, D, np.max(Gl[0].reshape(nff, nff).diagonal()))
        perm, r, _W, _res = rv.rank_reveal(Gl, nff, nff, tau3)
        fv_nonzeros = sorted(int(v) for v in perm[:r])
        fv_zeros = sorted(int(v) for v in perm[r:])
    var_rels = VarRels((fv_zeros, fv_nonzeros, Rref, rhs, nf, ff))
    work = dict(D=D, kept=[np.sort(k) for k in kept], B_rows=B_rows, c_rows=c_rows)
    if on_device:
        work.update(Bc_planes=Bc_planes, Rref_pl=Rref_pl, rhs_pl=rhs_pl, gemm_batch=rv.gemm_batch)
    return cs, var_rels, work


def preprocess(sdp, prec: int = 256, reveal=None, device: int = 0, substitute: str = "host"):
    """The reference's `preprocess!` on a FlatSDP: returns (reduced FlatSDP, cs, var_rels); the input object itself when nothing was found.
    The substitution (remove_lindep_freevars!, :215-235) runs in mpmath at 52 D bits; its results keep D limb planes (hi, lo, `tails`), so
    that a solve with data_limbs = limbs sees them unrounded.  `reduced.constant` is the fp64 rounding of `var_rels.constant`.
    `substitute` = "device": the reduced B and c are one batch of multi-word products over the clusters, [B | c]_kept [changemat(:, kept columns) | -rhs],
    on the planes `rank_reveal` returned (`find_linear_dependencies`); b and the constant stay in mpmath."""
    mp = _mp()
    flat = sdp if isinstance(sdp, FlatSDP) else flatten(sdp)
    cs, vr, work = find_linear_dependencies(flat, prec=prec, reveal=reveal, device=device, substitute=substitute)
    fv_zeros, fv_nonzeros, Rref, rhs, nf, ff = vr
    D, kept = work["D"], work["kept"]
    with mp.workprec(52 * D):
        vr.constant = mp.mpf(flat.constant)
        if not cs and not nf and not fv_zeros:
            return flat, cs, vr
        if not nf and not fv_zeros:
            return select_constraints(flat, kept), cs, vr
        J, N = flat.n_clusters, flat.n_free
        cols = [ff[a] for a in fv_nonzeros]
        npl = _n_planes(flat)
        b = _mp_sum(flat.data_planes_of("b", npl))
        B_pl, c_pl = [], []
        if substitute == "device":
            nnz, nn = len(cols), len(nf)
            S = np.zeros((D, N + 1, nnz + 1))           # [changemat(:, kept columns) | -rhs] over a last row (0 .. 0 1) that carries c
            S[0, cols, np.arange(nnz)] = 1.0
            S[0, N, nnz] = 1.0
            if nn:
                S[:, nf, :nnz] = -work["Rref_pl"][:, :, fv_nonzeros]
                S[:, nf, nnz] = -work["rhs_pl"]
            jobs = [(work["Bc_planes"](j, kept[j]), S, None, 0, 0, 1, 0) for j in range(J) if len(kept[j])]
            done = iter(work["gemm_batch"](jobs) if jobs else [])
            for j in range(J):
                R = next(done) if len(kept[j]) else np.zeros((D, 0, nnz + 1))
                B_pl.append(np.ascontiguousarray(R[:, :, :nnz]))
                c_pl.append(np.ascontiguousarray(R[:, :, nnz]))
        else:
            for j in range(J):
                rows = kept[j]
                Bk = work["B_rows"](j, rows) if len(rows) else np.empty((0, N), dtype=object)
                ck = work["c_rows"](j, rows) if len(rows) else np.empty(0, dtype=object)
                Bn, cn = np.empty((len(rows), len(cols)), dtype=object), np.empty(len(rows), dtype=object)
                for i in range(len(rows)):
                    Bnf = [Bk[i, k] for k in nf]
                    for a, pos in enumerate(fv_nonzeros):
                        Bn[i, a] = Bk[i, cols[a]] - (_dot(Bnf, Rref[:, pos]) if nf else 0)
                    cn[i] = ck[i] - (_dot(Bnf, rhs) if nf else 0)
                B_pl.append(_split(Bn, max(D, 2)))
                c_pl.append(_split(cn, max(D, 2)))
        bnf = [b[k] for k in nf]
        bn = np.array([b[cols[a]] - (_dot(bnf, Rref[:, pos]) if nf else 0) for a, pos in enumerate(fv_nonzeros)], dtype=object)
        vr.constant = mp.mpf(flat.constant) + (_dot(bnf, rhs) if nf else 0)
        red = select_constraints(flat, kept, B_planes=B_pl, c_planes=c_pl, b_planes=_split(bn, max(D, 2)).reshape(max(D, 2), -1), constant=float(vr.constant))
    return red, cs, vr


def postprocess(x, y, cs, var_rels):
    """The reference's `postprocess` (:312-325): x with a zero for every removed constraint, y with the eliminated variables put back
    (`add_dependent_freevars`, :258-276: y_nf = rhs_changed - Rref y_ff).  x, y: fp64 vectors, or planar limbs (limbs, len)."""
    mp = _mp()
    fv_zeros, fv_nonzeros, Rref, rhs, nf, ff = var_rels
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    planar = x.ndim == 2
    x2 = np.atleast_2d(x)
    removed = sorted(c[0] for c in cs)
    full = np.zeros((x2.shape[0], x2.shape[1] + len(removed)))
    mask = np.ones(full.shape[1], dtype=bool)
    mask[removed] = False
    full[:, mask] = x2
    y2 = np.atleast_2d(y) if y.size else np.zeros((x2.shape[0], 0))
    K = y2.shape[0]
    if y2.shape[1] != len(fv_nonzeros):
        raise ValueError(f"postprocess: expected {len(fv_nonzeros)} free variables, got {y2.shape[1]}")
    N = len(nf) + len(ff)
    with mp.workprec(64 * K + 128):
        yff = [mp.mpf(0)] * len(ff)
        ym = _mp_sum(y2) if y2.size else []
        for a, pos in enumerate(fv_nonzeros):
            yff[pos] = ym[a]
        yo = [mp.mpf(0)] * N
        for pos, v in enumerate(ff):
            yo[v] = yff[pos]
        for a, v in enumerate(nf):
            yo[v] = rhs[a] - _dot(Rref[a, :], yff)
        yfull = _split(np.array(yo, dtype=object), K) if N else np.zeros((K, 0))
    if not planar:
        return full[0], (yfull[0] if y.ndim <= 1 else yfull)
    return full, yfull

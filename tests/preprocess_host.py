"""Host (mpmath) stand-ins for the device primitives of clrs_amd.preprocess, for the CPU tests, and the reference elimination the
kernel k_mw_rank_reveal is compared against: a diagonally pivoted Cholesky with the kernel's pivot rule (largest remaining diagonal
among the candidates, ties to the smallest original index, stop at pivots <= tau) whose relations W = G11^-1 G12 come from the same
elimination applied to the rows of a unit matrix."""
import mpmath as mp
import numpy as np

from clrs_amd.mw import to_limbs


def limbs_to_mp(planes):
    planes = np.atleast_2d(np.asarray(planes, dtype=np.float64))
    return [mp.fsum(mp.mpf(float(planes[l, i])) for l in range(planes.shape[0])) for i in range(planes.shape[1])]


def pivoted_cholesky(G, ncand=None, tau=0, bits=320, order=None):
    """G: n x n list of lists / object array of mpmath numbers.  Returns (perm, r, W, resid, pivots): perm = pivots in pivot order then the
    rest in original order, W[c][a] (r x (n - r)) the coefficient of pivot c in non-pivot a, resid the remaining diagonal of the
    non-pivots, pivots the accepted pivot values.  `order`: take these pivots in this order instead of choosing (and do not stop)."""
    n = len(G)
    ncand = n if ncand is None else ncand
    with mp.workprec(bits):
        A = [[+mp.mpf(G[i][j]) for j in range(n)] for i in range(n)]
        U = [[mp.mpf(0)] * n for _ in range(n)]          # unit part: U[i][c] = coefficient of pivot number c in row i
        piv, rest, pivots = [], list(range(n)), []
        while True:
            if order is not None:
                if len(piv) == len(order):
                    break
                p = order[len(piv)]
            else:
                cand = [i for i in rest if i < ncand]
                if not cand:
                    break
                p = max(cand, key=lambda i: (A[i][i], -i))
                if not A[p][p] > tau:
                    break
            k = len(piv)
            d = A[p][p]
            pivots.append(d)
            rest.remove(p)
            for i in rest:
                f = A[i][p] / d
                for c in rest:
                    if c <= i:
                        A[i][c] = A[c][i] = A[i][c] - f * A[c][p]
                for c in range(k):
                    U[i][c] = U[i][c] - f * U[p][c]
                U[i][k] = -f
            piv.append(p)
        r = len(piv)
        W = [[-U[i][c] for i in rest] for c in range(r)]
        resid = [A[i][i] for i in rest]
    return piv + rest, r, W, resid, pivots


def relation_residual(G, perm, r, W, bits):
    """max |G12 - G11 W| / max G_ii at `bits` bits, from the input G"""
    n = len(G)
    with mp.workprec(bits):
        piv, rest = perm[:r], perm[r:]
        worst = mp.mpf(0)
        for a, i in enumerate(rest):
            for c in piv:
                v = mp.mpf(G[c][i]) - mp.fsum(mp.mpf(G[c][piv[k]]) * W[k][a] for k in range(r))
                worst = max(worst, abs(v))
        scale = max(mp.mpf(G[i][i]) for i in range(n))
        return worst / scale if scale else worst


def constraint_matrices(flat, j):
    """[{block: n x n object matrix (symmetrised)}] for every constraint of cluster j, from all limb planes of the data"""
    npl = 2 + max([t.shape[0] for t in (flat.tails or {}).values()] + [0])
    lam, vs, ws, dA = (flat.data_planes_of(nm, npl) for nm in ("term_lambda", "term_vs", "term_ws", "dense_A"))
    out = [dict() for _ in range(int(flat.cluster_P[j]))]
    for b in range(flat.n_blocks):
        if int(flat.block_cluster[b]) != j:
            continue
        n, dl = int(flat.block_n[b]), int(flat.block_delta[b])

        def mat(p):
            return out[p].setdefault(b, [[mp.mpf(0)] * n for _ in range(n)])
        for t in range(int(flat.term_ptr[b]), int(flat.term_ptr[b + 1])):
            M = mat(int(flat.term_p[t]))
            v0 = int(flat.term_vec_ptr[t])
            l = limbs_to_mp(lam[:, t:t + 1])[0]
            v, w = limbs_to_mp(vs[:, v0:v0 + dl]), limbs_to_mp(ws[:, v0:v0 + dl])
            r0, s0 = int(flat.term_r[t]) * dl, int(flat.term_s[t]) * dl
            for a in range(dl):
                for c in range(dl):
                    M[r0 + a][s0 + c] += l * v[a] * w[c]
        for e in range(int(flat.dense_ptr[b]), int(flat.dense_ptr[b + 1])):
            M = mat(int(flat.dense_p[e]))
            a0 = int(flat.dense_A_ptr[e])
            A = limbs_to_mp(dA[:, a0:a0 + n * n])
            for a in range(n):
                for c in range(n):
                    M[a][c] += A[a + c * n]
    for d in out:
        for b, M in d.items():
            n = len(M)
            d[b] = [[(M[a][c] + M[c][a]) / 2 for c in range(n)] for a in range(n)]
    return out


class HostReveal:
    """The interface of clrs_amd.preprocess.DeviceReveal in mpmath at 52 D bits (tiny problems only)."""

    def __init__(self, flat, D):
        self.flat, self.D, self.bits = flat, D, 52 * D
        self._G = None

    def _grams(self):
        if self._G is None:
            f = self.flat
            self._G = []
            with mp.workprec(self.bits):
                for j in range(f.n_clusters):
                    A = constraint_matrices(f, j)
                    P = len(A)
                    G = [[mp.mpf(0)] * P for _ in range(P)]
                    for p in range(P):
                        for q in range(p + 1):
                            s = mp.mpf(0)
                            for b, M in A[p].items():
                                if b in A[q]:
                                    s += mp.fsum(M[a][c] * A[q][b][a][c] for a in range(len(M)) for c in range(len(M)))
                            G[p][q] = G[q][p] = s
                    self._G.append(G)
        return self._G

    def gram_diag(self):
        return [np.array([float(G[p][p]) for p in range(len(G))]) for G in self._grams()]

    def _pack(self, perm, r, W, resid):
        n = len(perm)
        Wl = to_limbs([W[c][a] for a in range(n - r) for c in range(r)], self.D) if r * (n - r) else np.zeros((self.D, 0))
        return np.array(perm, dtype=np.int32), r, Wl, (to_limbs(resid, self.D) if n - r else np.zeros((self.D, 0)))

    def dependencies(self, tau):
        return [self._pack(*pivoted_cholesky(G, None, tau[j], self.bits)[:4]) for j, G in enumerate(self._grams())]

    def free_gram(self):
        f = self.flat
        N, X = f.n_free, f.x_len
        npl = 2 + max([t.shape[0] for t in (f.tails or {}).values()] + [0])
        Bp = f.data_planes_of("B", npl)
        with mp.workprec(self.bits):
            cols = [[] for _ in range(N)]
            for j in range(f.n_clusters):
                o, P = int(f.cluster_off[j]), int(f.cluster_P[j])
                for a in range(N):
                    cols[a] += limbs_to_mp(Bp[:, o * N + a * P:o * N + (a + 1) * P])
            Q = [mp.fsum(x * y for x, y in zip(cols[a], cols[b])) for b in range(N) for a in range(N)]
        return to_limbs(Q, self.D) if N else np.zeros((self.D, 0))

    def rank_reveal(self, G, n, ncand, tau):
        with mp.workprec(64 * self.D + 128):
            g = limbs_to_mp(G)
        M = [[g[i + j * n] for j in range(n)] for i in range(n)]
        return self._pack(*pivoted_cholesky(M, ncand, tau, self.bits)[:4])

    def close(self):
        pass


# ---- planted dependencies in a real instance ----------------------------------------------------------------------------------------

def _planes_of(h, planes):
    return np.stack([np.asarray(h.plane(t), dtype=np.float64) for t in range(planes)])


def _hilo(pl):
    from clrs_amd.sdp import HiLo
    return HiLo(pl[0].copy(), pl[1].copy() if np.any(pl[1] != 0.0) else None, [p.copy() for p in pl[2:]] if pl.shape[0] > 2 and np.any(pl[2:] != 0.0) else None)


def _combine(rows, coeffs, planes):
    """sum_i coeffs[i] * rows[i] (each row: planar (k, ...) limbs), formed exactly in mpmath and split into `planes` limb planes"""
    shape = rows[0].shape[1:]
    out = np.zeros((planes,) + shape)
    with mp.workprec(2200):
        for idx in np.ndindex(*shape):
            v = mp.fsum(mp.mpf(c) * mp.mpf(float(r[(l,) + idx])) for r, c in zip(rows, coeffs) for l in range(r.shape[0]) if r[(l,) + idx] != 0.0)
            for l in range(planes):
                h = float(v)
                out[(l,) + idx] = h
                if h == 0.0:
                    break
                v = v - mp.mpf(h)
    return out


def plant_dependencies(sdp, plants, duplicate_free_column=True, planes=6):
    """A copy of the ClusteredLowRankSDP `sdp` with, per entry (j, {p: coeff}) of `plants`, one more constraint in cluster j that is the given
    combination of its constraints p (coefficients +-2^k: the low-rank terms are concatenated with scaled lambda -- exact in every limb plane --,
    dense matrices, the row of B and c are combined exactly in mpmath and carried in `planes` limb planes), and, first, one duplicated
    free-variable column (a copy of column 0, with the same objective coefficient).  The planted problem has the feasible set and optimum of
    `sdp`."""
    from clrs_amd.sdp import Block, ClusteredLowRankSDP, LowRankMat
    J = sdp.n_clusters
    Bs = [_planes_of(h, planes) for h in sdp.B]
    cs = [_planes_of(h, planes) for h in sdp.c]
    b = _planes_of(sdp.b, planes)
    if duplicate_free_column and sdp.n_free:
        Bs = [np.concatenate([B, B[:, :, :1]], axis=2) for B in Bs]
        b = np.concatenate([b, b[:, :1]], axis=1)
    blocks = [[Block(bl.m, bl.delta, {rs: dict(d) for rs, d in bl.entries.items()}, bl.name) for bl in cl] for cl in sdp.blocks]
    for j, comb in plants:
        ps, co = list(comb), [float(v) for v in comb.values()]
        assert all(abs(v) == 2.0 ** round(np.log2(abs(v))) for v in co), "coefficients must be +-2^k"
        P = Bs[j].shape[1]
        for bl in blocks[j]:
            for rs, d in bl.entries.items():
                have = [(p, c) for p, c in zip(ps, co) if p in d]
                if not have:
                    continue
                if isinstance(d[have[0][0]], LowRankMat):
                    lam = np.concatenate([c * _planes_of(d[p].lam, planes) for p, c in have], axis=1)
                    vs = np.concatenate([_planes_of(d[p].vs, planes) for p, c in have], axis=1)
                    ws = np.concatenate([_planes_of(d[p].ws, planes) for p, c in have], axis=1)
                    d[P] = LowRankMat(_hilo(lam), _hilo(vs), _hilo(ws))
                else:
                    d[P] = _hilo(_combine([_planes_of(d[p], planes) for p, c in have], [c for p, c in have], planes))
        Bs[j] = np.concatenate([Bs[j], _combine([Bs[j][:, p, :] for p in ps], co, planes)[:, None, :]], axis=1)
        cs[j] = np.concatenate([cs[j], _combine([cs[j][:, p] for p in ps], co, planes)[:, None]], axis=1)
    out = ClusteredLowRankSDP(sdp.maximize, sdp.constant, blocks, [_hilo(B) for B in Bs], [_hilo(c) for c in cs], sdp.C, _hilo(b), sdp.names)
    out.check()
    return out

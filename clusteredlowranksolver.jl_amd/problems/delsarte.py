"""Delsarte LP bound for spherical codes (reference examples/Delsarte.jl:7-49).

    minimise M  s.t.  sum_k a_k P_k^n(x) + <S1, b b^T> + (1+x)(cos t - x) <S2, b' b'^T> = -1   on samples
                      sum_k a_k + slack - M = -1,         a_k >= 0, slack >= 0
One cluster (all constraints share the a_k), P = 2d+2, N = 1; blocks: 2d dense 1x1 (a_k),
(d+1)x(d+1) and d x d rank-1 SOS blocks, one dense 1x1 slack.
"""
from __future__ import annotations

import numpy as np
import mpmath as mp

from ..sdp import Block, ClusteredLowRankSDP, HiLo, LowRankMat
from .polytools import (DEFAULT_PREC, approximate_fekete, chebyshev_values, gegenbauer_values,
                        sample_points_chebyshev)


def delsarte(n, d, costheta, prec=DEFAULT_PREC) -> ClusteredLowRankSDP:
    with mp.workprec(prec):
        ct = mp.mpf(costheta) if not isinstance(costheta, str) else mp.mpf(eval(costheta))
        xs = sample_points_chebyshev(2 * d, -1, ct)
        V, xs = approximate_fekete(chebyshev_values(2 * d, xs), xs)
        ns = len(xs)                      # 2d+1 samples
        P = ns + 1                        # + the scalar constraint
        G = gegenbauer_values(2 * d, n, xs)
        blocks, Cs = [], []
        one = np.ones((1, 1))
        for k in range(1, 2 * d + 1):     # a_k : dense 1x1, present in every constraint
            ent = {p: HiLo.of(np.array([[G[p, k]]], dtype=object)) for p in range(ns)}
            ent[ns] = HiLo.of(one)
            blocks.append(Block(m=1, delta=1, entries={(0, 0): ent}, name=("a", k)))
            Cs.append(np.zeros((1, 1)))
        e1 = {p: LowRankMat(np.array([1.0]), HiLo.of(V[p:p + 1, :d + 1]), HiLo.of(V[p:p + 1, :d + 1])) for p in range(ns)}
        blocks.append(Block(m=1, delta=d + 1, entries={(0, 0): e1}, name=("SOS", 1)))
        Cs.append(np.zeros((d + 1, d + 1)))
        e2 = {}
        for p in range(ns):
            lam = np.array([(1 + xs[p]) * (ct - xs[p])], dtype=object)
            e2[p] = LowRankMat(HiLo.of(lam), HiLo.of(V[p:p + 1, :d]), HiLo.of(V[p:p + 1, :d]))
        blocks.append(Block(m=1, delta=d, entries={(0, 0): e2}, name=("SOS", 2)))
        Cs.append(np.zeros((d, d)))
        blocks.append(Block(m=1, delta=1, entries={(0, 0): {ns: HiLo.of(one)}}, name="slack"))
        Cs.append(np.zeros((1, 1)))
        B = np.zeros((P, 1)); B[ns, 0] = -1.0
        c = -np.ones(P)
        return ClusteredLowRankSDP(maximize=False, constant=0.0, blocks=[blocks], B=[B], c=[c], C=[Cs],
                                   b=np.ones(1), names={"free": ["M"], "blocks": [[b.name for b in blocks]]})


def delsarte_exact(n, d, costheta, prec=DEFAULT_PREC) -> ClusteredLowRankSDP:
    """The Delsarte bound in the form whose optimal solution has a rational kernel (reference examples/DelsarteExact.jl:7-35), for the rounding step:

        minimise 1 + sum_{k=0}^{2d} a_k   s.t.  sum_k a_k P_k^n(x) + <A, b b^T> + (1+x)(cos t - x) <B, b' b'^T> = -1   on samples,   a_k >= 0

    with the plain Chebyshev basis b = (T_0 .. T_d), b' = (T_0 .. T_{d-1}) -- NO change of basis, so the kernel vectors of A and B are those of the
    polynomial problem, not of an approximately orthogonalised one -- and the 2d + 1 Chebyshev points of [-1, 1] rounded to four decimals (rational
    samples).  One cluster, P = 2d + 1, no free variables; blocks a_0 .. a_2d (dense 1 x 1), A ((d+1) x (d+1)) and B (d x d), rank one."""
    with mp.workprec(prec):
        ct = mp.mpf(costheta) if not isinstance(costheta, str) else mp.mpf(eval(costheta))
        xs = [mp.mpf(int(mp.nint(x * 10 ** 4))) / 10 ** 4 for x in sample_points_chebyshev(2 * d)]
        ns = len(xs)
        V = chebyshev_values(d, xs)
        G = gegenbauer_values(2 * d, n, xs)
        blocks, Cs = [], []
        for k in range(2 * d + 1):
            ent = {p: HiLo.of(np.array([[G[p, k]]], dtype=object)) for p in range(ns)}
            blocks.append(Block(m=1, delta=1, entries={(0, 0): ent}, name=("a", k)))
            Cs.append(np.ones((1, 1)))
        eA = {p: LowRankMat(np.array([1.0]), HiLo.of(V[p:p + 1, :d + 1]), HiLo.of(V[p:p + 1, :d + 1])) for p in range(ns)}
        blocks.append(Block(m=1, delta=d + 1, entries={(0, 0): eA}, name="A"))
        Cs.append(np.zeros((d + 1, d + 1)))
        eB = {}
        for p in range(ns):
            lam = np.array([(1 + xs[p]) * (ct - xs[p])], dtype=object)
            eB[p] = LowRankMat(HiLo.of(lam), HiLo.of(V[p:p + 1, :d]), HiLo.of(V[p:p + 1, :d]))
        blocks.append(Block(m=1, delta=d, entries={(0, 0): eB}, name="B"))
        Cs.append(np.zeros((d, d)))
        return ClusteredLowRankSDP(maximize=False, constant=1.0, blocks=[blocks], B=[np.zeros((ns, 0))], c=[-np.ones(ns)], C=[Cs],
                                   b=np.zeros(0), names={"free": [], "blocks": [[b.name for b in blocks]]})


def delsarte_exact_problem(n, d, costheta, field=None):
    """`delsarte_exact` over QQ, the problem `rounding.exact_solution` rounds to: the same four-decimal samples, the Chebyshev and Gegenbauer recurrences of
    polytools in `Fraction`s.  `delsarte_exact_problem(n, d, costheta).to_sdp(prec)` is `delsarte_exact(n, d, costheta, prec)`.
    With `field` (a `rounding.NumberField`) `costheta` is the tuple of its coefficients in g -- `(0, 1/5)` over x^2 - 5 for 1 / sqrt(5), `(1/4, 1/4)` for
    1 / (sqrt(5) - 1) -- and the weights of block "B" are field elements; every other number stays rational."""
    from fractions import Fraction as F
    from ..rounding import ExactBlock, ExactLowRank, ExactProblem, field_array
    if field is not None:
        ctf = tuple(F(c) for c in costheta)
        if len(ctf) != field.degree:
            raise ValueError(f"delsarte_exact_problem: costheta needs {field.degree} coefficients")
        weight = lambda x: field_array([tuple((1 + x) * (c - (x if k == 0 else 0)) for k, c in enumerate(ctf))])
    else:
        ct = F(costheta)
        weight = lambda x: [(1 + x) * (ct - x)]
    with mp.workprec(DEFAULT_PREC):
        xs = [F(int(mp.nint(x * 10 ** 4)), 10 ** 4) for x in sample_points_chebyshev(2 * d)]
    ns = len(xs)

    def recurrence(deg, step):
        V = np.empty((ns, deg + 1), dtype=object)
        for i, x in enumerate(xs):
            V[i, 0] = F(1)
            if deg >= 1:
                V[i, 1] = x
            for l in range(2, deg + 1):
                V[i, l] = step(l, x, V[i, l - 1], V[i, l - 2])
        return V
    V = recurrence(d, lambda l, x, v1, v2: 2 * x * v1 - v2)
    G = recurrence(2 * d, lambda l, x, v1, v2: F(2 * l + n - 4, l + n - 3) * x * v1 - F(l - 1, l + n - 3) * v2)
    blocks, Cs = [], []
    for k in range(2 * d + 1):
        blocks.append(ExactBlock(1, 1, {(0, 0): {p: np.array([[G[p, k]]], dtype=object) for p in range(ns)}}, ("a", k)))
        Cs.append(np.array([[F(1)]], dtype=object))
    blocks.append(ExactBlock(1, d + 1, {(0, 0): {p: ExactLowRank([F(1)], V[p:p + 1, :d + 1], V[p:p + 1, :d + 1]) for p in range(ns)}}, "A"))
    Cs.append(np.full((d + 1, d + 1), F(0), dtype=object))
    blocks.append(ExactBlock(1, d, {(0, 0): {p: ExactLowRank(weight(xs[p]), V[p:p + 1, :d], V[p:p + 1, :d]) for p in range(ns)}}, "B"))
    Cs.append(np.full((d, d), F(0), dtype=object))
    return ExactProblem(False, F(1), [blocks], [np.zeros((ns, 0), dtype=object)], [np.full(ns, F(-1), dtype=object)], [Cs], np.zeros(0, dtype=object),
                        {"free": [], "blocks": [[b.name for b in blocks]]}, field)

"""Shared by tests/test_field_system_cpu.py and tests/test_field_system_gpu.py: small systems over number fields in tuple arithmetic, a planted system for
`field_least_squares`, the reference's method (the primal normal equations solved in mpmath at 1000 bits) and a host stand-in for `mw.gemm_batch`."""
from fractions import Fraction

import mpmath as mp
import numpy as np

from clrs_amd import rounding
from clrs_amd.mw import from_limbs, to_limbs

SQRT5 = [-5, 0, 1]           # x^2 - 5
CBRT2 = [-2, 0, 0, 1]        # x^3 - 2


_FIELDS = {}


def field_of(minpoly, prec=700):
    with mp.workprec(prec):
        g = mp.sqrt(5) if minpoly == SQRT5 else mp.cbrt(2)
        return _FIELDS.setdefault((tuple(minpoly), prec), rounding.NumberField(minpoly, g, prec=prec))           # (inside: the constructor takes g at the current precision)


def random_tuples(rng, shape, d, den=4, zero=0.3):
    """an object array of tuples of d small `Fraction`s, a share `zero` of the coefficients 0"""
    out = np.empty(shape, dtype=object)
    for idx in np.ndindex(*shape):
        out[idx] = tuple(Fraction(0) if rng.random() < zero else Fraction(int(rng.integers(-9, 10)), int(rng.integers(1, den + 1))) for _ in range(d))
    return out


def mul(x, y, minpoly):
    d = len(minpoly) - 1
    t = [Fraction(0)] * (2 * d - 1)
    for a in range(d):
        for b in range(d):
            t[a + b] += x[a] * y[b]
    return rounding._field_fold(t, minpoly)


def matvec(A, x, minpoly):
    """A x over the field, entry by entry in tuple arithmetic"""
    d = len(minpoly) - 1
    out = []
    for r in range(A.shape[0]):
        s = [Fraction(0)] * d
        for c in range(A.shape[1]):
            s = [u + v for u, v in zip(s, mul(A[r, c], x[c], minpoly))]
        out.append(tuple(s))
    return out


def planted_system(seed=0, n=4, m=6, minpoly=SQRT5):
    """(A, b, xstar): A (n, m) and xstar (m,) of small tuples, b = A xstar"""
    rng = np.random.default_rng(seed)
    d = len(minpoly) - 1
    A = random_tuples(rng, (n, m), d)
    xstar = list(random_tuples(rng, (m,), d, den=3, zero=0.0))
    return A, matvec(A, xstar, minpoly), xstar


def embed(elems, field, prec=700):
    with mp.workprec(prec):
        gp = field.power_values(prec=prec)
        return [mp.fsum(mp.mpf(c.numerator) / c.denominator * g for c, g in zip(e, gp)) for e in elems]


def residual(Atot, btot, xr):
    """max_i |btot - Atot xr|_i, exact"""
    return max(abs(btot[i] - sum((Atot[i, c] * xr[c] for c in range(Atot.shape[1]) if Atot[i, c]), Fraction(0))) for i in range(Atot.shape[0]))


def reference_least_squares(Atot, btot, x, field, regularization=1e-30, decimals=40, prec=1000):
    """the reference's roundx(A, b, x, g, deg) (src/rounding.jl:537-568) in mpmath at `prec` bits: the primal normal equations by LU"""
    d, m, rows = field.degree, len(x), Atot.shape[0]
    with mp.workprec(prec):
        g = field.g
        num = lambda v: mp.mpf(v.numerator) / v.denominator if isinstance(v, Fraction) else mp.mpf(v)
        A = mp.matrix(rows, m * d)
        for r in range(rows):
            for c in range(m * d):
                A[r, c] = num(Atot[r, c])
        xs = mp.matrix([num(v) for v in x])
        rhs = mp.matrix([num(v) for v in btot]) - A[:, 0:m] * xs
        B = mp.matrix(rows, m * (d - 1))
        for j in range(1, d):
            B[:, m * (j - 1):m * j] = A[:, m * j:m * (j + 1)] - g ** j * A[:, 0:m]
        lhs = B.T * B + mp.mpf(regularization) * mp.eye(m * (d - 1))
        y = mp.lu_solve(lhs, B.T * rhs)
        x0 = [xs[c] - mp.fsum(g ** j * y[m * (j - 1) + c] for j in range(1, d)) for c in range(m)]
        scale = 10 ** decimals
        return [Fraction(int(mp.floor(v * scale)), scale) for v in x0 + list(y)]


def host_gemm(jobs, limbs, device=0):
    """`gemm=` in mpmath at 64 limbs + 128 bits, rounded to limbs: op(A) op(B) with alpha = 1, beta = 0, either operand transposed"""
    out = []
    with mp.workprec(64 * limbs + 128):
        for A, B, Cm, ta, tb, alpha, beta in jobs:
            assert alpha == 1 and beta == 0 and Cm is None
            a = np.array([from_limbs(A[:, i, :]) for i in range(A.shape[1])], dtype=object).reshape(A.shape[1], A.shape[2])
            b = np.array([from_limbs(B[:, i, :]) for i in range(B.shape[1])], dtype=object).reshape(B.shape[1], B.shape[2])
            c = (a.T if ta else a).dot(b.T if tb else b)
            out.append(to_limbs(c, limbs).reshape(limbs, c.shape[0], c.shape[1]))
    return out


# ---- a hand-made problem over QQ(sqrt 5): the structure of lrsys_util.handmade_problem with field entries in lam, the dense block, B and c -----------------------------
ZERO2, ONE2 = (Fraction(0), Fraction(0)), (Fraction(1), Fraction(0))


def handmade_field_problem(minpoly=SQRT5):
    rng = np.random.default_rng(77)
    d = len(minpoly) - 1
    fr = lambda shape: np.array([Fraction(int(a), int(b)) for a, b in zip(rng.integers(-9, 10, size=int(np.prod(shape))), rng.integers(1, 7, size=int(np.prod(shape))))],
                                dtype=object).reshape(shape)
    ft = lambda shape: random_tuples(rng, shape, d, den=5, zero=0.2)
    delta, P0, P1, N = 2, 3, 2, 2

    def sym_rank2():
        lam, v, w = ft((1,))[0], fr((delta,)), fr((delta,))
        return rounding.ExactLowRank(rounding.field_array([lam, lam]), [v, w], [w, v])

    def lowrank_entries(P):
        ent = {(0, 0): {}, (0, 1): {}, (1, 0): {}, (1, 1): {}}
        for p in range(P):
            ent[(0, 0)][p], ent[(1, 1)][p] = sym_rank2(), sym_rank2()
            off = rounding.ExactLowRank(ft((2,)), fr((2, delta)), fr((2, delta)))
            ent[(0, 1)][p] = off
            ent[(1, 0)][p] = rounding.ExactLowRank(off.lam, off.ws, off.vs)
        return ent

    def symm(n):
        M = ft((n, n))
        out = np.empty((n, n), dtype=object)
        for i in range(n):
            for j in range(n):
                out[i, j] = tuple(u + v for u, v in zip(M[i, j], M[j, i]))
        return out
    lr0 = rounding.ExactBlock(2, delta, lowrank_entries(P0), "L0")
    dn0 = rounding.ExactBlock(1, 3, {(0, 0): {p: symm(3) for p in range(P0)}}, "D0")
    lr1 = rounding.ExactBlock(2, delta, lowrank_entries(P1), "L1")
    return rounding.ExactProblem(True, Fraction(1, 3), [[lr0, dn0], [lr1]], [ft((P0, N)), ft((P1, N))], [ft((P0,)), ft((P1,))], [[symm(4), symm(3)], [symm(4)]],
                                 ft((N,)), field=field_of(minpoly))


def handmade_field_Bs(minpoly=SQRT5):
    """(B^T, Binv, s) over the field: unit lower triangular B with field entries below the diagonal, inverted by substitution; block 0 loses one dimension"""
    d = len(minpoly) - 1
    one, zero = (Fraction(1),) + (Fraction(0),) * (d - 1), (Fraction(0),) * d
    rng = np.random.default_rng(5)
    out = {}
    for key, (n, s) in {0: (4, 1), 1: (3, 0)}.items():
        low = random_tuples(rng, (n, n), d, den=3, zero=0.3)
        B = np.empty((n, n), dtype=object)
        for i in range(n):
            for j in range(n):
                B[i, j] = one if i == j else (low[i, j] if i > j else zero)
        Binv = np.empty((n, n), dtype=object)                 # column by column: Binv[i, j] = [i == j] - sum_{j <= k < i} B[i, k] Binv[k, j]
        for j in range(n):
            for i in range(n):
                acc = list(one if i == j else zero)
                for k in range(j, i):
                    acc = [u - v for u, v in zip(acc, mul(B[i, k], Binv[k, j], minpoly))]
                Binv[i, j] = tuple(acc) if i >= j else zero
        out[key] = (B.T.copy(), Binv, s)
    return out


def _el(v, d):
    return tuple(v) if isinstance(v, tuple) else (Fraction(v),) + (Fraction(0),) * (d - 1)


def dense_field_constraint(bl, p, minpoly):
    d = len(minpoly) - 1
    n, dl = bl.n, bl.delta
    M = np.empty((n, n), dtype=object)
    M.fill((Fraction(0),) * d)
    for (r, s), ent in bl.entries.items():
        e = ent.get(p)
        if e is None:
            continue
        if isinstance(e, rounding.ExactLowRank):
            for k in range(e.rank):
                for i in range(dl):
                    for j in range(dl):
                        t = mul(mul(_el(e.lam[k], d), _el(e.vs[k][i], d), minpoly), _el(e.ws[k][j], d), minpoly)
                        M[r * dl + i, s * dl + j] = tuple(u + v for u, v in zip(M[r * dl + i, s * dl + j], t))
        else:
            for i in range(n):
                for j in range(n):
                    M[i, j] = tuple(u + v for u, v in zip(M[i, j], _el(e[i][j], d)))
    return M


def restated_field_system(problem, Bs=None, minpoly=SQRT5):
    """(A rows, b, index) by triple loops in tuple arithmetic: P M P^T entry by entry, the factor 2 off the diagonal"""
    d = len(minpoly) - 1
    one, zero = (Fraction(1),) + (Fraction(0),) * (d - 1), (Fraction(0),) * d
    rows, index, kept = [], [], []
    for bi, (j, bl) in enumerate(problem.flat_blocks()):
        if Bs is not None and bi in Bs:
            Binv, s = Bs[bi][1], Bs[bi][2]
            kept.append([[Binv[r, c] for c in range(bl.n)] for r in range(s, bl.n)])
        else:
            kept.append([[one if r == c else zero for c in range(bl.n)] for r in range(bl.n)])
        index += [(bi, a, b) for a in range(len(kept[-1])) for b in range(a, len(kept[-1]))]
    index += [("free", k) for k in range(problem.b.size)]
    for j, cl in enumerate(problem.blocks):
        for p in range(len(problem.c[j])):
            row = []
            for bi, (jj, bl) in enumerate(problem.flat_blocks()):
                P, n = kept[bi], bl.n
                M = dense_field_constraint(bl, p, minpoly) if jj == j else None
                for a in range(len(P)):
                    for b in range(a, len(P)):
                        v = list(zero)
                        if M is not None:
                            for x in range(n):
                                for y in range(n):
                                    if any(P[a][x]) and any(M[x, y]) and any(P[b][y]):
                                        v = [u + w for u, w in zip(v, mul(mul(P[a][x], M[x, y], minpoly), P[b][y], minpoly))]
                        row.append(tuple(v) if a == b else tuple(2 * u for u in v))
            row += [_el(problem.B[j][p, k], d) for k in range(problem.b.size)]
            rows.append(row)
    return rows, [_el(v, d) for cj in problem.c for v in cj], index


# ---- the Delsarte problems over QQ(sqrt 5) and the host stand-ins of every device call of exact_solution(field=...) ---------------------------------------------------
COSTHETA = {"icosahedron": (0, Fraction(1, 5)), "600-cell": (Fraction(1, 4), Fraction(1, 4))}       # 1 / sqrt(5) = sqrt(5) / 5;  1 / (sqrt(5) - 1) = (1 + sqrt(5)) / 4


def delsarte_field_problem(name, prec=700):
    from clrs_amd import problems
    from tests import field_round_util as fru
    n, d = fru.DELSARTE[name][:2]
    return problems.delsarte_exact_problem(n, d, COSTHETA[name], field=field_of(SQRT5, prec))


def host_hooks():
    from tests import field_inverse_util as fiu, field_round_util as fru, kernel_vectors_util as ku, lrsys_util as lu, pd_field_util as pfu, posv_util as pu
    hooks = dict(lu.host_hooks())
    hooks.update(fiu.host_hooks())
    hooks.update(round_batch=fru.host_field_batch(ku.host_batch), minors=pfu.host_field_minors, gemm=host_gemm,
                 solve=lambda A, B, limbs, device=0: pu.host_solve(A, B, limbs))
    return hooks

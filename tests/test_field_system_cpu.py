"""CPU side of the system over a number field QQ(g): `convert_system` and `xrational_to_field` exactly in tuple arithmetic, and `field_least_squares` on a
planted system with every device call through a host stand-in (the product in mpmath, the solve by the host restatement of clrs_mw_posv) against the
reference's method, the primal normal equations solved in mpmath at 1000 bits."""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from clrs_amd import rounding
from tests import field_system_util as fu
from tests import posv_util as pu


def _host_solve(A, B, limbs, device=0):
    return pu.host_solve(A, B, limbs)


@pytest.mark.parametrize("minpoly", (fu.SQRT5, fu.CBRT2, [1, -3, 0, 2]), ids=("x^2-5", "x^3-2", "2x^3-3x+1"))
def test_convert_system_is_the_field_product_coefficient_by_coefficient(minpoly):
    """(Atot [x_0; ..; x_(d-1)])[n k + i] is the coefficient of g^k of (A x)[i], exactly; a minimal polynomial that is not monic too"""
    d = len(minpoly) - 1
    rng = np.random.default_rng(d)
    n, m = 3, 5
    A, x = fu.random_tuples(rng, (n, m), d), list(fu.random_tuples(rng, (m,), d, zero=0.1))
    b = fu.matvec(A, x, minpoly)
    Atot, btot = rounding.convert_system(A, b, minpoly)
    assert Atot.shape == (n * d, m * d) and len(btot) == n * d and all(isinstance(v, Fraction) for v in Atot.flat)
    xcat = [x[c][j] for j in range(d) for c in range(m)]
    prod = [sum((Atot[r, c] * xcat[c] for c in range(m * d)), Fraction(0)) for r in range(n * d)]
    assert prod == btot == [b[i][k] for k in range(d) for i in range(n)]
    assert rounding.xrational_to_field(xcat, minpoly) == x
    with pytest.raises(ValueError, match="convert_system: b has"):
        rounding.convert_system(A, b[:-1], minpoly)
    with pytest.raises(ValueError, match="no multiple of the degree"):
        rounding.xrational_to_field(xcat[:-1], minpoly)


@pytest.mark.parametrize("minpoly,n,m", ((fu.SQRT5, 4, 6), (fu.SQRT5, 7, 5), (fu.CBRT2, 3, 4)), ids=("sqrt5-wide", "sqrt5-tall", "cbrt2"))
def test_field_least_squares_on_a_planted_system(minpoly, n, m):
    """x* with small numerators and denominators, b = A x*, the numeric x off by 1e-45: r = max |btot - Atot x_rounded| of both forms (host solve) against
    r_ref of the reference's method; r <= 4 r_ref + ||Atot||_inf 10^-decimals"""
    limbs, dec = 5, 40
    field = fu.field_of(minpoly)
    A, b, xstar = fu.planted_system(seed=n + m, n=n, m=m, minpoly=minpoly)
    Atot, btot = rounding.convert_system(A, b, field)
    with mp.workprec(700):
        x = [v + mp.mpf(10) ** -45 * (1 + c) for c, v in enumerate(fu.embed(xstar, field))]
    r_ref = fu.residual(Atot, btot, fu.reference_least_squares(Atot, btot, x, field, decimals=dec))
    norm = max(sum((abs(v) for v in Atot[i]), Fraction(0)) for i in range(Atot.shape[0]))
    seen = {}
    for form in ("primal", "dual", "auto"):
        xr = rounding.field_least_squares(Atot, btot, x, field, limbs, 1e-30, dec, form=form, gemm=fu.host_gemm, solve=_host_solve)
        assert len(xr) == m * field.degree and all(isinstance(v, Fraction) and (v * 10 ** dec).denominator == 1 for v in xr)
        r = fu.residual(Atot, btot, xr)
        seen[form] = xr
        print(form, "r", float(r), "r_ref", float(r_ref), "allowed", float(4 * r_ref + norm * Fraction(1, 10 ** dec)))
        assert r <= 4 * r_ref + norm * Fraction(1, 10 ** dec)
        back = fu.embed(rounding.xrational_to_field(xr, field), field)
        assert max(abs(u - v) for u, v in zip(back, x)) < 1e-38              # the rounded coefficients still embed to the numeric solution
    assert seen["auto"] == seen["primal" if m * (field.degree - 1) <= n * field.degree else "dual"]


def test_field_least_squares_refuses_what_it_cannot_take():
    field = fu.field_of(fu.SQRT5)
    A, b, xstar = fu.planted_system()
    Atot, btot = rounding.convert_system(A, b, field)
    x = fu.embed(xstar, field)
    with pytest.raises(ValueError, match="form must be"):
        rounding.field_least_squares(Atot, btot, x, field, 5, form="both", gemm=fu.host_gemm, solve=_host_solve)
    with pytest.raises(ValueError, match="regularization must be positive"):
        rounding.field_least_squares(Atot, btot, x, field, 5, regularization=0.0, gemm=fu.host_gemm, solve=_host_solve)
    with pytest.raises(ValueError, match="Atot must be"):
        rounding.field_least_squares(Atot, btot, x[:-1], field, 5, gemm=fu.host_gemm, solve=_host_solve)


# ---- the problem over the field ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("icosahedron", "600-cell"))
def test_to_sdp_of_the_field_problems_is_delsarte_exact(name):
    """every number of `to_sdp(prec)` against `delsarte_exact(n, d, <the expression of field_round_util.DELSARTE>, prec)`, both flattened at 6 limbs:
    within 2^(6 - prec) absolute (the entries are O(1))"""
    import clrs_amd
    from clrs_amd import mw, problems, sdp
    from tests import field_round_util as fru
    prec = 256
    n, d, expr = fru.DELSARTE[name][:3]
    with sdp.data_planes(6):
        got = clrs_amd.flatten(fu.delsarte_field_problem(name).to_sdp(prec))
        want = clrs_amd.flatten(problems.delsarte_exact(n, d, expr, prec))
    assert got.constant == want.constant and got.maximize == want.maximize and np.array_equal(got.block_n, want.block_n)
    for key in ("B", "c", "C", "b", "term_lambda", "term_vs", "term_ws", "dense_A"):
        a, b = got.data_planes_of(key, 6), want.data_planes_of(key, 6)
        assert a.shape == b.shape, key
        worst = max([abs(v) for v in mw.from_limbs(a - b)] + [0]) if a.size else 0
        assert worst <= mp.ldexp(1, 6 - prec), (key, worst)
    lam = fu.delsarte_field_problem(name).blocks[0][-1].entries[(0, 0)][0].lam[0]
    assert isinstance(lam, tuple) and len(lam) == 2 and lam[1] != 0                       # the weights of block "B" are field elements
    with pytest.raises(ValueError, match="costheta needs 2 coefficients"):
        problems.delsarte_exact_problem(n, d, (Fraction(1),), field=fu.field_of(fu.SQRT5))


@pytest.mark.parametrize("transformed", (False, True))
def test_linear_system_over_the_field_against_the_dense_restatement(transformed):
    from tests import lrsys_util as lu
    problem = fu.handmade_field_problem()
    problem.to_sdp().check()                                            # the transposed partners are present
    Bs = fu.handmade_field_Bs() if transformed else None
    rows, b, index = fu.restated_field_system(problem, Bs)
    assemble = lu.Counting(lu.host_assemble)
    A, b2, index2 = rounding.linear_system(problem, Bs=Bs, assemble=assemble, field=problem.field)
    assert index2 == index == rounding.system_index(problem, Bs, problem.field) and b2 == b
    assert A.shape == (5, len(index)) and [list(r) for r in A] == rows
    assert len(assemble.calls) == 2                                     # still one call per low-rank block
    assert all(isinstance(v, tuple) and len(v) == 2 for v in A.flat) and any(v[1] != 0 for v in A.flat)
    from tests import dixon_multi_util as dm
    A3, _, _ = rounding.linear_system(problem, Bs=Bs, assemble=lu.host_assemble, matmul=dm.host_matmul, field=problem.field)
    assert [list(r) for r in A3] == rows
    cols = [len(index) - 1, 3, 3, 0]
    A4, _, index4 = rounding.linear_system(problem, Bs=Bs, columns=cols, assemble=lu.host_assemble, field=problem.field)
    assert index4 == [index[c] for c in cols] and [list(r) for r in A4] == [[row[c] for c in cols] for row in rows]


def test_exact_solution_over_the_field_on_the_oracle_iterate_of_the_icosahedron(oracle_built):
    """the 320-bit oracle's last iterate at the gap 1e-40 in 5 limbs, every device call through a host stand-in (the solve: the restatement of clrs_mw_posv)"""
    from tests import field_round_util as fru
    problem = fu.delsarte_field_problem("icosahedron")
    snap, _ = fru.oracle_iterate("icosahedron", 1e-40)
    sol = fru.Sol(np.asarray(snap.X)[:5], np.asarray(snap.Y)[:5])
    off = rounding.RoundingSettings(reduce_kernelvectors=False)
    with pytest.raises(NotImplementedError, match="reduction of kernel vectors over a number field"):
        rounding.exact_solution(problem, sol, limbs=5, field=problem.field, **fu.host_hooks())
    res = rounding.exact_solution(problem, sol, settings=off, limbs=5, field=problem.field, **fu.host_hooks())
    assert res.success and res.correct_slacks
    assert res.objective == (Fraction(12), Fraction(0))
    assert res.certificates and all(isinstance(c, rounding.FieldPDCertificate) and c.pd for c in res.certificates)
    assert [res.Bs[bi][2] for bi in sorted(res.Bs)] == [1, 0, 0, 0, 0, 0, 1, 3, 1]
    # every constraint holds exactly in the field for the untransformed blocks
    blocks = [bl for _, bl in problem.flat_blocks()]
    for p in range(len(problem.c[0])):
        total = [Fraction(0), Fraction(0)]
        for bl, Y in zip(blocks, res.Y):
            M = fu.dense_field_constraint(bl, p, fu.SQRT5)
            for i in range(bl.n):
                for j in range(bl.n):
                    if any(M[i, j]) and any(Y[i, j]):
                        total = [u + v for u, v in zip(total, fu.mul(M[i, j], Y[i, j], fu.SQRT5))]
        assert tuple(total) == (problem.c[0][p], Fraction(0)), p

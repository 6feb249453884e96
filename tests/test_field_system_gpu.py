"""`field_least_squares` with its device calls (the products by clrs_mw_gemm, the solve by clrs_mw_posv) on the planted systems of
tests/test_field_system_cpu.py, against the reference's method in mpmath at 1000 bits and against the run through the host stand-ins."""
from fractions import Fraction

import mpmath as mp
import pytest

from clrs_amd import rounding
from tests import field_system_util as fu
from tests import posv_util as pu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("minpoly,n,m", ((fu.SQRT5, 4, 6), (fu.SQRT5, 7, 5), (fu.CBRT2, 3, 4)), ids=("sqrt5-wide", "sqrt5-tall", "cbrt2"))
def test_field_least_squares_on_the_device(minpoly, n, m):
    limbs, dec = 5, 40
    field = fu.field_of(minpoly)
    A, b, xstar = fu.planted_system(seed=n + m, n=n, m=m, minpoly=minpoly)
    Atot, btot = rounding.convert_system(A, b, field)
    with mp.workprec(700):
        x = [v + mp.mpf(10) ** -45 * (1 + c) for c, v in enumerate(fu.embed(xstar, field))]
    r_ref = fu.residual(Atot, btot, fu.reference_least_squares(Atot, btot, x, field, decimals=dec))
    norm = max(sum((abs(v) for v in Atot[i]), Fraction(0)) for i in range(Atot.shape[0]))
    for form in ("primal", "dual"):
        xr = rounding.field_least_squares(Atot, btot, x, field, limbs, 1e-30, dec, form=form)
        r = fu.residual(Atot, btot, xr)
        print(form, "r", float(r), "r_ref", float(r_ref))
        assert r <= 4 * r_ref + norm * Fraction(1, 10 ** dec)
        # the device products and the mpmath stand-in round differently; the solve is the same bits given the same matrix: the cut numbers differ by a few units
        host = rounding.field_least_squares(Atot, btot, x, field, limbs, 1e-30, dec, form=form, gemm=fu.host_gemm, solve=lambda G, v, K, device=0: pu.host_solve(G, v, K))
        assert max(abs(u - v) for u, v in zip(xr, host)) <= Fraction(1, 10 ** (dec - 5))


@pytest.mark.parametrize("transformed", (False, True))
def test_linear_system_over_the_field_on_the_device(transformed):
    """the device `assemble` (clrs_zz_lowrank_system, one call per low-rank block) and `zz_matmul` against the dense restatement in tuple arithmetic"""
    from tests import lrsys_util as lu
    problem = fu.handmade_field_problem()
    Bs = fu.handmade_field_Bs() if transformed else None
    rows, b, index = fu.restated_field_system(problem, Bs)
    assemble = lu.Counting(rounding.lowrank_system)
    A, b2, index2 = rounding.linear_system(problem, Bs=Bs, assemble=assemble, matmul=rounding.zz_matmul, field=problem.field)
    assert index2 == index and b2 == b and [list(r) for r in A] == rows
    assert len(assemble.calls) == 2 and rounding.lowrank_system.last_info[0] == 0


@pytest.mark.parametrize("name,bound,kept", (("icosahedron", 12, {}), ("600-cell", 120, {19: 8, 20: 6})))
def test_exact_solution_over_the_field_on_the_device(name, bound, kept):
    """solvesdp_mw at 10 limbs, gap 1e-40, then every step of exact_solution(field=) with its device call: the exact bounds 12 and 120"""
    import clrs_amd
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    problem = fu.delsarte_field_problem(name)
    with data_planes(10):
        f = clrs_amd.flatten(problem.to_sdp(640))
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    assert res.error_code == 0 and res.status == "Optimal"
    sol = rounding.exact_solution(problem, res, rounding.RoundingSettings(reduce_kernelvectors=False), reconstruct=rounding.dixon_reconstruct,
                                  matmul=rounding.zz_matmul, field=problem.field)
    assert sol.success and sol.correct_slacks and sol.objective == (Fraction(bound), Fraction(0))
    assert sol.certificates and all(c.pd for c in sol.certificates)
    for bi, s in kept.items():
        assert sol.Bs[bi][2] == s

"""rounding.inverse_field, complete_basis_field, field_matmul, transform_field / undo_transform_field and basis_transformations(field=...) (DESIGN.md
section 25) through the host stand-ins of tests/field_inverse_util.py for `adjugate=`, `batch=` and `matmul=`, against `Fraction` eliminations over the field:
the golden kernels of the reference's 600-cell and icosahedron examples over Q(sqrt 5), planted matrices over every field of tests/pd_field_util.py, a
determinant equal to a split prime, a singular matrix, a coefficient at the edge of what the primes drawn can lift.  No GPU."""
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import rounding
from clrs_amd.rounding import RoundingSettings
from tests import field_inverse_util as iu
from tests import pd_field_util as fu

F5 = [-5, 0, 1]
UNREDUCED = RoundingSettings(reduce_kernelvectors=False)


def check_inverse(fld, B, want, result, nprimes=None):
    """`result` is the FieldInverse of B: the exact inverse, its certificate consistent, and the prime count the one the bound demands"""
    f = fld.minpoly
    n = len(B)
    assert iu.as_lists(result.inverse) == want
    assert iu.matmul_exact(f, B, iu.as_lists(result.inverse)) == iu.identity(f, n)
    scale, lc, M = iu.integer_form(fld, B)
    assert result.scale == scale and result.generator_scale == lc and result.minpoly == rounding._field_monic(fld)[0]
    det = iu.determinant_exact(f, [[tuple(x * scale for x in e) for e in row] for row in B])
    assert iu.to_g(lc, result.det) == det                                                     # det(scale B), exactly
    adj = [[iu.to_g(lc, e) for e in row] for row in result.adjugate]
    assert adj == [[fu.mul(f, det, e) for e in row] for row in iu.matmul_exact(f, want, [[fu.el(f, F(int(i == j), scale)) for j in range(n)] for i in range(n)])]
    bound = rounding.field_adjugate_bounds(M, fld)
    assert max(abs(c) for row in result.adjugate for e in row for c in e) <= bound and max(abs(c) for c in result.det) <= bound
    count = iu.first_primes_needed(fld, bound)
    assert len(result.primes) - len(result.discarded) == count and (nprimes is None or count == nprimes)
    assert result.primes == rounding.split_primes(fld, len(result.primes))[0]
    assert result.roots == [[r * lc % p for r in rr] for p, rr in zip(*rounding.split_primes(fld, len(result.primes)))]


@pytest.mark.parametrize("case,key", iu.GOLDEN_BLOCKS)
def test_golden_blocks(case, key):
    fld = fu.field("x2-5")
    N, s, vectors, extra, B, want = iu.golden_basis(case, key)
    assert extra == iu.GOLDEN_COMPLETIONS[(case, key)]
    iu.host_field_adjugate.calls.clear()
    result = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    assert result.discarded == [] and iu.host_field_adjugate.calls == [iu.GOLDEN_PRIMES[(case, key)]]          # one call, with the primes the bound demands
    check_inverse(fld, B, want, result, nprimes=iu.GOLDEN_PRIMES[(case, key)])
    again = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate, matmul=iu.host_matmul)
    assert iu.as_lists(again.inverse) == want and again.det == result.det


@pytest.mark.parametrize("name", fu.FIELDS)
@pytest.mark.parametrize("n", (1, 2, 5, 8))
def test_planted_matrices_over_every_field(name, n):
    fld, B, want = iu.planted(name, n)
    result = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    assert result.discarded == []
    check_inverse(fld, B, want, result)


def test_field_adjugate_bounds_is_hadamard_times_the_coefficient_factor():
    """x^2 - 5: rho = 5, T = [[2, 0], [0, 10]], the factor max(2 / 2, 2 * 5 / 10) = 1; rows (3 + 4 g, 0), (0, 1): E = [[23, 0], [0, 1]], H = 23"""
    fld = fu.field("x2-5")
    assert rounding.field_adjugate_bounds([[[3, 0], [0, 1]], [[4, 0], [0, 0]]], fld) == 23
    assert rounding.field_adjugate_bounds([[[3, 4], [0, 0]], [[0, 0], [0, 0]]], fld) == 5                 # a zero row counts as 1, not 0: the minors without it
    with pytest.raises(ValueError):
        rounding.field_adjugate_bounds([[[1]], [[1]], [[1]]], fld)
    # the non-monic 2 x^2 - 5: h = 2 g has h^2 = 10, rho = 10, T = [[2, 0], [0, 20]], factor max(1, 2 * 10 / 20) = 1
    assert rounding.field_adjugate_bounds([[[1]], [[1]]], fu.field("2x2-5")) == 11


def test_a_determinant_equal_to_the_first_split_prime():
    """diag(p, 1) U with U unimodular over Z[g]: both pairs of p are singular, p lands in `discarded`, and the inverse is that of the elimination"""
    fld = fu.field("x2-5")
    p, _ = fu.first_split_prime("x2-5")
    U = [[fu.el(F5, 1), fu.el(F5, 2, 1)], [fu.el(F5, 0), fu.el(F5, 1)]]
    B = iu.matmul_exact(F5, [[fu.el(F5, p), fu.el(F5, 0)], [fu.el(F5, 3, -1), fu.el(F5, 1)]], U)
    assert iu.determinant_exact(F5, B) == fu.el(F5, p)
    iu.host_field_adjugate.calls.clear()
    result = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    assert result.discarded == [p] and result.primes[0] == p and result.det == [p, 0]
    assert len(iu.host_field_adjugate.calls) == 2                                               # the replacement is a second call
    check_inverse(fld, B, iu.inverse_exact(F5, B), result)


def test_a_singular_matrix_is_proved_singular():
    """two columns proportional by g: every pair of every split prime is singular, and the discarded primes outgrow the bound on the norm"""
    fld = fu.field("x2-5")
    g = fu.el(F5, 0, 1)
    col = [fu.el(F5, 1, 2), fu.el(F5, -3, 1), fu.el(F5, 2)]
    B = [[col[i], fu.mul(F5, g, col[i]), fu.el(F5, i, 1)] for i in range(3)]
    assert iu.inverse_exact(F5, B) is None
    iu.host_field_adjugate.calls.clear()
    with pytest.raises(rounding.SingularSystemError, match="singular"):
        rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    _, _, M = iu.integer_form(fld, B)
    H, _ = rounding._field_hadamard(np.array(M, dtype=object), F5)
    primes = rounding.split_primes(fld, sum(iu.host_field_adjugate.calls))[0]
    assert np.prod(primes, dtype=object) > H ** 2 >= np.prod(primes[:-1], dtype=object)         # it stopped at the first product past H^d


@pytest.mark.parametrize("sign", (1, -1))
def test_a_coefficient_at_the_edge_of_the_primes_drawn_still_lifts(sign):
    """diag(a, 1) with 2 |a| = p - 1: the bound is |a| (factor 1 over x^2 - 5), ONE prime is drawn, and adj = diag(1, a) has a coefficient at the very end
    of the symmetric range of that prime"""
    fld = fu.field("x2-5")
    p, _ = fu.first_split_prime("x2-5")
    a = sign * (p - 1) // 2
    B = [[fu.el(F5, a), fu.el(F5, 0)], [fu.el(F5, 0), fu.el(F5, 1)]]
    assert rounding.field_adjugate_bounds(iu.integer_form(fld, B)[2], fld) == abs(a)
    result = rounding.inverse_field(B, fld, adjugate=iu.host_field_adjugate)
    assert result.primes == [p] and result.discarded == [] and result.det == [a, 0]
    assert [list(row) for row in result.adjugate] == [[(1, 0), (0, 0)], [(0, 0), (a, 0)]]
    assert iu.as_lists(result.inverse) == [[fu.el(F5, F(1, a)), fu.el(F5, 0)], [fu.el(F5, 0), fu.el(F5, 1)]]
    one_more = [[fu.el(F5, a + sign), fu.el(F5, 0)], [fu.el(F5, 0), fu.el(F5, 1)]]              # 2 |a| = p + 1: a second prime
    assert len(rounding.inverse_field(one_more, fld, adjugate=iu.host_field_adjugate).primes) == 2


def test_a_wrong_residue_is_caught_by_the_check():
    fld, B, _ = iu.planted("x2-2", 5)

    def off_by_one(mats, primes, roots, device=0):
        adj, det, brk = iu.host_field_adjugate(mats, primes, roots)
        adj[0, 0, 1, 2] = (adj[0, 0, 1, 2] + 1) % primes[0]
        return adj, det, brk
    with pytest.raises(ArithmeticError, match="adj"):
        rounding.inverse_field(B, fld, adjugate=off_by_one)


def test_degree_one_and_plain_entries_go_to_inverse_qq(monkeypatch):
    calls = []

    def recorder(B, **kw):
        calls.append((B, sorted(kw)))
        return "from inverse_qq"
    never = lambda *a, **kw: pytest.fail("the field path was taken")
    monkeypatch.setattr(rounding, "inverse_qq", recorder)
    B = [[F(2), F(1)], [F(1), F(1)]]
    assert rounding.inverse_field(B, fu.field("x2-5"), adjugate=never, primes=never) == "from inverse_qq"        # entries that are no tuples
    with fu.mp.workprec(200):
        rational = rounding.NumberField([-3, 2], fu.mp.mpf(3) / 2)
    assert rounding.inverse_field([[(F(2),), (F(1),)], [(F(1),), (F(1),)]], rational, adjugate=never, primes=never) == "from inverse_qq"
    assert [c[0] for c in calls] == [B, B] and calls[0][1] == ["check", "device", "matmul"]


@pytest.mark.parametrize("name", fu.FIELDS)
def test_field_matmul_with_and_without_matmul(name):
    fld = fu.field(name)
    f = fld.minpoly
    A, B = fu.random_elements(5, f, 4, 3), fu.random_elements(6, f, 3, 5)
    A = [[tuple(x / 3 for x in e) for e in row] for row in A]
    B = [[tuple(x / 2 for x in e) for e in row] for row in B]
    want = iu.matmul_exact(f, A, B)
    iu.host_matmul.calls = 0
    plain, stacked = rounding.field_matmul(A, B, fld), rounding.field_matmul(A, B, fld, matmul=iu.host_matmul)
    assert iu.host_matmul.calls == 1                                                            # ONE integer product of the stacked planes
    assert plain.shape == (4, 5) and iu.as_lists(plain) == want and iu.as_lists(stacked) == want
    assert iu.as_lists(rounding.field_matmul(A, B, f)) == want                                  # the minimal polynomial itself in place of the field
    with pytest.raises(ValueError):
        rounding.field_matmul(A, A, fld)


def test_transform_then_undo_transform_is_the_identity():
    """both against the products over the field; and with s = 0, `undo_transform_field` with the transposed inverse of the change takes back what
    `transform_field` did: B (Binv Y Binv^T) B^T = Y"""
    fld, Binv, B = iu.planted("x3-2", 5)                             # a random matrix in the role of Binv, its exact inverse in the role of B
    f, s = fld.minpoly, 2
    T = lambda M: [list(r) for r in zip(*M)]
    L = fu.random_elements(9, f, 5, 5, size=2)
    Y = iu.matmul_exact(f, L, T(L))                                  # a symmetric block
    assert Y == T(Y)
    P = Binv[s:]
    want = iu.matmul_exact(f, iu.matmul_exact(f, P, Y), T(P))
    for hook in (None, iu.host_matmul):
        got = rounding.transform_field(Y, Binv, s, fld, matmul=hook)
        assert got.shape == (3, 3) and iu.as_lists(got) == want
        padded = [[want[i - s][j - s] if i >= s and j >= s else iu.zero(f) for j in range(5)] for i in range(5)]
        back = rounding.undo_transform_field(want, Binv, s, fld, matmul=hook)
        assert back.shape == (5, 5) and iu.as_lists(back) == iu.matmul_exact(f, iu.matmul_exact(f, T(Binv), padded), Binv)
        whole = rounding.transform_field(Y, Binv, 0, fld, matmul=hook)
        assert iu.as_lists(rounding.undo_transform_field(whole, T(B), 0, fld, matmul=hook)) == Y
    with pytest.raises(ValueError):
        rounding.undo_transform_field(want, Binv, 3, fld)
    with pytest.raises(ValueError):
        rounding.transform_field(Y, Binv, 6, fld)


@pytest.mark.parametrize("case", ("600-cell", "icosahedron"))
def test_basis_transformations_on_the_golden_kernels(case):
    fld = fu.field("x2-5")
    kernels = iu.golden_kernels(case)
    out = rounding.basis_transformations(kernels, UNREDUCED, field=fld, **iu.host_hooks())
    assert list(out) == list(kernels)
    for key, (N, vectors) in kernels.items():
        Bt, Binv, s = out[key]
        B = [list(r) for r in zip(*iu.as_lists(Bt))]
        assert s == len(vectors) and Bt.shape == (N, N) and Binv.shape == (N, N)
        assert [[B[i][c] for i in range(N)] for c in range(s)] == vectors                        # the first s columns are the vectors
        extra = iu.completion_exact(F5, vectors, N)
        assert [[B[i][s + c] for i in range(N)] for c in range(N - s)] == [[fu.el(F5, int(i == j)) for i in range(N)] for j in extra]
        assert (case, key) not in iu.GOLDEN_COMPLETIONS or extra == iu.GOLDEN_COMPLETIONS[(case, key)]
        assert iu.matmul_exact(F5, B, iu.as_lists(Binv)) == iu.identity(F5, N)
        V = [[vectors[c][i] for c in range(s)] for i in range(N)]
        assert iu.matmul_exact(F5, iu.as_lists(Binv)[s:], V) == [[iu.zero(F5)] * s for _ in range(N - s)] or s == N
        if (case, key) in iu.GOLDEN_BLOCKS:
            assert iu.as_lists(Binv) == iu.golden_basis(case, key)[5]


def test_basis_transformations_keeps_its_refusals():
    fld = fu.field("x2-5")
    kernels = iu.golden_kernels("icosahedron")
    with pytest.raises(NotImplementedError, match="degree above 1"):                            # no field: today's message
        rounding.basis_transformations(kernels, UNREDUCED, **iu.host_hooks())
    with pytest.raises(NotImplementedError, match="reduce_kernelvectors.*(HNF|LLL)"):           # rational vectors, the reduction without reduce=
        rounding.basis_transformations({0: (2, [[F(1), F(2)]])}, None, **iu.host_hooks())
    for settings in (None, RoundingSettings()):
        with pytest.raises(NotImplementedError, match="reduction of kernel vectors over number fields"):
            rounding.basis_transformations(kernels, settings, field=fld, **iu.host_hooks())
    empty = rounding.basis_transformations({"none": (2, [])}, UNREDUCED, field=fld, **iu.host_hooks())           # nothing holds a tuple: the path over QQ
    assert empty["none"][2] == 0 and empty["none"][0][0, 0] == 1


def test_complete_basis_field():
    fld = fu.field("x2-5")
    N, vectors = iu.golden_kernels("600-cell")["20"]
    V = [[vectors[c][i] for c in range(len(vectors))] for i in range(N)]
    extra = rounding.complete_basis_field(V, fld, batch=iu.host_rref)
    p, roots = fu.first_split_prime("x2-5")
    assert list(extra) == [0, 1, 2] and extra.p == p and extra.root == roots[0] and extra.primes == [p]
    assert list(rounding.complete_basis_field([[fu.el(F5, 1)][:0]] * 3, fld, batch=iu.host_rref)) == [0, 1, 2]          # no vectors: every unit vector
    g = fu.el(F5, 0, 1)
    dependent = [[fu.el(F5, 1), g], [g, fu.el(F5, 5)], [fu.el(F5, 2), fu.mul(F5, g, fu.el(F5, 2))]]
    with pytest.raises(ValueError, match="dependent"):
        rounding.complete_basis_field(dependent, fld, maxprimes=2, batch=iu.host_rref)
    # r0 - g vanishes at the first pair only: the vector (r0 - g, 0) is refused there and accepted at the second root of the same prime
    late = rounding.complete_basis_field([[fu.el(F5, roots[0], -1)], [fu.el(F5, 0)]], fld, batch=iu.host_rref)
    assert list(late) == [1] and late.p == p and late.root == roots[1]

"""Linear-dependency preprocessing (clrs_amd.preprocess) on the CPU: the host-side steps (conditions on the free variables, substitution,
duplicate variables, renumbering, postprocess) driven by the mpmath rank-revealing elimination of tests/preprocess_host.py, and the
reference's linear-dependency suite (test/runtests_solver.jl:249-314) through `preprocess` and the 320-bit oracle."""
import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd.mw import to_limbs
from clrs_amd.preprocess import LINDEP_MESSAGE, detect_limbs, postprocess, preprocess, threshold
from clrs_amd.problems.toy import dense_sdp, lindep_suite
from clrs_amd.solver import _HostBlocks
from oracle.oracle import Oracle
from tests.preprocess_host import HostReveal, pivoted_cholesky
from tests.util import flat

SUITE = lindep_suite()
# removed constraints and free variables before -> after, per problem (None: the reference expects an error)
COUNTS = [(1, 2, 1), (2, 2, 0), (2, 2, 1), None, (0, 2, 1), (3, 3, 1), (1, 2, 1), None, None, (1, 0, 0)]
EXPECTED = [1.0, 1.25, 1.0, None, 1.5, 1.25, 0.0, None, None, 1.0]


def slacks(f, y, Y):
    """sum_l <A_p, Y_l> + (B y)_p - c_p of every constraint of the FlatSDP f (fp64)"""
    s = _HostBlocks(f).trace_A(np.asarray(Y, dtype=np.float64)) - f.c
    N = f.n_free
    for j in range(f.n_clusters):
        o, P = int(f.cluster_off[j]), int(f.cluster_P[j])
        if N:
            s[o:o + P] += f.B[o * N:(o + P) * N].reshape(P, N, order="F") @ np.asarray(y, dtype=np.float64)
    return s


def test_suite_is_the_references():
    assert len(SUITE) == 10
    assert [e for _, _, e, _ in SUITE] == EXPECTED
    assert [bool(kw) for _, _, _, kw in SUITE] == [True, True, True] + [False] * 7      # omega_p = omega_d = 10 where the reference passes it


@pytest.mark.parametrize("k", range(10), ids=[s[0] for s in SUITE])
def test_suite_through_preprocess_and_oracle(k):
    name, sdp, expect, kw = SUITE[k]
    f = clrs_amd.flatten(sdp)
    if expect is None:
        with pytest.raises(ValueError) as e:
            preprocess(f, reveal=HostReveal)
        assert str(e.value) == LINDEP_MESSAGE
        return
    red, cs, vr = preprocess(f, reveal=HostReveal)
    assert (len(cs), f.n_free, red.n_free) == COUNTS[k]
    assert red.x_len == f.x_len - len(cs)
    r = Oracle(red, mp_bits=320).solvesdp(**kw)
    assert r["error_code"] == 0
    print(name, "p_obj", r["p_obj"], "d_obj", r["d_obj"])
    assert abs(r["p_obj"] - expect) < 1e-5 and abs(r["d_obj"] - expect) < 1e-5
    x, y = postprocess(r["x"], r["y"], cs, vr)
    assert x.shape == (f.x_len,) and y.shape == (f.n_free,)
    assert all(x[i] == 0.0 for i, _, _ in cs)
    s = slacks(f, y, r["Y"])
    print(name, "slack norm", np.linalg.norm(s))
    assert np.linalg.norm(s) < 1e-5


def test_problem_without_dependencies_comes_back_unchanged():
    f = flat("x2p1")
    red, cs, vr = preprocess(f, reveal=HostReveal)
    assert red is f and cs == []
    assert vr[0] == [] and vr[4] == [] and vr[5] == list(range(f.n_free))


@pytest.mark.parametrize("e,rank", [(100, 3), (140, 2)])
def test_threshold_semantics_at_256_bits(e, rank):
    """A constraint equal to a combination of two others plus 2^-e times an independent direction: its Gram pivot is 2^-2e, on either side of
    eps = 2^-255 (|R_ii| on either side of the reference's tol = 2^-127.5)."""
    prec = 256
    D = detect_limbs(prec)
    assert D == 6
    with mp.workprec(52 * D + 64):
        v = [[mp.mpf(1), 0, 0, 0], [0, mp.mpf(1), 0, 0]]
        v.append([mp.mpf(2), mp.mpf(-3), mp.mpf(2) ** -e, 0])
        G = [[mp.fsum(a * b for a, b in zip(v[i], v[j])) for j in range(3)] for i in range(3)]
        Gl = to_limbs([G[i][j] for j in range(3) for i in range(3)], D)
    tau = threshold(prec, D, float(max(G[i][i] for i in range(3))))
    assert tau == 2.0 ** -255
    perm, r, W, resid = HostReveal(None, D).rank_reveal(Gl, 3, 3, tau)
    assert r == rank
    if r == 2:
        assert sorted(perm[:2]) == [0, 2] and perm[2] == 1          # largest diagonals first: 13, then 1 (ties to the smallest index)


def _planted():
    rng = np.random.default_rng(7)
    n = 3
    A = [rng.integers(-3, 4, (n, n)).astype(float) for _ in range(4)]
    A = [a + a.T for a in A]
    B = rng.integers(-2, 3, (4, 3)).astype(float)
    B = np.hstack([B, B[:, :1]])                       # a duplicated free-variable column
    c = rng.integers(-2, 3, 4).astype(float)
    cons = [(c[i], {0: A[i]}, list(B[i])) for i in range(4)]
    cons.append((2 * c[0] - c[2], {0: 2 * A[0] - A[2]}, list(2 * B[0] - B[2])))                 # an exact dependency: 0 = 0 on the free variables
    cons.append((c[1] + c[3] + 1.0, {0: A[1] + A[3]}, list(B[1] + B[3] + np.array([0, 1.0, 2.0, 0]))))      # fixes y_1 + 2 y_2 = 1
    return dense_sdp([n], cons, {0: np.eye(n)}, maximize=False, free=list("abcd"), b=[1.0, -1.0, 0.5, 2.0])


def test_round_trip_on_planted_relations():
    f = clrs_amd.flatten(_planted())
    red, cs, vr = preprocess(f, reveal=HostReveal)
    fv_zeros, fv_nonzeros, Rref, rhs, nf, ff = vr
    assert len(cs) == 2 and len(nf) == 1 and len(fv_zeros) == 1 and red.n_free == 2
    rng = np.random.default_rng(1)
    xr, yr = rng.standard_normal(red.x_len), rng.standard_normal(red.n_free)
    x, y = postprocess(xr, yr, cs, vr)
    assert all(x[i] == 0.0 for i, _, _ in cs) and np.array_equal(np.delete(x, [i for i, _, _ in cs]), xr)
    # [I Rref] [y_nf; y_ff] = rhs_changed
    for a, v in enumerate(nf):
        assert abs(y[v] + sum(float(Rref[a, k]) * y[ff[k]] for k in range(len(ff))) - float(rhs[a])) < 1e-13
    assert all(y[ff[k]] == 0.0 for k in fv_zeros)
    # the kept constraints of the original problem at the postprocessed y are the reduced problem's at the reduced y ...
    Y = np.zeros(f.xy_len)
    s_full, s_red = slacks(f, y, Y), slacks(red, yr, Y)
    kept = np.delete(np.arange(f.x_len), [i for i, _, _ in cs])
    assert np.max(np.abs(s_full[kept] - s_red)) < 1e-12
    # ... the removed ones follow from them, and the objectives agree
    assert abs((f.constant + f.b @ y) - (red.constant + red.b @ yr)) < 1e-12
    # planar limbs go through unrounded
    x2, y2 = postprocess(np.vstack([xr, 1e-20 * xr]), np.vstack([yr, 1e-20 * yr]), cs, vr)
    assert x2.shape == (2, f.x_len) and y2.shape == (2, f.n_free) and np.allclose(y2[0], y)


def test_host_elimination_pivot_rule():
    G = [[mp.mpf(v) for v in row] for row in [[4, 2, 4, 0], [2, 5, 2, 1], [4, 2, 4, 0], [0, 1, 0, 9]]]
    perm, r, W, resid, piv = pivoted_cholesky(G, ncand=3, tau=mp.mpf(2) ** -200)
    assert perm[:r] == [1, 0] and r == 2 and perm[r:] == [2, 3]            # 5 first, then the tie 4 = 4 goes to index 0; index 3 is no candidate
    assert abs(W[1][0] - 1) < 1e-60 and abs(W[0][0]) < 1e-60               # column 2 = column 0

"""Linear-dependency preprocessing on the device: the rank-revealing Cholesky kernel (k_mw_rank_reveal) against the mpmath elimination of
tests/preprocess_host.py, the constraint Gram matrices against the oracle's assembly at X = Y = I, the reference's linear-dependency suite
(test/runtests_solver.jl:249-314) through `solvesdp_mw(preprocess=True)`, and dependencies planted into real instances.

Accuracy of the relations W = G11^-1 G12 (a measurement, at the first seed whose instance is unambiguous): residual max |G12 - G11 W| / max G_ii at
4 * 52 K bits, device / host elimination at 52 K bits with the same pivots -- written per (K, n) to profiles/preprocess/rank_reveal_residuals.json
when CLRS_WRITE_PROFILES is set."""
import json
import os

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd.preprocess import LINDEP_MESSAGE
from clrs_amd.problems.toy import lindep_suite
from tests.preprocess_host import limbs_to_mp, pivoted_cholesky, plant_dependencies, relation_residual
from tests.util import flat, instance, mw_relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, planted rank, candidates): one row, a rank-1 pair, LDS-resident sizes, candidates < n, and sizes beyond LDS at every limb count
SHAPES = [(1, 1, 1), (2, 1, 2), (7, 4, 7), (33, 20, 33), (64, 30, 50), (65, 25, 65), (130, 40, 130)]


def planted_gram(n, r, seed):
    """G = M^T M, M small-integer with n columns of which r are independent and the others integer combinations of two or three of them: the
    dependencies are exact in fp64; column i is scaled by a distinct factor pattern so that the column norms differ."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, (r + 3, r)).astype(float)
    cols = rng.permutation(n)
    M = np.zeros((r + 3, n))
    M[:, cols[:r]] = base
    for c in cols[r:]:
        k = rng.choice(r, size=min(r, int(rng.integers(2, 4))), replace=False)
        M[:, c] = base[:, k] @ rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(k))
    return M.T @ M


def unambiguous(G, ncand, tau, bits):
    """host elimination at `bits` bits; None unless the smallest accepted pivot is >= 2^64 tau and every choice is clear of the runner-up"""
    perm, r, W, resid, piv = pivoted_cholesky([[mp.mpf(v) for v in row] for row in G], ncand, tau, bits)
    if r and min(piv) < mp.mpf(2) ** 64 * tau:
        return None
    return perm, r


def clear_choices(G, ncand, order, bits):
    """every pivot of `order` beats the other remaining candidates by a relative margin > 2^-30 (or ties exactly, which both sides break by index)"""
    n = len(G)
    with mp.workprec(bits):
        A = [[mp.mpf(v) for v in row] for row in G]
        rest = list(range(n))
        for p in order:
            d = A[p][p]
            for i in rest:
                if i != p and i < ncand and A[i][i] != d and abs(A[i][i] - d) <= d * mp.mpf(2) ** -30:
                    return False
            rest.remove(p)
            for i in rest:
                f = A[i][p] / d
                for c in rest:
                    if c <= i:
                        A[i][c] = A[c][i] = A[i][c] - f * A[c][p]
    return True


@pytest.mark.parametrize("K", [4, 5, 6, 8, 10])
def test_rank_reveal_kernel_matches_host_elimination(K):
    from clrs_amd.mw import rank_reveal
    bits = 4 * 52 * K
    mats, host = [], []
    for (n, r, ncand) in SHAPES:
        for seed in range(20):
            G = planted_gram(n, r, 1000 * n + seed)
            tau = 2.0 ** -(52 * K - 32) * float(np.max(np.diag(G)))
            h = unambiguous(G, ncand, tau, bits)
            if h is not None and clear_choices(G, ncand, h[0][:h[1]], bits):
                break
        else:
            raise AssertionError(("no unambiguous instance", n, r))
        # precondition (host, 4 * 52 K bits): the smallest accepted pivot is >= 2^64 tau, so the rank is not a matter of rounding
        assert h is not None
        mats.append((G, n, ncand, tau))
        host.append(h)
    Gl = np.zeros((K, sum(n * n for _, n, _, _ in mats)))
    Gl[0] = np.concatenate([G.reshape(-1, order="F") for G, _, _, _ in mats])
    out = rank_reveal(Gl, [m[1] for m in mats], [m[2] for m in mats], [m[3] for m in mats], K)
    record = {}
    for (G, n, ncand, tau), (hperm, hr), (perm, r, W, resid) in zip(mats, host, out):
        assert r == hr, (n, r, hr)
        assert list(perm) == list(hperm), (n, list(perm), hperm)
        assert all(p < ncand for p in perm[:r])
        assert sorted(perm[r:]) == list(perm[r:])
        Gm = [[mp.mpf(v) for v in row] for row in G]
        with mp.workprec(bits):
            w = limbs_to_mp(W)
            Wd = [[w[c + a * r] for a in range(n - r)] for c in range(r)]
            res_dev = relation_residual(Gm, list(perm), r, Wd, bits)
            # the remaining diagonal of exact dependencies is rounding noise
            rd = limbs_to_mp(resid)
            assert all(abs(v) <= tau for a, v in enumerate(rd) if perm[r + a] < ncand)
        _, _, Wh, _, _ = pivoted_cholesky(Gm, ncand, tau, 52 * K, order=list(hperm[:hr]))
        res_host = relation_residual(Gm, list(hperm), hr, Wh, bits)
        bound = max(64 * res_host, mp.mpf(2) ** -(52 * K))
        print("K", K, "n", n, "r", r, "residual device", mp.nstr(res_dev, 5), "host", mp.nstr(res_host, 5), "bound", mp.nstr(bound, 5))
        record[str(n)] = dict(rank=r, ncand=ncand, device=float(mp.log(res_dev, 2)) if res_dev else None, host=float(mp.log(res_host, 2)) if res_host else None,
                              bound=float(mp.log(bound, 2)))
        assert res_dev <= bound, (K, n, mp.nstr(res_dev, 5), mp.nstr(bound, 5))
    if os.environ.get("CLRS_WRITE_PROFILES"):
        path = os.path.join(ROOT, "profiles", "preprocess", "rank_reveal_residuals.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {"what": "log2 of max |G12 - G11 W| / max G_ii per limb count K and size n: device kernel, host elimination at 52 K bits, bound"}
        data["K=%d" % K] = record
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("e,rank", [(100, 3), (140, 2)])
def test_threshold_semantics_on_the_device(e, rank):
    from clrs_amd.mw import rank_reveal, to_limbs
    from clrs_amd.preprocess import detect_limbs, threshold
    D = detect_limbs(256)
    with mp.workprec(52 * D + 64):
        v = [[mp.mpf(1), 0, 0], [0, mp.mpf(1), 0], [mp.mpf(2), mp.mpf(-3), mp.mpf(2) ** -e]]
        G = [[mp.fsum(a * b for a, b in zip(v[i], v[j])) for j in range(3)] for i in range(3)]
        Gl = to_limbs([G[i][j] for j in range(3) for i in range(3)], D)
    perm, r, W, resid = rank_reveal(Gl, [3], [3], [threshold(256, D, 13.0)], D)[0]
    assert r == rank


def _mini(**kw):
    from tests.test_hip_parity import _mini_sdp
    return clrs_amd.flatten(_mini_sdp(**kw))


@pytest.mark.parametrize("K", [5, 6])
@pytest.mark.parametrize("name", ["ce_8_15", "sdpa_small", "threepoint_4", "mini_rank2", "mini_m2"])
def test_constraint_gram_matches_oracle_assembly_at_identity(name, K, oracle_built):
    from clrs_amd.mw import MwSchurContext
    from oracle.oracle import Oracle
    from tests.test_mw_parity import tol
    f = _mini(rank2=True) if name == "mini_rank2" else _mini(m=2) if name == "mini_m2" else flat(name)
    ident = np.zeros((K + 1, f.xy_len))
    for b in range(f.n_blocks):
        n = int(f.block_n[b])
        ident[0, int(f.block_off[b]) + np.arange(n) * (n + 1)] = 1.0
    S_ref, _ = Oracle(f, mp_bits=320 if K <= 5 else 640).schur_assemble_mw(ident, ident)
    ctx = MwSchurContext(f, limbs=K)
    G = ctx.constraint_gram()
    err = mw_relerr(G, S_ref)
    print(name, K, "relative error of G", err)
    assert err <= tol(K, 22), (name, K, err)
    if f.n_free:
        N = f.n_free
        Q = ctx.free_gram()
        B = np.vstack([(f.B + f.B_lo)[int(f.cluster_off[j]) * N:int(f.cluster_off[j + 1]) * N].reshape(-1, N, order="F") for j in range(f.n_clusters)])
        ref = B.T @ B
        assert np.max(np.abs(Q[0].reshape(N, N, order="F") - ref)) <= 1e-12 * np.max(np.abs(ref))
    ctx.close()


def _slacks(f, y, Y):
    from tests.test_preprocess_cpu import slacks
    return slacks(f, y, Y)


SUITE = lindep_suite()


@pytest.mark.parametrize("k", range(10), ids=[s[0] for s in SUITE])
def test_suite_on_the_device(k):
    from clrs_amd.mw import solvesdp_mw
    name, sdp, expect, kw = SUITE[k]
    f = clrs_amd.flatten(sdp)
    if expect is None:
        with pytest.raises(ValueError) as e:
            solvesdp_mw(f, limbs=5, preprocess=True, **kw)
        assert str(e.value) == LINDEP_MESSAGE
        return
    res = solvesdp_mw(f, limbs=5, preprocess=True, **kw)
    assert res.error_code == 0
    print(name, "p_obj", res.primal_objective, "d_obj", res.dual_objective)
    assert abs(res.primal_objective - expect) < 1e-5 and abs(res.dual_objective - expect) < 1e-5
    assert res.x.shape == (5, f.x_len) and res.y.shape == (5, f.n_free)
    assert all(np.all(res.x[:, i] == 0.0) for i, _, _ in res.timings["preprocess"]["cs"])
    s = _slacks(f, res.y[0], res.Y[0])
    print(name, "slack norm", np.linalg.norm(s))
    assert np.linalg.norm(s) < 1e-5


def test_first_suite_problem_fails_without_preprocessing():
    """Today's behaviour, on record for the contrast: a duplicated PSD part makes S_j singular at the first iteration."""
    from clrs_amd.mw import solvesdp_mw
    name, sdp, expect, kw = SUITE[0]
    res = solvesdp_mw(clrs_amd.flatten(sdp), limbs=5, preprocess=False, **kw)
    assert res.error_code == 1


def test_refused_combinations():
    from clrs_amd.mw import MwSchurContext, solvesdp_mw
    f = flat("x2p1")
    ctx = MwSchurContext(f, limbs=5)
    with pytest.raises(ValueError, match="ctx"):
        solvesdp_mw(f, ctx=ctx, preprocess=True)
    ctx.close()
    with pytest.raises(ValueError, match="shard"):
        solvesdp_mw(f, limbs=5, preprocess=True, shard_info=dict())
    g = clrs_amd.flatten(SUITE[0][1])
    warm = type("W", (), dict(x=np.zeros(g.x_len), y=np.zeros(g.n_free), X=np.ones(g.xy_len), Y=np.ones(g.xy_len)))()
    with pytest.raises(ValueError, match="warm start"):
        solvesdp_mw(g, limbs=5, preprocess=True, dualsol=warm, primalsol=warm)


def _planted_case(name, plants, limbs=5):
    """The planted constraints carry coefficients below 1, so that they have the smaller norms and are the ones the pivoting removes: the reduced
    problem is then the unplanted one, row for row.  (With larger coefficients the pivoting keeps the planted combination and removes one of its parts,
    as the reference's column-pivoted QR does; the reduced problem is equivalent but differently scaled, and Nsphere_packing(8, 15, 3 radii), which is at
    the edge of 5 limbs, then ends with a failed factorisation at gap 6e-17, primal error 2e-21 -- measured)"""
    from clrs_amd.mw import solvesdp_mw
    base = instance(name)
    f0 = clrs_amd.flatten(base)
    f1 = clrs_amd.flatten(plant_dependencies(base, plants))
    dup = 1 if f0.n_free else 0          # one duplicated free-variable column where there are free variables
    assert f1.x_len == f0.x_len + len(plants) and f1.n_free == f0.n_free + dup
    a = solvesdp_mw(f0, limbs=limbs)
    b = solvesdp_mw(f1, limbs=limbs, preprocess=True)
    pre = b.timings["preprocess"]
    print(name, "removed", len(pre["cs"]), "free", f1.n_free, "->", pre["n_free"], "preprocess seconds", pre["time"])
    assert len(pre["cs"]) == len(plants)
    assert sorted({j for _, j, _ in pre["cs"]}) == sorted({j for j, _ in plants})
    assert f1.n_free - pre["n_free"] == dup
    assert a.error_code == 0 and b.error_code == 0
    assert b.x.shape[1] == f1.x_len and b.y.shape[1] == f1.n_free
    bound = 2 * (a.duality_gap + b.duality_gap) * max(1.0, abs(a.primal_objective) + abs(a.dual_objective))
    print(name, "objectives", a.primal_objective, b.primal_objective, a.dual_objective, b.dual_objective, "bound", bound)
    assert abs(a.primal_objective - b.primal_objective) <= bound and abs(a.dual_objective - b.dual_objective) <= bound
    c = solvesdp_mw(f1, limbs=limbs, preprocess=False)
    assert c.error_code == 1


def test_planted_dependencies_low_rank_instance():
    # a scaled copy, a genuine combination of two constraints, and a copy in which the sign flips
    _planted_case("ce_8_15", [(0, {0: 0.5}), (0, {1: 0.25, 3: -0.5}), (0, {2: -0.125})])


def test_planted_dependencies_dense_instance():
    _planted_case("sdpa_small", [(0, {0: 0.25}), (0, {1: 0.125, 2: 0.25})])


def test_planted_dependencies_in_clusters_beyond_lds():
    """Nsphere_packing(8, 15, 3 radii): 11 clusters, one of P = 192 -- far beyond LDS at 6 limbs: the global-memory residence of the kernel through the
    context entry point -- beside LDS-resident ones; one dependency planted in the large cluster, one in a cluster of 32."""
    _planted_case("ns_8_15_3", [(1, {0: 0.25, 5: 0.125}), (3, {10: -0.5})])

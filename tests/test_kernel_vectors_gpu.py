"""Kernel vectors of solution blocks on the device (clrs_mw_kernel_vectors: k_mw_rank_reveal, k_mw_kv_scatter, k_mw_gemm, k_mw_kv_colmax): planted blocks at
every limb count against the mpmath elimination of tests/preprocess_host.py, the residuals against `gemm_batch` bit for bit, the vectors against their
restatement from (perm, rank, W), the write discipline, the five problems end to end through `solvesdp_mw`, and the refusals.

Accuracy of the relations inside the vectors (a measurement beside the assertion): max |G12 - G11 W| / max G_ii of the eliminated block at 4 * 52 K bits,
device / host elimination at 52 K bits with the same pivots.  The largest residual per problem of the end-to-end runs goes to
profiles/rounding/kernel_vector_residuals.json when CLRS_WRITE_PROFILES is set."""
import json
import os

import mpmath as mp
import numpy as np
import pytest

from clrs_amd import _lib
from clrs_amd.rounding import RoundingSettings, kernel_vectors, kernel_vectors_batch
from tests import kernel_vectors_util as ku
from tests.preprocess_host import limbs_to_mp, pivoted_cholesky, relation_residual
from tests.test_preprocess_gpu import clear_choices, unambiguous

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1          # CLRS_ERR_INVALID
SENTINEL = -7.25
TAU = 2.0 ** -80      # 2^20 above the planted 2^-100 perturbation; `unambiguous` wants every accepted pivot >= 2^64 TAU = 2^-16
LDS_MAX_N = {4: 49, 5: 44, 6: 40, 8: 35, 10: 31}          # the largest LDS-resident n of k_mw_rank_reveal (MW_RANK_LDS)


def shapes(K):
    m = LDS_MAX_N[K]
    return [(1, 0), (1, 1), (5, 2), (16, 16), (17, 0), (33, 7), (m, 3), (m + 1, 3)]


def planted_instances(K):
    """per shape the first seed whose pair is unambiguous for BOTH eliminations (of X and of Y): [(n, r, X, Y, {branch: (perm, rank)})]"""
    bits = 4 * 52 * K
    out = []
    for n, r in shapes(K):
        for seed in range(40):
            X, Y = ku.planted_pair(n, r, K, 1000 * n + 10 * r + seed)
            host = {}
            for branch, planes in (("dual", X), ("primal", Y)):
                with mp.workprec(bits):                     # (the helpers copy G with mp.mpf(v): exact only under this precision)
                    G = ku.block_mp(planes, n)
                    h = unambiguous(G, n, TAU, bits)
                    if h is None or not clear_choices(G, n, h[0][:h[1]], bits):
                        break
                host[branch] = (G, h[0], h[1])
            if len(host) == 2:
                break
        else:
            raise AssertionError(("no unambiguous instance", n, r))
        # the planted ranks, not a matter of rounding (smallest accepted pivot >= 2^64 TAU at 4 * 52 K bits)
        assert host["dual"][2] == r and host["primal"][2] == n - r, (n, r, host["dual"][2], host["primal"][2])
        out.append((n, r, X, Y, host))
    return out


@pytest.mark.parametrize("K", ku.LIMBS)
def test_planted_blocks_both_branches(K):
    from clrs_amd.mw import gemm_batch, rank_reveal
    bits = 4 * 52 * K
    inst = planted_instances(K)
    ns = [i[0] for i in inst]
    Xp, Yp = (np.ascontiguousarray(np.concatenate([i[k] for i in inst], axis=1)) for k in (2, 3))
    off = np.concatenate([[0], np.cumsum(np.array(ns, dtype=np.int64) ** 2)])
    for branch in ("dual", "primal"):
        V = np.full((K, int(off[-1])), SENTINEL)
        out = kernel_vectors_batch(ns, Xp, Yp, K, TAU, branch == "dual", float("inf"), V=V)
        # the same elimination by the kernel's own entry point: (perm, rank, W) for the restatement of the scatter
        Ep = Xp if branch == "dual" else Yp
        rr = rank_reveal(Ep, ns, ns, [TAU] * len(ns), K)
        for b, ((n, r0, X, Y, host), k, (dperm, dr, dW, dres)) in enumerate(zip(inst, out, rr)):
            G, hperm, hr = host[branch]
            count = hr if branch == "dual" else n - hr
            assert k.branch == branch and k.rank == hr and k.count == count, (K, branch, n, k.rank, hr)
            assert list(k.perm) == list(hperm), (K, branch, n, list(k.perm), hperm)
            assert k.count == r0                                                    # both branches: rank X vectors
            assert k.rank == dr and list(k.perm) == list(dperm)
            # the scattered vectors are the restatement from (perm, r, W), entry for entry, and nothing else of V was written
            Wd = np.transpose(dW.reshape(K, n - dr, dr), (0, 2, 1))
            want = ku.restate_vectors(branch, list(dperm), dr, Wd)
            assert k.vectors.shape == want.shape == (K, n, count)
            assert np.array_equal(k.vectors, want), (K, branch, n)
            blk = V[:, off[b]:off[b + 1]]
            assert np.array_equal(blk[:, :n * count].reshape(K, count, n).transpose(0, 2, 1), k.vectors)
            assert np.all(blk[:, n * count:] == SENTINEL), (K, branch, n, "V written outside n x count")
            assert np.array_equal(k.pivot_resid, dres)
            # relations: against the host elimination at 52 K bits with the same pivots (the yardstick of test_preprocess_gpu.py)
            with mp.workprec(bits):
                w = limbs_to_mp(ku.w_of_vectors(branch, list(k.perm), hr, k.vectors).transpose(0, 2, 1).reshape(K, -1)) if hr * (n - hr) else []
                Wm = [[w[c + a * hr] for a in range(n - hr)] for c in range(hr)]
                res_dev = relation_residual(G, list(k.perm), hr, Wm, bits)
            _, _, Wh, _, _ = pivoted_cholesky(G, n, TAU, 52 * K, order=list(hperm[:hr]))
            res_host = relation_residual(G, list(hperm), hr, Wh, bits)
            bound = max(64 * res_host, mp.mpf(2) ** -(52 * K))
            print("K", K, branch, "n", n, "rank", hr, "vectors", count, "relation residual device", mp.nstr(res_dev, 5), "host", mp.nstr(res_host, 5), "bound",
                  mp.nstr(bound, 5), "max resid_max", float(np.max(k.resid_max)) if count else 0.0)
            assert res_dev <= bound, (K, branch, n, mp.nstr(res_dev, 5), mp.nstr(bound, 5))
            # residuals: the heads of gemm_batch(Y_b, V_b) on the returned planes, bit for bit, and below the reference's bound
            if count:
                Yb = np.transpose(Y.reshape(K, n, n), (0, 2, 1))
                R = gemm_batch([(Yb, k.vectors, None, 0, 0, 1, 0)], K)[0]
                assert np.array_equal(k.resid_max, np.max(np.abs(R[0]), axis=0)), (K, branch, n)
                assert np.array_equal(k.v_max, np.max(np.abs(k.vectors[0]), axis=0))
                assert np.all(k.resid_max < 1e-10), (K, branch, n, float(np.max(k.resid_max)))
            else:
                assert k.resid_max.size == 0 and k.v_max.size == 0


@pytest.fixture(scope="module")
def residual_record():
    rec = {}
    yield rec
    if os.environ.get("CLRS_WRITE_PROFILES") and rec:
        path = os.path.join(ROOT, "profiles", "rounding", "kernel_vector_residuals.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump({"what": "largest max_i |head (Y_b v)_i| over the kernel vectors of solvesdp_mw(limbs=5, duality_gap_threshold=1e-30), per problem and branch",
                   **rec}, open(path, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("name", list(ku.RANKS))
def test_end_to_end_on_the_five_problems(name, residual_record):
    from clrs_amd.mw import solvesdp_mw
    f = ku.problem(name)
    res = solvesdp_mw(f, limbs=5, duality_gap_threshold=1e-30)
    # (how the solve ended is not this test's subject: cohnelkies(8, 3) stops at gap 4e-29 at 5 limbs with a failed factorisation; the iterate is what is examined)
    print(name, "solve:", res.status, "error code", res.error_code, "gap", res.duality_gap)
    dual = kernel_vectors(f, res, res, check_dimensions=True)
    primal = kernel_vectors(f, res, settings=RoundingSettings(kernel_use_dual=False), check_dimensions=True)
    worst = {tag: max([float(np.max(k.resid_max)) for k in ks if k.count] + [0.0]) for tag, ks in (("dual", dual), ("primal", primal))}
    print(name, "largest residual", worst)
    residual_record[name] = dict(worst, status=res.status, duality_gap=float(res.duality_gap))
    assert all(k.branch == "dual" for k in dual) and all(k.branch == "primal" for k in primal)
    assert [k.count for k in dual] == ku.RANKS[name]
    assert [k.count for k in primal] == [k.count for k in dual]
    assert all(k.vectors.shape == (5, int(n), k.count) for ks in (dual, primal) for k, n in zip(ks, f.block_n))
    assert all(np.all(k.resid_max < 1e-10) for ks in (dual, primal) for k in ks)


def test_refusals_leave_the_library_usable():
    L = _lib.load()
    K = 5
    ns = [5, 1]
    X0, Y0 = ku.planted_pair(5, 2, K, 7)
    X1, Y1 = ku.planted_pair(1, 1, K, 8)
    X, Y = (np.ascontiguousarray(np.concatenate(p, axis=1)) for p in ((X0, X1), (Y0, Y1)))
    good = kernel_vectors_batch(ns, X, Y, K, TAU, True, float("inf"))
    assert [k.count for k in good] == [2, 1]
    n = np.array(ns, np.int32)
    bufs = dict(branch=np.zeros(2, np.int32), perm=np.zeros(6, np.int32), rank=np.zeros(2, np.int32), count=np.zeros(2, np.int32), V=np.zeros((K, 26)),
                resid_max=np.zeros(6), v_max=np.zeros(6), pivot_resid=np.zeros((K, 6)))

    def call(limbs=K, nblk=2, n=n, X=X, Y=Y, plane=26, tau=TAU, null=None):
        p = lambda a: None if a is None else a.ctypes.data_as(_lib.p_i32 if a.dtype == np.int32 else _lib.p_d)
        o = {k: (None if k == null else v) for k, v in bufs.items()}
        return L.clrs_mw_kernel_vectors(0, limbs, nblk, p(n), p(None if null == "X" else X), p(None if null == "Y" else Y), plane, tau, 1, float("inf"),
                                        p(o["branch"]), p(o["perm"]), p(o["rank"]), p(o["count"]), p(o["V"]), p(o["resid_max"]), p(o["v_max"]), p(o["pivot_resid"]))
    refused = [("limbs = 3", dict(limbs=3)), ("limbs = 7", dict(limbs=7)), ("negative block count", dict(nblk=-1)), ("negative size", dict(n=np.array([5, -1], np.int32))),
               ("negative plane", dict(plane=-1)), ("blocks leave the plane", dict(plane=25)), ("tau = 0", dict(tau=0.0)), ("tau < 0", dict(tau=-1e-10)),
               ("tau NaN", dict(tau=float("nan"))), ("n null", dict(n=None))]
    refused += [(name + " null", dict(null=name)) for name in ("X", "Y", *bufs)]
    for what, kw in refused:
        assert call(**kw) == INVALID, what
        assert L.clrs_last_error(), what
        assert all(np.all(v == 0) for v in bufs.values()), what                  # nothing was written
    # the next valid call still works
    assert call() == 0
    again = kernel_vectors_batch(ns, X, Y, K, TAU, True, float("inf"))
    assert list(bufs["count"]) == [2, 1] and list(bufs["rank"]) == [k.rank for k in good]
    assert all(np.array_equal(a.vectors, b.vectors) and np.array_equal(a.resid_max, b.resid_max) for a, b in zip(good, again))

"""Rounding kernel vectors to rationals on the device (k_mw_rationalize; clrs_mw_rationalize, clrs_mw_kernel_vectors_rational): the kernel against the host
build of the same function with ==, the write discipline, the refusals, planted pairs whose exact echelon vectors are known from their integer matrices, the
existing entry against the new one bit for bit in what they share, and delsarte_exact(8, 3, 1/2) end to end through `solvesdp_mw`."""
from fractions import Fraction

import numpy as np
import pytest

from clrs_amd import _lib
from clrs_amd.rounding import (RoundingSettings, kernel_vectors, kernel_vectors_batch, kernel_vectors_rational_batch, rationalize,
                               vectors_to_fractions)
from tests import rationalize_util as ru

pytestmark = pytest.mark.gpu

INVALID = -1          # CLRS_ERR_INVALID
SENTINEL = -7.25
ISENTINEL = -77
TAU = 2.0 ** -80
LDS_MAX_N = {4: 49, 5: 44, 6: 40, 8: 35, 10: 31}          # the largest LDS-resident n of k_mw_rank_reveal
COMMON_SHAPES = [(1, 0), (1, 1), (5, 2), (16, 16), (17, 0), (33, 7)]
SEED = 1


def shapes(K):
    m = LDS_MAX_N[K]
    return COMMON_SHAPES + [(m, 3), (m + 1, 3)]


def _pd(a):
    return None if a is None else a.ctypes.data_as(_lib.p_i32 if a.dtype == np.int32 else _lib.p_d)


@pytest.mark.parametrize("K", ru.LIMBS)
def test_kernel_against_the_host_build(K):
    L = _lib.load()
    for count in (1, 63, 65, 2049):
        v = ru.drawn_pool(K, count, seed=100 * K + count % 97)
        want = ru.host_rationalize(v, K)
        assert set(int(s) for s in want[2]) == {0, 1, 2} or count < 63                 # every status occurs in the larger pools
        plane = count + 5                                                              # five sentinels behind every plane
        vin = np.full((K, plane), 1.0 / 3)
        vin[:, :count] = v
        num, den, status, vq = np.full(plane, SENTINEL), np.full(plane, SENTINEL), np.full(plane, ISENTINEL, np.int32), np.full((K, plane), SENTINEL)
        assert L.clrs_mw_rationalize(0, K, count, _pd(vin), plane, ru.EPS, _pd(num), _pd(den), _pd(status), _pd(vq)) == 0
        assert np.array_equal(num[:count], want[0]) and np.array_equal(den[:count], want[1]) and np.array_equal(status[:count], want[2]), (K, count)
        assert np.array_equal(vq[:, :count], want[3]), (K, count)
        assert np.all(num[count:] == SENTINEL) and np.all(den[count:] == SENTINEL) and np.all(status[count:] == ISENTINEL) and np.all(vq[:, count:] == SENTINEL)
        got = rationalize(v, K)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (K, count)
    # errbound = 1e-40 where the arithmetic carries it: the irrationals run into the cap
    if K == 10:
        v = dict(ru.input_classes(10, 1))["irrational"]
        got, want = rationalize(v, 10, errbound=1e-40), ru.host_rationalize(v, 10, 1e-40)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and list(got[2]) == [1, 1, 1]
    assert all(a.size == 0 for a in rationalize(np.zeros((K, 0)), K)[:3])


def test_refusals_of_rationalize_leave_the_library_usable():
    L = _lib.load()
    K, count, plane = 5, 3, 4
    v = np.zeros((K, plane))
    v[0, :count] = [0.5, -0.25, 3.0]
    bufs = dict(num=np.zeros(plane), den=np.zeros(plane), status=np.zeros(plane, np.int32), vq=np.zeros((K, plane)))

    def call(limbs=K, count=count, v=v, plane=plane, errbound=1e-15, null=None):
        o = {k: (None if k == null else a) for k, a in bufs.items()}
        return L.clrs_mw_rationalize(0, limbs, count, _pd(None if null == "v" else v), plane, errbound, _pd(o["num"]), _pd(o["den"]), _pd(o["status"]), _pd(o["vq"]))
    refused = [("limbs = 3", dict(limbs=3)), ("limbs = 7", dict(limbs=7)), ("limbs = 12", dict(limbs=12)), ("count < 0", dict(count=-1)),
               ("plane < count", dict(plane=2)), ("errbound = 0", dict(errbound=0.0)), ("errbound < 0", dict(errbound=-1e-15)),
               ("errbound NaN", dict(errbound=float("nan")))]
    refused += [(name + " null", dict(null=name)) for name in ("v", *bufs)]
    for what, kw in refused:
        assert call(**kw) == INVALID, what
        assert L.clrs_last_error(), what
        assert all(np.all(a == 0) for a in bufs.values()), what                       # nothing was written
    assert call(count=0, null="v") == 0                                                # count = 0: nothing to point at
    assert call() == 0
    assert list(bufs["num"]) == [1.0, -1.0, 3.0, 0.0] and list(bufs["den"]) == [2.0, 4.0, 1.0, 0.0] and list(bufs["status"]) == [0, 0, 0, 0]
    # the round_errbound of the combined entry is checked alike
    X = np.zeros((K, 1)); X[0, 0] = 1.0
    with pytest.raises(_lib.ClrsError, match="round_errbound"):
        kernel_vectors_rational_batch([1], X, np.zeros((K, 1)), K, TAU, True, float("inf"), 0.0)
    with pytest.raises(_lib.ClrsError, match="round_errbound"):
        kernel_vectors_rational_batch([1], X, np.zeros((K, 1)), K, TAU, True, float("inf"), float("nan"))


@pytest.fixture(scope="module")
def planted_runs():
    """K -> branch -> [(n, r, X0 or Y0 (the integer matrix that was eliminated), Y planes, BlockKernel)] and the pools of the call: one device call per
    limb count and branch over all shapes, computed once"""
    runs = {}
    for K in ru.LIMBS:
        inst = [(n, r) + ru.planted_pair_exact(n, r, K, SEED) for n, r in shapes(K)]
        ns = [i[0] for i in inst]
        Xp, Yp = (np.ascontiguousarray(np.concatenate([i[k] for i in inst], axis=1)) for k in (2, 3))
        plane = Xp.shape[1]
        runs[K] = {}
        for branch in ("dual", "primal"):
            V = np.full((K, plane), SENTINEL)
            rounded = (np.full(plane, SENTINEL), np.full(plane, SENTINEL), np.full(plane, ISENTINEL, np.int32), np.full((K, plane), SENTINEL))
            out = kernel_vectors_rational_batch(ns, Xp, Yp, K, TAU, branch == "dual", float("inf"), ru.EPS, V=V, rounded=rounded)
            runs[K][branch] = dict(blocks=[(n, r, X0 if branch == "dual" else Y0, Y, k) for (n, r, X, Y, X0, Y0), k in zip(inst, out)], V=V, rounded=rounded,
                                   ns=ns, X=Xp, Y=Yp)
    return runs


@pytest.mark.parametrize("branch", ["dual", "primal"])
@pytest.mark.parametrize("K", ru.LIMBS)
def test_planted_pairs_round_to_their_exact_echelon_vectors(K, branch, planted_runs):
    from clrs_amd.mw import gemm_batch
    run = planted_runs[K][branch]
    off, worst_den, jobs = 0, 0, []
    for n, r, A0, Y, k in run["blocks"]:
        assert k.branch == branch and k.count == r and k.rank == (r if branch == "dual" else n - r), (K, branch, n, r, k.rank)
        assert k.num.shape == k.den.shape == k.round_status.shape == (n, r) and k.vectors_rounded.shape == (K, n, r) and k.round_resid_max.shape == (r,)
        assert np.all(k.round_status == 0), (K, branch, n, r)
        # == the exact echelon vectors over the returned pivots, from the integer matrix
        want = ru.exact_echelon_vectors(A0, branch, k.perm, k.rank)
        got = vectors_to_fractions(k)
        assert got == [[want[i][v] for i in range(n)] for v in range(r)], (K, branch, n, r)
        worst_den = max(worst_den, k.max_den)
        # == the host build on the returned vectors: num, den, status and num / den in K limbs
        flat = np.ascontiguousarray(np.transpose(k.vectors, (0, 2, 1)).reshape(K, -1))
        hnum, hden, hst, hvq = ru.host_rationalize(flat, K)
        assert np.array_equal(k.num.T.reshape(-1), hnum) and np.array_equal(k.den.T.reshape(-1), hden) and np.array_equal(k.round_status.T.reshape(-1), hst)
        assert np.array_equal(np.transpose(k.vectors_rounded, (0, 2, 1)).reshape(K, -1), hvq), (K, branch, n, r)
        # nothing outside n x count was written, in any of the pools
        blk = slice(off + n * r, off + n * n)
        num, den, status, Vq = run["rounded"]
        assert np.all(num[blk] == SENTINEL) and np.all(den[blk] == SENTINEL) and np.all(status[blk] == ISENTINEL) and np.all(Vq[:, blk] == SENTINEL)
        assert np.all(run["V"][:, blk] == SENTINEL)
        off += n * n
        if r:
            jobs.append((np.transpose(Y.reshape(K, n, n), (0, 2, 1)), k.vectors_rounded, None, 0, 0, 1, 0))
    # the second residual: the heads of gemm_batch(Y_b, Vq_b), bit for bit; exact vectors of exact blocks plus 2^-100 noise: far below the bound
    R = gemm_batch(jobs, K)
    for (n, r, A0, Y, k), Rb in zip([b for b in run["blocks"] if b[1]], R):
        assert np.array_equal(k.round_resid_max, np.max(np.abs(Rb[0]), axis=0)), (K, branch, n, r)
        assert np.all(k.round_resid_max < 1e-10)
    print("K", K, branch, "largest denominator", worst_den)


def test_planted_pairs_give_the_same_rationals_at_every_limb_count(planted_runs):
    for branch in ("dual", "primal"):
        ref = planted_runs[ru.LIMBS[0]][branch]["blocks"]
        for K in ru.LIMBS[1:]:
            for (n, r, _, _, k0), (n2, r2, _, _, k) in zip(ref[:len(COMMON_SHAPES)], planted_runs[K][branch]["blocks"][:len(COMMON_SHAPES)]):
                assert (n, r) == (n2, r2)
                assert np.array_equal(k0.num, k.num) and np.array_equal(k0.den, k.den), (K, branch, n, r)


@pytest.mark.parametrize("K", ru.LIMBS)
def test_existing_entry_returns_the_shared_outputs_bit_for_bit(K, planted_runs):
    for branch in ("dual", "primal"):
        run = planted_runs[K][branch]
        V = np.full_like(run["V"], SENTINEL)
        old = kernel_vectors_batch(run["ns"], run["X"], run["Y"], K, TAU, branch == "dual", float("inf"), V=V)
        assert np.array_equal(V, run["V"])
        for a, (_, _, _, _, b) in zip(old, run["blocks"]):
            assert (a.branch, a.rank, a.count) == (b.branch, b.rank, b.count) and np.array_equal(a.perm, b.perm)
            assert np.array_equal(a.vectors, b.vectors) and np.array_equal(a.resid_max, b.resid_max) and np.array_equal(a.v_max, b.v_max)
            assert np.array_equal(a.pivot_resid, b.pivot_resid)
            assert a.num is None and a.round_resid_max is None


def test_end_to_end_delsarte_exact():
    """solvesdp_mw on delsarte_exact(8, 3, 1/2) at 10 limbs to the reference's gap of 1e-40, then the kernel with the rounding on the device: 240, the
    reference's own test value; a_0, A and B have 1, 4 and 2 vectors with entries 0 and +-1."""
    import clrs_amd
    from clrs_amd import problems as P
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    with data_planes(10):                                      # the sampled problem at the working precision (two limb planes describe a neighbouring
        f = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5, prec=640))    # problem: its optimum is 2e-30 away from 240, measured)
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    print("delsarte_exact(8, 3, 1/2) at 10 limbs:", res.status, "error code", res.error_code, "iterations", res.iterations, "gap", res.duality_gap,
          "objectives", res.primal_objective, res.dual_objective)
    assert res.error_code == 0 and res.status == "Optimal", (res.status, res.error_code, res.duality_gap)
    d_obj, p_obj = (ru.exact_value(res.timings["objectives_limbs"][i]) for i in (0, 1))                # the objectives at the working precision
    print("objectives - 240:", float(d_obj - 240), float(p_obj - 240))
    assert abs(d_obj - 240) <= Fraction(1e-30) and abs(p_obj - 240) <= Fraction(1e-30)
    for settings in (RoundingSettings(), RoundingSettings(kernel_use_dual=False)):
        blocks = kernel_vectors(f, res, res, settings=settings, check_dimensions=True, rationalize=True)
        assert all(k.branch == ("dual" if settings.kernel_use_dual else "primal") for k in blocks)
        assert all(k.vectors.shape[0] == 10 for k in blocks)
        ru.check_delsarte_exact_kernel(blocks)
        print("branch", blocks[0].branch, "largest residual before / after rounding", max(float(np.max(k.resid_max)) for k in blocks if k.count),
              max(float(np.max(k.round_resid_max)) for k in blocks if k.count))

"""The batched multi-word product on the device (clrs_mw_gemm, k_mw_gemm) against its host restatement (bit for bit) and mpmath (within the bound of
tests/mw_gemm_util.py), its write discipline and refusals, and preprocess / solvesdp_mw with the substitution on the device."""
import ctypes as C

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib
from clrs_amd.preprocess import LINDEP_MESSAGE, DeviceReveal, detect_limbs, preprocess
from clrs_amd.problems.toy import lindep_suite
from tests import mw_gemm_util as gu
from tests.preprocess_host import plant_dependencies
from tests.util import instance

pytestmark = pytest.mark.gpu
SUITE = lindep_suite()
INVALID = -1          # CLRS_ERR_INVALID


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("K", gu.LIMBS)
def test_job_list_is_the_host_restatement_bit_for_bit_and_within_the_bound(K):
    """The same operation order, every operation an IEEE add, multiply or fma, contraction off: the device result IS the host loop's.  The pools'
    padding (C: a sentinel, checked by `check`; A, B: NaN, which would spread) is neither written nor read."""
    b = gu.issue_batch(K)
    dev, host = gu.run_device(b), gu.run_host(b)
    diff = np.argwhere(dev.view(np.uint64) != host.view(np.uint64))
    print("K", K, "entries that differ from the host restatement:", len(diff), diff[:5].tolist())
    assert len(diff) == 0
    print("K", K, "worst error / bound", b.check(dev))


@pytest.mark.parametrize("K", gu.LIMBS)
def test_inner_product_that_cancels(K):
    b = gu.cancel_batch(K)
    dev = gu.run_device(b)
    assert _same_bits(dev, gu.run_host(b))
    print("K", K, "worst error / bound", b.check(dev))


def test_beta_zero_never_reads_c():
    """C full of NaN (the padding rows keep their sentinel) under beta = 0: a finite, correct result, identical to the one over a clean C."""
    K = 5
    b = gu.Batch(K, ((17, 15, 7, 0, 0, 1, 0), (16, 33, 20, 1, 1, -1, 0)), seed=77)
    A, B, Cp = b.pools()
    clean = gu.run_device(b)
    Cp[Cp != gu.SENTINEL] = np.nan
    _lib.check(_lib.load().clrs_mw_gemm(0, K, len(b.shapes), b.table, A.ctypes.data_as(_lib.p_d), A.shape[1], B.ctypes.data_as(_lib.p_d), B.shape[1],
                                        Cp.ctypes.data_as(_lib.p_d), Cp.shape[1]))
    assert np.all(np.isfinite(Cp)) and _same_bits(Cp, clean)
    b.check(Cp)


@pytest.mark.parametrize("K", (5, 10))
def test_gram_matrix_on_one_pool_is_symmetric_bit_for_bit(K):
    rng = np.random.default_rng(19 + K)
    m, n = 19, 23
    A = gu.to_limbs(gu.rand_values(rng, m * n, K), K)                   # 19 x 23 column-major
    job = (_lib.MwGemmJob * 1)(_lib.MwGemmJob(n, n, m, 1, 0, 1, 0, m, m, n, 0, 0, 0))
    G = np.zeros((K, n * n))
    _lib.check(_lib.load().clrs_mw_gemm(0, K, 1, job, A.ctypes.data_as(_lib.p_d), A.shape[1], A.ctypes.data_as(_lib.p_d), A.shape[1],
                                        G.ctypes.data_as(_lib.p_d), G.shape[1]))
    G = G.reshape(K, n, n)
    assert np.all(G[0].diagonal() > 0) and _same_bits(G, np.ascontiguousarray(np.transpose(G, (0, 2, 1))))


def test_refusals_leave_the_library_usable():
    L = _lib.load()
    K = 4
    b = gu.Batch(K, ((5, 4, 3, 0, 0, 1, 0), (4, 5, 3, 1, 0, 1, 1)), seed=3)
    A, B, Cp = b.pools()

    def call(limbs, table):
        return L.clrs_mw_gemm(0, limbs, len(table), table, A.ctypes.data_as(_lib.p_d), A.shape[1], B.ctypes.data_as(_lib.p_d), B.shape[1],
                              Cp.ctypes.data_as(_lib.p_d), Cp.shape[1])

    def edited(**kw):
        t = (_lib.MwGemmJob * len(b.shapes))()
        C.memmove(t, b.table, C.sizeof(t))
        for k, v in kw.items():
            setattr(t[0], k, v)
        return t
    before = Cp.copy()
    for what, rc in (("limbs = 3", call(3, b.table)), ("alpha = 2", call(K, edited(alpha=2))), ("lda < rows", call(K, edited(lda=4))),
                     ("overlapping C", call(K, edited(c_off=int(b.table[1].c_off) + 1)))):
        assert rc == INVALID, what
        assert L.clrs_last_error(), what
        assert _same_bits(Cp, before), what
        assert call(K, b.table) == 0, what                                 # a correct call afterwards succeeds
        b.check(Cp)
        Cp[:] = before


def test_gemm_batch_matches_the_host_restatement():
    """mw.gemm_batch (operands as (planes, rows, cols), zero padded to the limb count, one call per list) on shapes of the substitution"""
    from clrs_amd.mw import gemm_batch
    K = 6
    rng = np.random.default_rng(5)

    def planes(p, r, c):
        return np.transpose(gu.to_limbs(gu.rand_values(rng, r * c, p), p).reshape(p, c, r), (0, 2, 1))
    W, Bk, Br, M = planes(6, 7, 3), planes(2, 7, 5), planes(2, 3, 5), planes(6, 20, 5)
    got = gemm_batch([(W, Bk, Br, 1, 0, -1, 1), (M, M, None, 1, 0, 1, 0)], K)
    assert [g.shape for g in got] == [(K, 3, 5), (K, 5, 5)]

    def cm(x):       # (p, r, c) -> planar column-major (K, r * c)
        return np.pad(np.transpose(x, (0, 2, 1)).reshape(x.shape[0], -1), ((0, K - x.shape[0]), (0, 0)))
    AB = np.ascontiguousarray(np.concatenate([cm(W), cm(Bk), cm(M)], axis=1))
    Cp = np.ascontiguousarray(np.concatenate([cm(Br), np.zeros((K, 25))], axis=1))
    table = (_lib.MwGemmJob * 2)(_lib.MwGemmJob(3, 5, 7, 1, 0, -1, 1, 7, 7, 3, 0, 21, 0), _lib.MwGemmJob(5, 5, 20, 1, 0, 1, 0, 20, 20, 5, 56, 56, 15))
    assert gu.host_lib().mw_gemm_host(K, 2, table, AB.ctypes.data_as(_lib.p_d), AB.shape[1], AB.ctypes.data_as(_lib.p_d), AB.shape[1],
                                      Cp.ctypes.data_as(_lib.p_d), Cp.shape[1]) == 0
    assert _same_bits(cm(got[0]), np.ascontiguousarray(Cp[:, :15])) and _same_bits(cm(got[1]), np.ascontiguousarray(Cp[:, 15:]))


# ---- solvesdp_mw(preprocess=True, preprocess_substitute="device") ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(10), ids=[s[0] for s in SUITE])
def test_suite_with_the_substitution_on_the_device(k):
    """the assertions of test_preprocess_gpu.py::test_suite_on_the_device, and the iteration count of the "host" run of the same instance"""
    from clrs_amd.mw import solvesdp_mw
    from tests.test_preprocess_cpu import slacks
    name, sdp, expect, kw = SUITE[k]
    f = clrs_amd.flatten(sdp)
    if expect is None:
        with pytest.raises(ValueError) as e:
            solvesdp_mw(f, limbs=5, preprocess=True, preprocess_substitute="device", **kw)
        assert str(e.value) == LINDEP_MESSAGE
        return
    res = solvesdp_mw(f, limbs=5, preprocess=True, preprocess_substitute="device", **kw)
    assert res.error_code == 0
    print(name, "p_obj", res.primal_objective, "d_obj", res.dual_objective)
    assert abs(res.primal_objective - expect) < 1e-5 and abs(res.dual_objective - expect) < 1e-5
    assert res.x.shape == (5, f.x_len) and res.y.shape == (5, f.n_free)
    assert all(np.all(res.x[:, i] == 0.0) for i, _, _ in res.timings["preprocess"]["cs"])
    s = slacks(f, res.y[0], res.Y[0])
    print(name, "slack norm", np.linalg.norm(s))
    assert np.linalg.norm(s) < 1e-5
    host = solvesdp_mw(f, limbs=5, preprocess=True, **kw)
    assert host.error_code == 0 and res.iterations == host.iterations


PLANTED = {"ce_8_15": gu.PLANTS_CE, "sdpa_small": [(0, {0: 0.25}), (0, {1: 0.125, 2: 0.25})], "ns_8_15_3": [(1, {0: 0.25, 5: 0.125}), (3, {10: -0.5})]}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_dependencies_with_the_substitution_on_the_device(name):
    """the assertions of test_preprocess_gpu.py::_planted_case at 5 limbs with the plants of the tests there, and the "host" run's iteration count"""
    from clrs_amd.mw import solvesdp_mw
    plants, limbs = PLANTED[name], 5
    base = instance(name)
    f0 = clrs_amd.flatten(base)
    f1 = clrs_amd.flatten(plant_dependencies(base, plants))
    dup = 1 if f0.n_free else 0
    assert f1.x_len == f0.x_len + len(plants) and f1.n_free == f0.n_free + dup
    a = solvesdp_mw(f0, limbs=limbs)
    b = solvesdp_mw(f1, limbs=limbs, preprocess=True, preprocess_substitute="device")
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
    h = solvesdp_mw(f1, limbs=limbs, preprocess=True)
    print(name, "iterations: device substitution", b.iterations, "host substitution", h.iterations, "host preprocess seconds", h.timings["preprocess"]["time"])
    assert h.error_code == 0 and b.iterations == h.iterations


def test_reduced_problem_of_both_substitutions_through_the_device():
    f = clrs_amd.flatten(plant_dependencies(instance("ce_8_15"), gu.PLANTS_CE))
    host, dev = preprocess(f, reveal=DeviceReveal), preprocess(f, reveal=DeviceReveal, substitute="device")
    assert len(dev[1]) == len(gu.PLANTS_CE) and dev[0].n_free == f.n_free - 1
    print("worst difference / (2 x bound)", gu.assert_same_reduction(f, host, dev, detect_limbs(256)))

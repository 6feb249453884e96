"""CPU side of the batched multi-word product (clrs_mw_gemm, csrc/clrs_mw_gemm.hip.h) and of preprocess(substitute="device"):
the kernel's entry functions compiled for the host against mpmath, the binding, and the substitution on limb planes driven by a host stand-in
of `gemm_batch` (the package has no CPU implementation of it)."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib
from clrs_amd import preprocess as pre
from clrs_amd.mw import to_limbs
from clrs_amd.preprocess import LINDEP_MESSAGE, detect_limbs, preprocess
from clrs_amd.problems.toy import lindep_suite
from tests import mw_gemm_util as gu
from tests.preprocess_host import HostReveal, limbs_to_mp, plant_dependencies
from tests.util import instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = lindep_suite()


@pytest.mark.parametrize("K", gu.LIMBS)
def test_host_restatement_against_mpmath(K):
    """The entry functions the kernel calls, looped on the host over the issue's job list: every entry within the bound, padding rows of C untouched,
    padding rows of A and B (NaN) never read."""
    worst = gu.issue_batch(K).check(gu.run_host(gu.issue_batch(K)))
    print("K", K, "worst error / bound", worst)


@pytest.mark.parametrize("K", gu.LIMBS)
def test_host_restatement_under_cancellation(K):
    worst = gu.cancel_batch(K).check(gu.run_host(gu.cancel_batch(K)))
    print("K", K, "worst error / bound", worst)


def test_lib_binds_clrs_mw_gemm_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    ret, args = re.search(r"^\s*(\w+)\s+clrs_mw_gemm\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    table = {"int": C.c_int, "int64_t": C.c_int64, "const double *": _lib.p_d, "double *": _lib.p_d, "const clrs_mw_gemm_job *": C.POINTER(_lib.MwGemmJob)}
    want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
    assert ret == "int" and _lib.SYMBOLS["clrs_mw_gemm"] == (C.c_int, want)
    body = re.search(r"typedef struct clrs_mw_gemm_job \{(.*?)\} clrs_mw_gemm_job;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.strip().split(None, 1)
            fields += [(nm.strip(), {"int32_t": C.c_int32, "int64_t": C.c_int64}[typ]) for nm in names.split(",")]
    assert fields == list(_lib.MwGemmJob._fields_) and C.sizeof(_lib.MwGemmJob) == 64
    from clrs_amd import mw
    assert callable(mw.gemm_batch)


class HostGemmReveal(HostReveal):
    """HostReveal plus `gemm_batch` in mpmath: the exact value of every entry, rounded to D planes."""

    def gemm_batch(self, jobs):
        out = []
        with mp.workprec(64 * self.D + 1200):
            for A, B, Cm, ta, tb, alpha, beta in jobs:
                def vals(M):
                    M = np.asarray(M, dtype=np.float64)
                    return np.array(limbs_to_mp(M.reshape(M.shape[0], -1)), dtype=object).reshape(M.shape[1:])
                a, b = vals(A), vals(B)
                a, b = (a.T if ta else a), (b.T if tb else b)
                m, n = a.shape[0], b.shape[1]
                c = vals(Cm) if beta else None
                ex = [alpha * mp.fsum(a[i, r] * b[r, j] for r in range(a.shape[1])) + (beta * c[i, j] if beta else 0) for i in range(m) for j in range(n)]
                out.append(to_limbs(ex, self.D).reshape(self.D, m, n) if m * n else np.zeros((self.D, m, n)))
        return out


def _both(f, **kw):
    return preprocess(f, reveal=HostReveal, **kw), preprocess(f, reveal=HostGemmReveal, substitute="device", **kw)


@pytest.mark.parametrize("k", range(10), ids=[s[0] for s in SUITE])
def test_device_substitution_matches_host_on_the_suite(k):
    name, sdp, expect, kw = SUITE[k]
    f = clrs_amd.flatten(sdp)
    if expect is None:
        for sub, rv in (("host", HostReveal), ("device", HostGemmReveal)):
            with pytest.raises(ValueError) as e:
                preprocess(f, reveal=rv, substitute=sub)
            assert str(e.value) == LINDEP_MESSAGE
        return
    host, dev = _both(f)
    print(name, "worst difference / (2 x bound)", gu.assert_same_reduction(f, host, dev, detect_limbs(256)))


@pytest.fixture(scope="module")
def planted_ce():
    return plant_dependencies(instance("ce_8_15"), gu.PLANTS_CE)


def test_device_substitution_matches_host_on_planted_instance(planted_ce):
    f = clrs_amd.flatten(planted_ce)
    host, dev = _both(f)
    assert len(host[1]) == len(gu.PLANTS_CE) and host[0].n_free == f.n_free - 1
    print("worst difference / (2 x bound)", gu.assert_same_reduction(f, host, dev, detect_limbs(256)))


def test_substitute_keyword_is_checked():
    f = clrs_amd.flatten(SUITE[0][1])
    with pytest.raises(ValueError, match="gemm_batch"):
        preprocess(f, reveal=HostReveal, substitute="device")
    with pytest.raises(ValueError, match="substitute"):
        preprocess(f, reveal=HostReveal, substitute="gpu")


def test_mpmath_helpers_never_see_the_constraint_dimension(planted_ce, monkeypatch):
    """Elements that _mp_sum, _split and _dot process: under "device" the same for the planted instance and for a copy with every cluster twice
    (sum_j P_j doubles, N does not), up to the doubled count of removed constraints; under "host" twice as many, up to the part that depends on N alone."""
    seen = {}

    def counted(name, size):
        fn = getattr(pre, name)

        def wrapper(*a, **kw):
            seen[name] = seen.get(name, 0) + size(*a)
            return fn(*a, **kw)
        monkeypatch.setattr(pre, name, wrapper)
    counted("_mp_sum", lambda planes: int(np.prod(np.shape(planes)[1:])))
    counted("_split", lambda a, planes: int(np.size(np.asarray(a, dtype=object))))
    counted("_dot", lambda u, v: len(u))
    f1, f2 = clrs_amd.flatten(planted_ce), clrs_amd.flatten(gu.replicate_clusters(planted_ce))
    assert f2.x_len == 2 * f1.x_len and f2.n_free == f1.n_free
    counts = {}
    for sub, rv in (("device", HostGemmReveal), ("host", HostReveal)):
        for tag, f in (("once", f1), ("twice", f2)):
            seen.clear()
            red, cs, vr = preprocess(f, reveal=rv, substitute=sub)
            counts[sub, tag] = (sum(seen.values()), len(cs))
    print(counts)
    (d1, r1), (d2, r2), (h1, _), (h2, _) = counts["device", "once"], counts["device", "twice"], counts["host", "once"], counts["host", "twice"]
    assert r1 == len(gu.PLANTS_CE) and r2 == 2 * r1
    assert abs(d2 - d1) <= r2 - r1
    # host: everything over a constraint dimension doubles; what does not is the N x N Gram matrix of the free variables (_mp_sum), the (N + 1)^2 and N^2
    # Gram matrices handed to rank_reveal (_split), b and the relations -- a count that depends on N alone, at most 4 (N + 1)^2
    fixed = 2 * h1 - h2
    assert 0 <= fixed <= 4 * (f1.n_free + 1) ** 2 and h2 - h1 > 100 * d1

"""find_field on the device (clrs_mw_minpoly): the kernel against the host build of the same header byte for byte, the launch cuts, the
times, the refusals, the independent device path through clrs_zz_lll, and the icosahedron end to end with every device default."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from tests import minpoly_util as mu

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 63, 64, 65, 193)


@pytest.mark.parametrize("limbs", rounding.LIMBS)
@pytest.mark.parametrize("deg", (1, 2, 3, 4))
def test_device_equals_the_host_build(deg, limbs):
    vals, bits, eb = mu.mixed(deg, limbs)
    host = mu.mixed_host(deg, limbs)
    status, rung = host[1], host[2]
    print("deg", deg, "limbs", limbs, "statuses of the first wave", sorted(set(int(s) for s in status[:64])), "rungs", int(rung[:64].min()), "..",
          int(rung[:64].max()), "most exchanges", int(host[4][0, :mu.TOTAL].max()), "most rungs", int(host[4][1, :mu.TOTAL].max()))
    found = rung[:64][status[:64] == 0]
    assert {0, 1, 2, 4} <= set(int(s) for s in status[:64]) and status[1] in (0, 5) and rung[1] == 1 and found.max() > 5 * found.min()     # (early and late)
    for count in COUNTS:
        mu.same(mu.device_call(limbs, deg, count, vals, mu.TOTAL + mu.PAD, bits, eb, mu.ND), host, count)


@pytest.mark.parametrize("deg", (1, 2, 3, 4))
def test_result_does_not_depend_on_the_launch_cut(deg):
    limbs = 6
    vals, bits, eb = mu.mixed(deg, limbs)
    host = mu.mixed_host(deg, limbs)
    L = _lib.load()
    try:
        for n in (1, 7, 0):
            assert L.clrs_config_set(b"field_round_launch_rungs", n) == 0
            mu.same(mu.device_call(limbs, deg, 65, vals, mu.TOTAL + mu.PAD, bits, eb, mu.ND), host, 65)
    finally:
        L.clrs_config_set(b"field_round_launch_rungs", 0)


def test_times_are_reported():
    vals, bits, eb = mu.mixed(2, 4)
    mu.device_call(4, 2, 65, vals, mu.TOTAL + mu.PAD, bits, eb, mu.ND)
    a, b = C.c_double(-1), C.c_double(-1)
    assert _lib.load().clrs_mw_minpoly_times(C.byref(a), C.byref(b)) == 0 and 0.0 < a.value <= b.value


def test_refusals_come_before_any_device_work():
    L = _lib.load()
    limbs, deg, n, nd = 4, 2, 3, 2
    v = np.zeros((limbs, n))
    rel, status, rung, err, info = mu._pools(deg, n, nd)
    pi, pd = mu._pi, mu._pd

    def call(limbs=limbs, deg=deg, count=n, plane=n, eb=1e-15, nd=nd):
        return L.clrs_mw_minpoly(0, limbs, deg, count, pd(v), plane, 100, eb, nd, pi(rel), pi(status), pi(rung), pd(err), pi(info))

    for kw in (dict(limbs=3), dict(limbs=7), dict(limbs=12), dict(deg=0), dict(deg=5), dict(count=n + 1), dict(nd=0), dict(nd=rounding.LLL_MAX_DIGITS + 1), dict(eb=0.0),
               dict(eb=-1e-15)):
        assert call(**kw) == -1, kw                                              # CLRS_ERR_INVALID
        assert b"minpoly" in L.clrs_last_error()
    assert (status == mu.SENTINEL).all() and (rel == mu.SENTINEL).all() and (err == mu.SENTINEL).all() and (info == mu.SENTINEL).all()
    a, b = C.c_double(-1), C.c_double(-1)
    assert L.clrs_mw_minpoly_times(C.byref(a), C.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0      # no device work was timed
    assert call() == 0 and list(status) == [5, 5, 5]                             # (0 + 1 v ~ 0 for v = 0)


# ---- the independent device path ---------------------------------------------------------------------------------------------------------------------------------
def test_relations_by_lll_batch_give_the_same_polynomials():
    limbs, bits = 5, mu.generic_bits(4, 4)
    for name, (x, poly) in mu.PLANTED.items():
        v, deg = mu.planes([x], limbs), len(poly) - 1
        kernel = rounding.minimal_polynomials(v, limbs, max_degree=deg, min_degree=deg, bits=bits, relations=False)
        rel, status, rung, err = rounding.minpoly_relations_lll(v, deg, limbs, bits=bits)
        assert kernel.degree[0] == deg and kernel.path[0, deg - 1] == 0 and status[0] == 0 and err[0] < 1e-15, name
        assert kernel.minpoly[0] == poly == rounding._primitive(rel[0]), name


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------------
def test_icosahedron_end_to_end_with_every_device_default():
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    from tests import field_system_util as fsu
    problem = fsu.delsarte_field_problem("icosahedron")
    with data_planes(10):
        f = clrs_amd.flatten(problem.to_sdp(640))
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    assert res.error_code == 0 and res.status == "Optimal"
    found = rounding.find_field(f, res)
    print("icosahedron: minpoly", found.minpoly, "g", mp.nstr(found.g, 20))
    assert found.degree == 2
    with mp.workprec(700):
        c, = rounding.to_field([mp.sqrt(5)], found, limbs=10)
        back = mp.fsum(mp.mpf(x.numerator) / x.denominator * found.g ** k for k, x in enumerate(c))
        assert abs(back - mp.sqrt(5)) < 1e-10
    out = rounding.kernel_vectors(f, res, rationalize=True, field=found)
    assert sum(k.count for k in out) > 0 and all((k.round_status == 0).all() for k in out if k.count)

"""clrs_mw_field_round on the device: digit for digit against the host build of the same header, on batches that mix early and late
acceptances and every status inside one wave, at every count around a wave and over several workgroups, for every (degree, limbs) on offer and for every
cut of the launches; `field_relations_lll` (clrs_zz_lll) as the independent device path; and the two Delsarte problems over QQ(sqrt 5) end to end."""
import functools
import json
import os

import mpmath as mp
import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd.mw import to_limbs
from clrs_amd.rounding import RoundingSettings, kernel_vectors
from tests import field_round_util as fu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "delsarte_field_kernel.json")
COUNTS = (0, 1, 63, 64, 65, 193)
TOTAL, PAD, ND = 193, 3, 6
FIELD_OF = {2: ("x2-5", (4, 16, 40)), 3: ("x3-2", (4, 16)), 4: ("x4-x-1", (4, 16))}


@functools.lru_cache(maxsize=None)
def _mixed(deg, limbs):
    """193 numbers whose first wave holds, side by side: zeros and small integers (accepted at the first rungs), planted elements of every height (the
    tallest accepted last), pi (no relation before the ladder, cut by `bits`, ends: status 1), NaN and Inf (2) and a number too large (4).  errbound is
    the one of the tallest planted height; bits = (deg + 1)(h + 8) - 6 leaves the ladder short of the p ~ (deg + 1)(h + 8) at which deg + 1 generic reals
    have a relation below it.  Returns (field, values (limbs, 196), bits, errbound, the planted elements by position)."""
    name, heights = FIELD_OF[deg]
    f, h = fu.field(name), max(heights)
    eb, bits = fu.planted_errbound(deg, h), (deg + 1) * (h + 8) - 6
    vals, planted = np.zeros((limbs, TOTAL + PAD)), {}
    special = {0: 0.0, 1: 1.0, 2: -3.0, 5: np.nan, 9: np.inf, 13: 2.0 ** 23, 62: -np.inf, 64: 7.0, 100: np.nan}
    with mp.workprec(fu.MP_PREC):
        pis = {3: mp.pi, 40: mp.e, 130: -mp.pi / 7}
        pools = {hh: fu.planted(name, hh, TOTAL, limbs=limbs, seed=deg) for hh in heights}
        for i in range(TOTAL):
            if i in special:
                vals[0, i] = special[i]
            elif i in pis:
                vals[:, i] = to_limbs([pis[i]], limbs)[:, 0]
            else:
                hh = heights[i % len(heights)]
                vals[:, i] = pools[hh][1][:, i]
                planted[i] = pools[hh][0][i]
    vals[:, TOTAL:] = 0.5                                                        # behind every count: must never be read into a result
    return f, vals, bits, eb, planted


@functools.lru_cache(maxsize=None)
def _host(deg, limbs):
    f, vals, bits, eb, planted = _mixed(deg, limbs)
    return fu.host_call(limbs, deg, f.powers(limbs), TOTAL, vals, TOTAL + PAD, bits, eb, ND)


def _same(dev, host, count):
    """bit for bit on the first `count` entries of every row; sentinels behind them"""
    for name, d, h in zip(("rel", "status", "rung", "err", "vq", "info"), dev, host):
        assert d[..., :count].tobytes() == np.ascontiguousarray(h[..., :count]).tobytes(), name
        assert (d[..., count:] == fu.SENTINEL).all(), name


@pytest.mark.parametrize("limbs", rounding.LIMBS)
@pytest.mark.parametrize("deg", (2, 3, 4))
def test_device_equals_the_host_build(deg, limbs):
    f, vals, bits, eb, planted = _mixed(deg, limbs)
    host = _host(deg, limbs)
    rel, status, rung = host[0], host[1], host[2]
    wave = status[:64]
    print("deg", deg, "limbs", limbs, "statuses of the first wave", sorted(set(int(s) for s in wave)), "rungs", int(rung[:64].min()), "..", int(rung[:64].max()),
          "most exchanges", int(host[5][0, :TOTAL].max()), "most rungs", int(host[5][1, :TOTAL].max()))
    assert {0, 1, 2, 4} <= set(int(s) for s in wave) and status[0] == 0 and rung[0] == 1 and rung[:64].max() > 5 * rung[1]
    ints = rounding.planes_to_ints(rel[:, :, :TOTAL]).T
    for i, e in planted.items():                                                 # the host build is right, so the device is compared with the right thing
        assert status[i] == 0 and tuple(rounding._field_coeffs(ints[i:i + 1], status[i:i + 1])[0]) == e, i
    for count in COUNTS:
        _same(fu.device_call(limbs, deg, f.powers(limbs), count, vals, TOTAL + PAD, bits, eb, ND), host, count)


def test_a_relation_among_the_powers_alone_is_status_5_on_the_device():
    """3/2 passed off as a generator of degree 2: 3 - 2 g = 0 is the first row for every number whose own relation is longer, so status 5 cannot share a
    call with late acceptances; it shares one with rung-1 acceptances (0, 1: shorter relations), NaN and pi"""
    f, limbs = fu.field("3/2"), 5
    vals = np.zeros((limbs, 70))
    with mp.workprec(fu.MP_PREC):
        vals[:, 3] = to_limbs([mp.pi], limbs)[:, 0]
        vals[:, 66] = to_limbs([mp.sqrt(7)], limbs)[:, 0]
    vals[0, 1], vals[0, 2], vals[0, 65] = 1.0, np.nan, np.inf
    vals[0, 4:64] = np.sqrt(np.arange(4, 64) + 0.5)
    host = fu.host_call(limbs, 2, f.powers(limbs), 67, vals, 70, 1000, 1e-15, ND)
    assert list(host[1][:4]) == [0, 0, 2, 5] and (host[1][4:64] == 5).all() and list(host[1][64:67]) == [0, 2, 5]
    _same(fu.device_call(limbs, 2, f.powers(limbs), 67, vals, 70, 1000, 1e-15, ND), host, 67)


@pytest.mark.parametrize("deg", (2, 3, 4))
def test_result_does_not_depend_on_the_launch_cut(deg):
    limbs = 6
    f, vals, bits, eb, planted = _mixed(deg, limbs)
    host = _host(deg, limbs)
    L = _lib.load()
    try:
        for n in (1, 7, 0):
            assert L.clrs_config_set(b"field_round_launch_rungs", n) == 0
            _same(fu.device_call(limbs, deg, f.powers(limbs), 65, vals, TOTAL + PAD, bits, eb, ND), host, 65)
    finally:
        L.clrs_config_set(b"field_round_launch_rungs", 0)


def test_times_are_reported():
    import ctypes as C
    f, vals, bits, eb, planted = _mixed(2, 4)
    fu.device_call(4, 2, f.powers(4), 65, vals, TOTAL + PAD, bits, eb, ND)
    a, b = C.c_double(-1), C.c_double(-1)
    assert _lib.load().clrs_mw_field_round_times(C.byref(a), C.byref(b)) == 0 and 0.0 < a.value <= b.value


# ---- the independent device path ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h", [("x2-5", 16), ("x2-2", 40), ("x3-2", 16), ("x4-x-1", 4)])
def test_relations_by_lll_batch_give_the_same_elements(name, h):
    f = fu.field(name)
    limbs, eb = fu.planted_limbs(f.degree, h), fu.planted_errbound(f.degree, h)
    elems, vals = fu.planted(name, h, 4)
    kernel = rounding.round_to_field(vals, f, limbs, errbound=eb, relations=False)
    by_lll = rounding.field_relations_lll(vals, f, limbs, errbound=eb)
    assert (kernel.status == 0).all() and (by_lll.status == 0).all() and (kernel.path == 0).all() and (by_lll.path == 1).all()
    assert [tuple(c) for c in kernel.coeffs] == elems == [tuple(c) for c in by_lll.coeffs]
    assert (by_lll.err < eb).all() and fu.vq_error(by_lll.vq, elems, f) <= mp.ldexp(1, -53 * limbs + limbs + 6) * 2 ** (h + 2)


def test_degree_5_and_the_rescue_of_status_4():
    f = fu.field("x5-x-1")
    elems, vals = fu.planted("x5-x-1", 4, 3, limbs=4)
    r = rounding.round_to_field(vals, f, 4, errbound=fu.planted_errbound(5, 4))  # no kernel for degree 5: all through clrs_zz_lll
    assert (r.status == 0).all() and (r.path == 1).all() and [tuple(c) for c in r.coeffs] == elems
    with pytest.raises(ValueError, match="degrees"):
        rounding.round_to_field(vals, f, 4, relations=False)
    f2 = fu.field("x2-5")
    elems, vals = fu.planted("x2-5", 40, 3)
    eb = fu.planted_errbound(2, 40)
    stuck = rounding.round_to_field(vals, f2, 4, errbound=eb, nd=1, relations=False)
    assert (stuck.status == 4).all()
    r = rounding.round_to_field(vals, f2, 4, errbound=eb, nd=1)
    assert (r.status == 0).all() and (r.path == 1).all() and [tuple(c) for c in r.coeffs] == elems


# ---- the kernel vectors and their rounding in one call -----------------------------------------------------------------------------------------------------------
def test_kernel_vectors_field_is_kernel_vectors_then_field_round_then_gemm():
    """clrs_mw_kernel_vectors_field against its three parts called one by one: bit for bit on the shared outputs of clrs_mw_kernel_vectors, on
    clrs_mw_field_round of the vectors' entries, and on max |head (Y_b Vq_b)| restated by gemm_batch; on blocks of 1, 3 and 5 rows, one without vectors"""
    from clrs_amd.mw import gemm_batch
    f, limbs = fu.field("x2-5"), 6
    with mp.workprec(fu.MP_PREC):
        g = f.g
        ws = [[mp.mpf(1)], [1 / g, (1 + g) / 4, mp.mpf(1)], [mp.mpf(2) / 3, g / 7, mp.mpf(0), (3 - g) / 11, mp.mpf(1)]]
        Xs, Ys = [], []
        for w in ws:
            nn = mp.fsum(x * x for x in w)
            Xs.append(to_limbs([[a * b for a in w] for b in w], limbs))
            Ys.append(to_limbs([[(1 if i == j else 0) - a * b / nn for i, a in enumerate(w)] for j, b in enumerate(w)], limbs))
        Xs.append(to_limbs([[mp.mpf(0)] * 2] * 2, limbs))                      # X = 0, Y = 1: no vector
        Ys.append(to_limbs([[mp.mpf(1), mp.mpf(0)], [mp.mpf(0), mp.mpf(1)]], limbs))
    block_n = [1, 3, 5, 2]
    X, Y = np.concatenate(Xs, axis=1), np.concatenate(Ys, axis=1)
    args = (block_n, X, Y, limbs, 1e-10, True, 1e7, 1e-15)
    one = rounding.kernel_vectors_field_batch(*args, field=f, bits=1000)                                          # the single call
    parts = rounding.kernel_vectors_field_batch(*args, field=f, bits=1000, batch=rounding.kernel_vectors_batch)    # the three calls
    plain = rounding.kernel_vectors_batch(*args[:7])
    assert [k.count for k in one] == [1, 1, 1, 0]
    for a, b, c in zip(one, parts, plain):
        for name in ("perm", "vectors", "resid_max", "v_max", "pivot_resid"):
            assert getattr(a, name).tobytes() == getattr(c, name).tobytes(), name
        assert (a.branch, a.rank, a.count) == (c.branch, c.rank, c.count) and a.num is None and a.den is None
        for name in ("round_status", "round_rung", "vectors_rounded", "round_resid_max"):
            assert np.ascontiguousarray(getattr(a, name)).tobytes() == np.ascontiguousarray(getattr(b, name)).tobytes(), name
        assert a.coeffs.shape == b.coeffs.shape and (a.coeffs == b.coeffs).all() and (a.round_status == 0).all()
    vec = rounding.vectors_to_field(one[2])[0]
    scale = vec[4][0]                                                            # the entry that is 1 in w
    assert scale != 0 and vec[4][1] == 0 and [tuple(x / scale for x in e) for e in vec] == [(rounding.Fraction(2, 3), 0), (0, rounding.Fraction(1, 7)), (0, 0),
                                                                                         (rounding.Fraction(3, 11), rounding.Fraction(-1, 11)), (1, 0)]
    off = 0
    for nn, k in zip(block_n, one):
        if k.count:
            again = gemm_batch([(Y[:, off:off + nn * nn].reshape(limbs, nn, nn), k.vectors_rounded, None, False, False, 1, 0)], limbs)[0]
            assert np.max(np.abs(again[0]), axis=0).tobytes() == k.round_resid_max.tobytes() and (k.round_resid_max < 1e-10).all()
        off += nn * nn


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------------------
def _tuples(out):
    return {str(b): [[[str(x) for x in e] for e in vec] for vec in rounding.vectors_to_field(k)] for b, k in enumerate(out) if k.count}


@pytest.mark.parametrize("name", list(fu.DELSARTE))
def test_delsarte_problems_over_q_sqrt5_end_to_end(name):
    from clrs_amd.mw import gemm_batch, solvesdp_mw
    n, d, cos, objective, blocks, counts, height = fu.DELSARTE[name]
    f = fu.delsarte_flat(name)
    res = solvesdp_mw(f, limbs=6, data_limbs=6, duality_gap_threshold=1e-60)
    print(name, res.status, "error code", res.error_code, "iterations", res.iterations, "gap", res.duality_gap, "objective", res.primal_objective)
    # (how the solve ended is not this test's subject: at 6 limbs the icosahedron stalls at a gap of 3.6e-60, just above the threshold; the iterate is what is rounded)
    assert res.duality_gap <= 1e-55 and abs(res.primal_objective - objective) <= 1e-9
    with mp.workprec(400):
        field = rounding.NumberField([-5, 0, 1], mp.sqrt(5))
    out = kernel_vectors(f, res, limbs=6, rationalize=True, field=field)
    assert {b: k.count for b, k in enumerate(out) if k.count} == counts
    # The vectors of a block come in pivot order, and the elimination of the 600-cell's block 19 meets two equal diagonal entries (pivots 3 and 9): which goes
    # first is decided by the last bits of the iterate, and the device's iterate takes the other order than the oracle's.  Same vectors, so: as sorted lists.
    golden = json.load(open(GOLDEN))[name]["blocks"]
    got = _tuples(out)
    assert sorted(got) == sorted(golden) and all(sorted(got[b]) == sorted(golden[b]) for b in golden)
    tau = RoundingSettings().kernel_errbound
    for b, k in enumerate(out):
        if not k.count:
            continue
        assert k.num is None and k.den is None and (k.round_status == 0).all()
        nn = int(f.block_n[b])
        off = int(sum(int(x) ** 2 for x in f.block_n[:b]))
        Yb = np.asarray(res.Y)[:6, off:off + nn * nn].reshape(6, nn, nn)
        again = gemm_batch([(Yb, k.vectors_rounded, None, False, False, 1, 0)], 6)[0]
        assert np.max(np.abs(again[0]), axis=0).tobytes() == k.round_resid_max.tobytes() and (k.round_resid_max < tau).all()


def test_field_none_is_todays_path_over_qq():
    from clrs_amd import problems as P
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.sdp import data_planes
    with data_planes(10):
        f = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5, prec=640))
    res = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
    assert res.error_code == 0
    with mp.workprec(700):
        degree_one = rounding.NumberField([-1, 2], mp.mpf(1) / 2)
    today = kernel_vectors(f, res, res, rationalize=True, round_batch=rounding.kernel_vectors_rational_batch)
    for fld in (None, degree_one):
        now = kernel_vectors(f, res, res, rationalize=True, field=fld)
        for a, b in zip(today, now):
            assert a.num.tobytes() == b.num.tobytes() and a.den.tobytes() == b.den.tobytes() and a.round_status.tobytes() == b.round_status.tobytes()
            assert a.vectors_rounded.tobytes() == b.vectors_rounded.tobytes() and b.coeffs is None and b.round_rung is None

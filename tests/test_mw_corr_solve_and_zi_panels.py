"""The launch form of k_mwi_Zi, which does the SAME floating-point operations in the same order whatever the form:

`clrs_config_set("mw_zi_narrow", 1)` (default): workgroups of 256 threads with column panels of half the width -- one wave per SIMD -- where the
launch keeps a compute unit per workgroup (csrc/clrs_mw_zi_panels.h); 0: always 512 threads, the launch as it was.

Every result must therefore agree BIT FOR BIT between the forms.  The Zs panels are rewritten by every launch and handed to the last arriver of twice as
many workgroups, so a consumer that read a stale L1 or L2 line would show as a bit difference.  These are ordinary solves; nothing is provoked.

(The file is named after the change it came with; the other half of that change, the corrector's refined solve as one launch, was measured at no gain
and is not in the code: DESIGN.md section 5.9.)"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests.util import flat

pytestmark = pytest.mark.gpu

VARIANTS = [("default", {}), ("mw_zi_narrow=0", {"mw_zi_narrow": 0})]
RADII3, RADII5 = [1.0, 1.125, 1.25], [1.0, 1.125, 1.25, 1.375, 1.5]


def _set(cfg):
    from clrs_amd import _lib
    L = _lib.load()
    for k, v in cfg.items():
        _lib.check(L.clrs_config_set(k.encode(), v))


def _restore():
    from clrs_amd import _lib
    L = _lib.load()
    L.clrs_config_set(b"mw_zi_narrow", 1)


def _context(f, cfg, **kw):
    """a context created under the switches `cfg`; the process-wide configuration is back at its defaults afterwards"""
    from clrs_amd.mw import MwSchurContext
    try:
        _set(cfg)
        return MwSchurContext(f, **kw)
    finally:
        _restore()


def _assert_same_solve(a, b, what):
    assert a.error_code == b.error_code and a.status == b.status and a.iterations == b.iterations, (what, a.status, b.status, a.iterations, b.iterations)
    assert np.array_equal(np.asarray(a.history), np.asarray(b.history)), what          # (the table rows carry no wall-clock column)
    for name in ("x", "y", "X", "Y"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)
    assert np.array_equal(a.timings["objectives_limbs"], b.timings["objectives_limbs"]), what


def _multi(radii):
    import clrs_amd
    from clrs_amd.problems import cohnelkies_multi
    return clrs_amd.flatten(cohnelkies_multi(8, 15, radii))


def _problem(name):
    return _multi(RADII3) if name == "ce_multi3" else _multi(RADII5) if name == "ce_multi5" else flat(name)


INSTANCES = [
    # the workload's shapes (2 clusters, 16 x 16 blocks, N = 31) in both dispatches of the factor limbs
    ("ce_8_15", dict(limbs=5, data_limbs=5), {}),
    # (4 limbs, ~209 bits: error thresholds 1e-25 instead of the 256-bit defaults, as test_four_limbs_reach_the_objective_with_thresholds_for_209_bits)
    ("ce_8_15", dict(limbs=4, data_limbs=4), dict(dual_error_threshold=1e-25, primal_error_threshold=1e-25, duality_gap_threshold=1e-12)),
    ("ce_8_3", dict(limbs=5), dict(maxiterations=15)),        # two clusters of 4 x 4 blocks: one panel per block, a hand-off with a single arriver
    ("polyopt8", dict(limbs=5), {}),                          # sides of 5 and below: a panel wider than the block
    ("x2p1", dict(limbs=5), {}),
    ("polyopt40", dict(limbs=5), {}),                         # 21 rows: one-column panels, n no multiple of the pass
    ("delsarte_3_10", dict(limbs=5), {}),
    ("ce_multi3", dict(limbs=5), {}),                         # four clusters, 8 blocks: 64 narrow workgroups
    ("ce_multi5", dict(limbs=5), {}),                         # six clusters, 12 blocks: 96 narrow workgroups
]


@pytest.mark.parametrize("name,ckw,skw", INSTANCES, ids=["%s-K%d" % (n, c["limbs"]) for n, c, _ in INSTANCES])
def test_switch_for_switch_bit_identity(name, ckw, skw):
    """whole solves with the switch at 0: x, y, X, Y, the objectives' limbs and every table row identical to the default's"""
    from clrs_amd.mw import solvesdp_mw
    f = _problem(name)
    res = []
    for label, cfg in VARIANTS:
        ctx = _context(f, cfg, **ckw)
        try:
            res.append((label, solvesdp_mw(f, ctx=ctx, **skw)))
        finally:
            ctx.close()
    ref = res[0][1]
    assert ref.error_code in (0, 2) and ref.iterations >= 5, (ref.status, ref.error_code, ref.iterations)
    if "maxiterations" not in skw:
        assert ref.error_code == 0 and ref.status == "Optimal", (ref.status, ref.error_code)
    for label, r in res[1:]:
        _assert_same_solve(ref, r, (name, label))


_TRACED = """
import sys
sys.path.insert(0, sys.argv[1])
from tests.util import flat
from clrs_amd import _lib
from clrs_amd.mw import MwSchurContext, solvesdp_mw
_lib.check(_lib.load().clrs_config_set(b"mw_zi_narrow", int(sys.argv[2])))
f = flat("ce_8_15")
ctx = MwSchurContext(f, limbs=5, data_limbs=5)
solvesdp_mw(f, ctx=ctx, maxiterations=2)
ctx.close()
"""


@pytest.mark.parametrize("narrow,expect", [(1, (8, 256)), (0, (4, 512))], ids=["default", "mw_zi_narrow=0"])
def test_zi_is_launched_narrow_on_the_workload_and_wide_when_switched_off(narrow, expect, tmp_path):
    """cohnelkies(8,15): 4 blocks, the largest 16 x 16 -- eight panels of two columns in workgroups of 256 threads by default, four panels of four
    columns in workgroups of 512 threads with the switch off.  The library offers no accessor for the shape of a launch and the C ABI gains none for this:
    the launches themselves are read from a kernel trace of a two-iteration solve in a child process (this test is about that trace)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to read the launch shape of k_mwi_Zi"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "--", sys.executable, "-c", _TRACED, root, str(narrow)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    traces = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    assert traces, os.listdir(str(tmp_path))
    shapes = set()
    for t in traces:
        for row in csv.DictReader(open(t)):
            if "k_mwi_Zi<" in row["Kernel_Name"]:
                wg = int(row["Workgroup_Size_X"])
                assert int(row["Workgroup_Size_Y"]) == 1 and int(row["Grid_Size_X"]) == 4 * wg          # one workgroup per block in x
                shapes.add((int(row["Grid_Size_Y"]), wg))
    assert shapes == {expect}, shapes                          # every launch of the solve: (panels per block, threads)


def test_many_live_contexts_reuse_zs_without_stale_lines():
    """Six contexts alive at once, two streams each, two whole solves in every context in turn: Zs is rewritten by every launch, and a last arriver
    that read a line of an earlier launch -- from its compute unit's L1 or its XCD's L2 -- would end with different bits than the wide launch's"""
    from clrs_amd.mw import solvesdp_mw
    f = flat("ce_8_15")
    kw = dict(limbs=5, data_limbs=5)
    wide = _context(f, {"mw_zi_narrow": 0}, **kw)
    try:
        ref = solvesdp_mw(f, ctx=wide)
    finally:
        wide.close()
    assert ref.error_code == 0 and ref.status == "Optimal"
    ctxs = [_context(f, {}, **kw) for _ in range(6)]
    try:
        for rep in range(2):
            for c in ctxs:
                _assert_same_solve(ref, solvesdp_mw(f, ctx=c), ("live contexts", rep))
    finally:
        for c in ctxs:
            c.close()


def test_switches_on_a_sharded_solve_on_one_gpu():
    """two ranks on one GPU (contexts of one process, one thread each, in-process exchanges; each rank 2 clusters, 4 blocks of up to 16 rows: the rule
    gives it the narrow panels too) -- equal bits under both values of the switch"""
    from clrs_amd.mw import LocalGroup, MwSchurContext, shard_problem, solvesdp_mw
    full = _multi(RADII3)
    world = 2

    def solve(cfg):
        group = LocalGroup(world)
        out, err = [None] * world, [None] * world
        shards = [shard_problem(full, r, world) for r in range(world)]
        try:                                          # the switches are process-wide and read at creation: create every rank's context here, then let the threads run
            _set(cfg)
            ctxs = [MwSchurContext(s, limbs=5) for s, _ in shards]
        finally:
            _restore()

        def run(rank):
            try:
                ctxs[rank].comm_init_local(group, rank)
                out[rank] = solvesdp_mw(shards[rank][0], ctx=ctxs[rank], shard_info=shards[rank][1])
            except Exception as e:                  # a failing rank must not leave the others waiting in a collective: nothing to do but report
                err[rank] = e
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        for c in ctxs:
            c.close()
        group.close()
        assert all(e is None for e in err), err
        assert all(o is not None for o in out)
        return out
    ref = solve({})
    assert ref[0].error_code == 0 and ref[0].status == "Optimal"
    for label, cfg in VARIANTS[1:]:
        got = solve(cfg)
        for rank in range(world):
            _assert_same_solve(ref[rank], got[rank], ("sharded", label, rank))

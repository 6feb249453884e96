"""A plain `bench.py` run on the GPU: the headline fields, nothing of `--full`, and `--dump-outputs` holding the timed solve's own result."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_plain_bench_run_reports_the_headline_and_dumps_the_last_timed_solve(tmp_path):
    import clrs_amd
    from clrs_amd.mw import MwSchurContext, solvesdp_mw
    from clrs_amd.problems import cohnelkies
    from clrs_amd.sdp import data_planes
    from tests.util import mw_relerr
    K = 5
    with data_planes(K):
        flat = clrs_amd.flatten(cohnelkies(8, 15))
    ctx = MwSchurContext(flat, limbs=K, device=0, data_limbs=K)
    ref = solvesdp_mw(flat, ctx=ctx, dual_error_threshold=1e-30, primal_error_threshold=1e-30, duality_gap_threshold=1e-15)
    ctx.close()
    assert ref.status == "Optimal" and ref.iterations > 0
    # as many timed iterations as one whole solve takes: the last timed call is that solve, from the same starting point
    n = ref.iterations
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", "3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "interior-point iterations/sec" and line["unit"] == "iterations/s" and line["higher_is_better"] is True
    assert line["steps"] == n and line["warmup"] == 3 and line["dtype"].startswith(f"f64x{K}")
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    for key in ("full_solve", "hot_path", "parity", "cpu_baseline", "roofline", "roofline_mw", "roofline_timed", "fp64", "multi_gpu"):
        assert key not in line, key
    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["X", "Y", "history", "objectives", "x", "y"]
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["history"].shape == ref.history.shape
    for name, want in (("x", ref.x), ("y", ref.y), ("X", ref.X), ("Y", ref.Y), ("objectives", ref.timings["objectives_limbs"].T)):
        a = got[name] if name != "objectives" else got[name].T
        assert a.shape == want.shape and mw_relerr(a, want) <= 1e-60, name
    assert abs(math.fsum(got["objectives"][1]) - math.pi ** 4 / 384) <= 1e-4

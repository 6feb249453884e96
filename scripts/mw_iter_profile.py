"""Whole interior-point solves of cohnelkies(8,15) at 5 limbs, for `rocprofv3 --kernel-trace`: the trace of the last solve is what
scripts/iter_timeline.py turns into a per-iteration timeline (kernel, stream, start offset, duration, gap).
    python scripts/mw_iter_profile.py [instance [solves]] [switch=value ...]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.util import flat
from clrs_amd.mw import MwSchurContext, solvesdp_mw

args = [a for a in sys.argv[1:] if "=" not in a]
name = args[0] if len(args) > 0 else "ce_8_15"
reps = int(args[1]) if len(args) > 1 else 3
for a in sys.argv[1:]:                      # key=value: a switch of clrs_config_set, set before the context is created (e.g. mw_xinv_product=0)
    if "=" in a:
        from clrs_amd import _lib
        _lib.check(_lib.load().clrs_config_set(a.split("=")[0].encode(), int(a.split("=")[1])))
f = flat(name)
ctx = MwSchurContext(f, limbs=5)
for _ in range(reps):
    t = time.time()
    r = solvesdp_mw(f, ctx=ctx)
    dt = time.time() - t
    print(name, r.status, r.iterations, "%.4f s, %.1f us / iteration (host loop %.4f s)" % (dt, 1e6 * r.time_total / r.iterations, r.time_total))
ctx.close()

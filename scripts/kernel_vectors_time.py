"""Wall time of `kernel_vectors` (clrs_amd.rounding, one clrs_mw_kernel_vectors call over all blocks, copies included) on the solutions `solvesdp_mw`
reaches on the BASELINE configurations, the same with `check_dimensions` (a second call), and one interior-point iteration of the same solve beside them;
writes profiles/rounding/kernel_vectors_times.json.

    python scripts/kernel_vectors_time.py [--limbs 5] [--gap 1e-30] [--instances delsarte_3_10,polyopt40,...] [--out profiles/rounding/kernel_vectors_times.json]

A solution whose vectors fail the reference's checks is recorded with the message (the time is then that of the device calls made until the check failed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# BASELINE configurations 1-5 at the sizes the test suite solves (tests/util.py: instance)
INSTANCES = ("delsarte_3_10", "polyopt40", "ce_8_15", "threepoint_4", "sdpa_small")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limbs", type=int, default=5)
    ap.add_argument("--gap", type=float, default=1e-30)
    ap.add_argument("--instances", default=",".join(INSTANCES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "kernel_vectors_times.json"))
    args = ap.parse_args()
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.rounding import KernelVectorError, kernel_vectors, kernel_vectors_batch
    from tests.util import flat
    out = dict(limbs=args.limbs, duality_gap_threshold=args.gap, instances={})
    for name in [s for s in args.instances.split(",") if s]:
        f = flat(name)
        r = solvesdp_mw(f, limbs=args.limbs, duality_gap_threshold=args.gap)
        rec = dict(blocks=int(f.n_blocks), max_n=int(np.max(f.block_n)), xy_len=int(f.xy_len), iterations=int(r.iterations), error_code=int(r.error_code),
                   duality_gap=float(r.duality_gap), seconds_per_iteration=r.time_total / max(r.iterations, 1))
        for tag, check in (("kernel_vectors", False), ("kernel_vectors_check_dimensions", True)):
            best = None
            for rep in range(1 + args.repeats):                        # (the first call loads the code objects: not counted)
                dev = [0.0, 0]

                def batch(*a, **kw):
                    t = time.perf_counter()
                    try:
                        return kernel_vectors_batch(*a, **kw)
                    finally:
                        dev[0] += time.perf_counter() - t
                        dev[1] += 1
                t = time.perf_counter()
                try:
                    ks = kernel_vectors(f, r, r, limbs=args.limbs, check_dimensions=check, batch=batch)
                    info = dict(vectors=int(sum(k.count for k in ks)), largest_residual=max([float(np.max(k.resid_max)) for k in ks if k.count] + [0.0]))
                except KernelVectorError as e:
                    info = dict(refused=str(e))
                cur = dict(seconds=time.perf_counter() - t, device_call_seconds=dev[0], device_calls=dev[1], **info)
                if rep > 0 and (best is None or cur["seconds"] < best["seconds"]):
                    best = cur
            best["ratio_to_one_iteration"] = best["seconds"] / rec["seconds_per_iteration"]
            rec[tag] = best
        out["instances"][name] = rec
        print(name, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

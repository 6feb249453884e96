"""Wall time of `preprocess` (clrs_amd.preprocess) next to one interior-point iteration of `solvesdp_mw` on the same instance and limb count, with and
without planted dependencies, and the time of one stand-alone rank-revealing call (copies included) on a matrix beyond LDS and on LDS-resident ones; writes profiles/preprocess/times.json.

    python scripts/preprocess_time.py [--limbs 5] [--out profiles/preprocess/times.json]

`--substitute device` / `both`: the substitution on the device (preprocess(substitute="device")), alone or next to the host substitution in the same
process; per instance and mode the total seconds and the seconds spent outside the device steps (host: mpmath); writes profiles/preprocess/times_device.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANTS = {"ce_8_15": [(0, {0: 0.5}), (0, {1: 0.25, 3: -0.5})], "ns_8_15_2": [(0, {0: 0.5}), (1, {1: 0.25, 3: -0.5})],
          "threepoint_4": [(0, {0: 0.5})], "ns_8_15_3": [(1, {0: 0.25, 5: 0.125}), (3, {10: -0.5})]}


def timed_reveal(log):
    from clrs_amd.preprocess import DeviceReveal

    class Timed(DeviceReveal):
        pass

    def wrap(name):
        inner = getattr(DeviceReveal, name)

        def f(self, *a, **k):
            t = time.perf_counter()
            try:
                return inner(self, *a, **k)
            finally:
                log[name] = log.get(name, 0.0) + time.perf_counter() - t
        return f
    for name in ("__init__", "gram_diag", "dependencies", "free_gram", "rank_reveal", "gemm_batch"):
        setattr(Timed, name, wrap(name))
    return Timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limbs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--substitute", choices=("host", "device", "both"), default="host")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "preprocess", "times.json" if args.substitute == "host" else "times_device.json")
    import clrs_amd
    from clrs_amd.mw import rank_reveal, solvesdp_mw
    from clrs_amd.preprocess import preprocess
    from tests.preprocess_host import plant_dependencies
    from tests.util import instance
    out = dict(limbs=args.limbs, instances={})
    if args.substitute != "host":
        from clrs_amd.preprocess import detect_limbs
        out = dict(prec=256, detect_limbs=detect_limbs(256), instances={})          # (no solve here: --limbs is not used)
        modes = ("host", "device") if args.substitute == "both" else ("device",)
        for name, plants in PLANTS.items():
            base = instance(name)
            for tag, sdp in (("as_is", base), ("planted", plant_dependencies(base, plants))):
                f = clrs_amd.flatten(sdp)
                rec = dict(clusters=int(f.n_clusters), max_P=int(np.max(f.cluster_P)), n_free=int(f.n_free))
                for mode in modes:
                    preprocess(f, prec=256, substitute=mode)              # (first call: loads the code objects)
                    best = None
                    for _ in range(3):
                        log = {}
                        t = time.perf_counter()
                        red, cs, vr = preprocess(f, prec=256, reveal=timed_reveal(log), substitute=mode)
                        t_pre = time.perf_counter() - t
                        if best is None or t_pre < best["total_seconds"]:
                            best = dict(total_seconds=t_pre, host_mpmath_seconds=t_pre - sum(log.values()), device_steps_seconds=log,
                                        removed_constraints=len(cs), removed_variables=int(f.n_free - red.n_free))
                    rec[mode] = best
                if len(modes) == 2:
                    rec["host_over_device"] = rec["host"]["total_seconds"] / rec["device"]["total_seconds"]
                out["instances"][f"{name}/{tag}"] = rec
                print(name, tag, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
        print("wrote", args.out)
        return
    for name, plants in PLANTS.items():
        base = instance(name)
        for tag, sdp in (("as_is", base), ("planted", plant_dependencies(base, plants))):
            f = clrs_amd.flatten(sdp)
            preprocess(f, prec=256)                                   # (first call: loads the code objects)
            log = {}
            t = time.perf_counter()
            red, cs, vr = preprocess(f, prec=256, reveal=timed_reveal(log))
            t_pre = time.perf_counter() - t
            r = solvesdp_mw(red, limbs=args.limbs)
            rec = dict(clusters=int(f.n_clusters), max_P=int(np.max(f.cluster_P)), n_free=int(f.n_free), removed_constraints=len(cs),
                       removed_variables=int(f.n_free - red.n_free), preprocess_seconds=t_pre, device_steps_seconds=log,
                       host_seconds=t_pre - sum(log.values()), iterations=int(r.iterations), seconds_per_iteration=r.time_total / max(r.iterations, 1),
                       error_code=int(r.error_code))
            rec["ratio_to_one_iteration"] = rec["preprocess_seconds"] / rec["seconds_per_iteration"]
            out["instances"][f"{name}/{tag}"] = rec
            print(name, tag, json.dumps(rec), flush=True)
    # the kernel alone where the matrix lives in global memory: a 192 x 192 Gram matrix of rank 190 at 6 limbs
    rng = np.random.default_rng(0)
    M = rng.integers(-3, 4, (200, 190)).astype(float)
    M = np.hstack([M, M[:, :1] + M[:, 1:2], M[:, 2:3] - M[:, 3:4]])
    G = np.zeros((6, 192 * 192))
    G[0] = (M.T @ M).reshape(-1)
    rank_reveal(G, [192], [192], [2.0 ** -280 * np.max(G[0])], 6)
    t = time.perf_counter()
    res = rank_reveal(G, [192], [192], [2.0 ** -280 * np.max(G[0])], 6)
    out["rank_reveal_call_global_memory_192_rank190_6limbs_seconds"] = time.perf_counter() - t
    assert res[0][1] == 190
    for n in (32, 40):
        Gs = np.zeros((6, n * n))
        Gs[0] = (M[:, :n].T @ M[:, :n]).reshape(-1)
        t = time.perf_counter()
        rank_reveal(Gs, [n], [n], [2.0 ** -280 * np.max(Gs[0])], 6)
        out[f"rank_reveal_call_lds_{n}_full_rank_6limbs_seconds"] = time.perf_counter() - t
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

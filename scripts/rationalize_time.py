"""Wall time of the rounding of kernel vectors to rationals (clrs_amd.rounding): `rationalize` alone on pools of planted rationals at every limb count, and
`kernel_vectors(rationalize=True)` beside `kernel_vectors` on the solution `solvesdp_mw` reaches on delsarte_exact(8, 3, 1/2) and on larger members of the
family; writes profiles/rounding/rationalize_times.json.  No time is a pass criterion.

    python scripts/rationalize_time.py [--counts 256,4096,65536] [--instances 8:3,8:6,24:12] [--out profiles/rounding/rationalize_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(fn, repeats):
    fn()                                                     # (the first call loads the code objects: not counted)
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="256,4096,65536")
    ap.add_argument("--instances", default="8:3,8:6,24:12")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "rationalize_times.json"))
    args = ap.parse_args()
    import clrs_amd
    from clrs_amd import problems as P
    from clrs_amd.mw import solvesdp_mw
    from clrs_amd.rounding import KernelVectorError, kernel_vectors, rationalize
    from clrs_amd.sdp import data_planes
    out = dict(pools={}, instances={})
    rng = np.random.default_rng(0)
    for count in (int(c) for c in args.counts.split(",") if c):
        q = rng.integers(1, 10 ** 6, count)
        p = rng.integers(-40 * q, 40 * q)
        for K in (4, 5, 6, 8, 10):
            v = np.zeros((K, count))
            v[0] = p / q                                     # fp64 roundings of p / q: rationals with noise of 1e-16 p / q, below the bound times q only for small q
            v[1] = (p - v[0] * q) / q                        # the next limb: p / q to ~1e-32
            sec, (num, den, status, vq) = best_of(lambda: rationalize(v, K), args.repeats)
            rec = dict(seconds=sec, numbers_per_second=count / sec, found=int(np.sum(status == 0)), recovered=int(np.sum(num * q == p * den)))
            out["pools"][f"{count}x{K}"] = rec
            print("pool", count, "limbs", K, json.dumps(rec), flush=True)
    for n, d in ((int(a), int(b)) for a, b in (s.split(":") for s in args.instances.split(",") if s)):
        with data_planes(10):                                # the sampled problem at the working precision
            f = clrs_amd.flatten(P.delsarte_exact(n, d, 0.5, prec=640))
        r = solvesdp_mw(f, limbs=10, data_limbs=10, duality_gap_threshold=1e-40)
        rec = dict(blocks=int(f.n_blocks), max_n=int(np.max(f.block_n)), iterations=int(r.iterations), status=r.status, error_code=int(r.error_code),
                   duality_gap=float(r.duality_gap), primal_objective=float(r.primal_objective), seconds_per_iteration=r.time_total / max(r.iterations, 1))
        for tag, kw in (("kernel_vectors", {}), ("kernel_vectors_rationalize", dict(rationalize=True))):
            try:
                sec, ks = best_of(lambda: kernel_vectors(f, r, r, **kw), args.repeats)
                rec[tag] = dict(seconds=sec, vectors=int(sum(k.count for k in ks)))
                if kw:
                    rec[tag].update(max_num=max(k.max_num for k in ks), max_den=max(k.max_den for k in ks),
                                    largest_rounded_residual=max([float(np.max(k.round_resid_max)) for k in ks if k.count] + [0.0]))
            except KernelVectorError as e:
                rec[tag] = dict(refused=str(e))
        out["instances"][f"delsarte_exact({n}, {d}, 1/2)"] = rec
        print(n, d, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

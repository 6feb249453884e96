"""Wall time of the pivots of integer systems by RREF mod p on the device (clrs_amd.rounding.rref_mod_p -> clrs_modp_rref) at
p = 10007: random full-row-rank systems of 256 x 1536, 1024 x 6144 and 2048 x 12288 (six columns per row, as the reference selects them) and one
1024 x 6144 system of rank 700; the best of three calls after one warm-up, copies and the Python layer included.  Beside each, where it is estimated to end
within a minute, one run of the numpy restatement of the tests (tests/modp_util.rref_mod_p) on the host, with which the pivots are compared.  Writes
profiles/rounding/modp_pivots_times.json.  No time is a pass criterion.

    python scripts/modp_pivots_time.py [--out profiles/rounding/modp_pivots_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = 10007
HOST_LIMIT = 60.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "modp_pivots_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd.rounding import rref_mod_p
    from tests import modp_util as mu
    rng = np.random.default_rng(0)
    out, host_rate = {}, None                                 # host_rate: seconds per rank * nrows * ncols of the restatement, from the last run
    for nrows, ncols, rank in ((256, 1536, None), (1024, 6144, None), (1024, 6144, 700), (2048, 12288, None)):
        if rank is None:
            A = mu.random_matrix(rng, nrows, ncols, P)
        else:                                                 # rank 700: 700 random rows and 324 random combinations of them, shuffled
            B = mu.random_matrix(rng, rank, ncols, P)
            A = np.concatenate([B, mu.random_matrix(rng, nrows - rank, rank, P) @ B % P])[rng.permutation(nrows)]
        rref_mod_p(A, P)                                      # (the first call loads the code objects: not counted)
        best = None
        for _ in range(args.repeats):
            t = time.perf_counter()
            pivots, r = rref_mod_p(A, P)
            dt = time.perf_counter() - t
            best = dt if best is None or dt < best else best
        rec = dict(nrows=nrows, ncols=ncols, p=P, rank=int(r), device_seconds=best, planted_rank=rank)
        work = float(r) * nrows * ncols
        if host_rate is None or host_rate * work < HOST_LIMIT:
            t = time.perf_counter()
            ref_pivots, ref_rank, _ = mu.rref_mod_p(A, P)
            rec["host_numpy_seconds"] = time.perf_counter() - t
            rec["pivots_equal"] = bool(ref_rank == r and np.array_equal(ref_pivots, pivots))
            host_rate = rec["host_numpy_seconds"] / work
        else:
            rec["host_numpy_seconds"] = None
            rec["host_numpy_estimate_seconds"] = host_rate * work
        out[f"{nrows}x{ncols}" + ("" if rank is None else f"_rank{rank}")] = rec
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Time of the batched LLL reduction (clrs_amd.rounding.lll_batch -> clrs_zz_lll) on scrambled small bases -- a basis with entries
in [-2, 2] times 4 d elementary row operations with multipliers in [-3, 3] (tests/lll_util.scrambled) -- for batches of 1 and 64 lattices at d = 16, 32, 64,
on the rung `lll_first_rung` chooses.  Per row:

  device          the raw calls of clrs_zz_lll `lll_batch` makes (one per (rung, digits) in the batch, `device_calls`), summed: milliseconds in k_zz_lll over all
                  launches and of the whole calls from the first upload to the last download, by device events (clrs_zz_lll_times), the best of `--repeats`
                  after one warm-up; exchanges, passes and launches summed over the batch
  whole           `lll_batch` as a whole, wall time (digit conversion on the host included)
  fraction        at d = 16 only: the `Fraction` LLL of the test helpers (tests/lll_util.fraction_lll) on the first lattice of the batch, wall time, beside the
                  device time of the same lattice alone

Every output must be (0.98, 0.52)-reduced exactly (asserted for the first lattice of each batch).  Writes profiles/rounding/lll_times.json.  No time is a
pass criterion.

    python scripts/lll_time.py [--out profiles/rounding/lll_times.json] [--sizes 16 32 64] [--batches 1 64]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 32, 64])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "lll_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    from tests import lll_util as lu
    L = _lib.load()

    calls = []                           # (kernel ms, whole ms) of every device call since the list was cleared

    def timed_call(*a, **kw):
        out = rounding._lll_call_device(*a, **kw)
        k, w = C.c_double(), C.c_double()
        assert L.clrs_zz_lll_times(C.byref(k), C.byref(w)) == 0
        calls.append((k.value, w.value))
        return out

    def reduce_timed(lattices):
        """(outputs, kernel ms, whole ms, device calls): lll_batch, its device times summed over the calls it made (one per (rung, digits) of the batch)"""
        del calls[:]
        out = rounding.lll_batch(lattices, call=timed_call)
        return out, sum(c[0] for c in calls), sum(c[1] for c in calls), len(calls)

    rows = []
    for d in args.sizes:
        for nb in args.batches:
            lattices = [lu.scrambled(5000 + 100 * d + i, d) for i in range(nb)]
            reduce_timed(lattices)                                                      # warm-up
            best = None
            for _ in range(args.repeats):
                t = time.perf_counter()
                out, kernel_ms, whole_ms, ncalls = reduce_timed(lattices)
                wall = time.perf_counter() - t
                if best is None or whole_ms < best[1]:
                    best = (kernel_ms, whole_ms, wall, ncalls)
            info = rounding.lll_batch.last_info
            assert all(i["status"] == 0 for i in info) and lu.is_lll_reduced(out[0])
            row = {"d": d, "batch": nb, "limbs_and_digits": sorted({(i["limbs"], i["nd"]) for i in info}), "device_calls": best[3],
                   "entry_bits": max(abs(int(v)).bit_length() for A in lattices for v in A.flat), "exchanges": sum(i["swaps"] for i in info),
                   "passes": sum(i["passes"] for i in info), "launches": sum(i["launches"] for i in info), "kernel_seconds": best[0] / 1e3,
                   "raw_call_seconds": best[1] / 1e3, "lll_batch_wall_seconds": best[2]}
            if d == 16:
                t = time.perf_counter()
                red = lu.fraction_lll(lattices[0])
                row["fraction_lll_seconds_first_lattice"] = time.perf_counter() - t
                assert lu.is_lll_reduced(red)
                row["raw_call_seconds_first_lattice"] = reduce_timed(lattices[:1])[2] / 1e3
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "rounding.lll_batch on scrambled small bases, one MI355X; device times by device events, the best of %d after a warm-up" % args.repeats,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

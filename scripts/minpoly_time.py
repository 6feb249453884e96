"""Time of the minimal-polynomial search of find_field (clrs_amd.rounding.minimal_polynomials -> clrs_mw_minpoly).  Per row: `count`
planted numbers r + q s, with s = sqrt 2 (quadratic) or the real root of x^4 - x - 1 (quartic) and rationals r = n / m, |n|, m < 2^4, q in {1/3 .. 3}, searched
at their own degree at 5 and at 10 limbs, bits = (d + 1)(h + 8) - 6 for the height h = 32 of such a polynomial, errbound 2^-(d (h + 8)).  Three columns:

  kernel          clrs_mw_minpoly: milliseconds in k_mw_minpoly over all launches and of the whole call from the first upload to the last download, by device
                  events (clrs_mw_minpoly_times); the median of `--repeats` after one warm-up
  lll_batch       the same numbers through `minpoly_relations_lll` on the device (one clrs_zz_lll call per rung over the numbers still open, the lattices
                  built on the host), wall time; the median of `--repeats`, one run above `--single-above` numbers
  host            the host build of the same header (tests/mw_host/minpoly_host.cpp, g++ -O2) on one core, wall time, likewise

Every number must be found by every path, with the same primitive polynomial (asserted).  Writes profiles/rounding/minpoly_times.json.  No time is a pass
criterion.

    python scripts/minpoly_time.py [--out profiles/rounding/minpoly_times.json] [--counts 64 1024 16384] [--repeats 3] [--single-above 1024]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--counts", type=int, nargs="*", default=[64, 1024, 16384])
    ap.add_argument("--single-above", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "minpoly_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    from clrs_amd.mw import to_limbs
    from tests import minpoly_util as mu
    L = _lib.load()
    h = 32
    rows = []
    for deg in (2, 4):
        bits, eb = mu.generic_bits(deg, h), 2.0 ** -(deg * (h + 8))
        base = mu._planted_roots(deg, 4, 1024, seed=11)
        for limbs in (5, 10):
            base_vals = to_limbs(base, limbs)
            nd = rounding.field_default_digits(bits, limbs)
            for count in args.counts:
                vals = np.ascontiguousarray(np.tile(base_vals, (1, -(-count // base_vals.shape[1])))[:, :count])
                reps = args.repeats if count <= args.single_above else 1
                mu.device_call(limbs, deg, min(count, 64), vals, count, bits, eb, nd)                      # warm-up
                kernel, whole = [], []
                for _ in range(args.repeats):
                    dev = mu.device_call(limbs, deg, count, vals, count, bits, eb, nd)
                    k, w = C.c_double(), C.c_double()
                    assert L.clrs_mw_minpoly_times(C.byref(k), C.byref(w)) == 0
                    kernel.append(k.value / 1e3)
                    whole.append(w.value / 1e3)
                assert (dev[1][:count] == 0).all()
                polys = [rounding._primitive(a) for a in rounding.planes_to_ints(dev[0][:, :, :count]).T]
                lll_s, host_s = [], []
                for _ in range(reps):
                    t = time.perf_counter()
                    rel, status, _, _ = rounding.minpoly_relations_lll(vals, deg, limbs, errbound=eb, bits=bits)
                    lll_s.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    host = mu.host_call(limbs, deg, count, vals, count, bits, eb, nd)
                    host_s.append(time.perf_counter() - t)
                assert (status == 0).all() and [rounding._primitive(a) for a in rel] == polys
                assert all(a[..., :count].tobytes() == b[..., :count].tobytes() for a, b in zip(dev, host))
                row = {"degree": deg, "limbs": limbs, "count": count, "bits": bits, "nd": nd, "kernel_seconds": statistics.median(kernel),
                       "call_seconds": statistics.median(whole), "lll_batch_wall_seconds": statistics.median(lll_s), "host_one_core_wall_seconds": statistics.median(host_s),
                       "device_repeats": args.repeats, "other_repeats": reps, "worst_rung_bits": int(dev[2][:count].max()),
                       "most_exchanges": int(dev[4][0, :count].max()), "mean_exchanges": float(dev[4][0, :count].mean())}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "clrs_mw_minpoly, minpoly_relations_lll and the host build of the header on the same planted numbers, one MI355X; device times by "
                           "device events; medians after a warm-up", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Time of the rounding to a number field by integer relations (clrs_amd.rounding.round_to_field -> clrs_mw_field_round).  Rows:

  planted         batches of 1, 4096 and 65536 planted elements sum_k (n_k / m) g^k, |n_k|, m < 2^16, at degree 2 (x^2 - 5) and 4 (x^4 - x - 1), 4 limbs,
                  errbound 2^-(deg 24): milliseconds in k_mw_field_round over all launches and of the whole call from the first upload to the last download,
                  by device events (clrs_mw_field_round_times), the best of `--repeats` after one warm-up; wall time of `round_to_field` (conversion of the
                  relations to Python integers and Fractions included); the worst rung, rung count and exchange count of the batch.  Beside them, for the
                  batches of 1 and of `--lll-count` numbers, `field_relations_lll` (one clrs_zz_lll call per rung over the numbers still open), wall time
  delsarte        the kernel vectors of delsarte_exact(3, 3, 1/sqrt 5) and delsarte_exact(4, 9, 1/(sqrt 5 - 1)) over QQ(sqrt 5), from solvesdp_mw at 6
                  limbs: every entry of every vector in one call; the same times, and `field_relations_lll` on the same entries

Every planted element must come back (asserted).  Writes profiles/rounding/field_round_times.json.  No time is a pass criterion.

    python scripts/field_round_time.py [--out profiles/rounding/field_round_times.json] [--counts 1 4096 65536] [--lll-count 256]
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
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 4096, 65536])
    ap.add_argument("--lll-count", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "field_round_times.json"))
    args = ap.parse_args()
    import mpmath as mp
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    from clrs_amd.mw import solvesdp_mw
    from tests import field_round_util as fu
    L = _lib.load()

    def timed(values, field, limbs, errbound):
        """(result, kernel s, call s, wall s) of round_to_field without the rescue: the best of the repeats after a warm-up"""
        rounding.round_to_field(values[:, :min(values.shape[1], 64)], field, limbs, errbound=errbound, relations=False)
        best = None
        for _ in range(args.repeats):
            t = time.perf_counter()
            r = rounding.round_to_field(values, field, limbs, errbound=errbound, relations=False)
            wall = time.perf_counter() - t
            k, w = C.c_double(), C.c_double()
            assert L.clrs_mw_field_round_times(C.byref(k), C.byref(w)) == 0
            if best is None or w.value < best[2]:
                best = (r, k.value / 1e3, w.value / 1e3, wall)
        return best

    def lll_wall(values, field, limbs, errbound):
        t = time.perf_counter()
        r = rounding.field_relations_lll(values, field, limbs, errbound=errbound)
        return r, time.perf_counter() - t

    rows = []
    for name, h, limbs in (("x2-5", 16, 4), ("x4-x-1", 16, 4)):
        f = fu.field(name)
        eb = fu.planted_errbound(f.degree, h)
        base_elems, base_vals = fu.planted(name, h, min(max(args.counts), 4096), limbs=limbs, seed=11)
        for count in args.counts:
            reps = -(-count // len(base_elems))
            elems, vals = (base_elems * reps)[:count], np.ascontiguousarray(np.tile(base_vals, (1, reps))[:, :count])
            r, kernel_s, call_s, wall_s = timed(vals, f, limbs, eb)
            assert (r.status == 0).all() and [tuple(c) for c in r.coeffs[:64]] == elems[:64]
            row = {"what": "planted", "field": name, "degree": f.degree, "height_bits": h, "limbs": limbs, "count": count, "kernel_seconds": kernel_s,
                   "call_seconds": call_s, "round_to_field_wall_seconds": wall_s, "worst_rung_bits": int(r.rung.max()), "most_rungs": int(r.rungs.max()),
                   "most_exchanges": int(r.exchanges.max()), "mean_exchanges": float(r.exchanges.mean())}
            if count == 1 or count == min(args.counts[1:] or [count]):
                n = min(count, args.lll_count)
                rl, row["field_relations_lll_wall_seconds"] = lll_wall(vals[:, :n], f, limbs, eb)
                row["field_relations_lll_count"] = n
                assert (rl.status == 0).all() and [tuple(c) for c in rl.coeffs] == elems[:n]
            rows.append(row)
            print(json.dumps(row), flush=True)
    with mp.workprec(400):
        sqrt5 = rounding.NumberField([-5, 0, 1], mp.sqrt(5))
    for name in fu.DELSARTE:
        flat = fu.delsarte_flat(name)
        res = solvesdp_mw(flat, limbs=6, data_limbs=6, duality_gap_threshold=1e-50)
        blocks = rounding.kernel_vectors(flat, res, limbs=6)
        pool = np.concatenate([np.asarray(k.vectors).reshape(6, -1) for k in blocks], axis=1)
        r, kernel_s, call_s, wall_s = timed(pool, sqrt5, 6, 1e-15)
        assert (r.status == 0).all()
        rl, lll_s = lll_wall(pool, sqrt5, 6, 1e-15)
        assert (rl.status == 0).all() and all(tuple(a) == tuple(b) for a, b in zip(r.coeffs, rl.coeffs))
        row = {"what": "delsarte", "problem": name, "degree": 2, "limbs": 6, "count": int(pool.shape[1]), "kernel_seconds": kernel_s, "call_seconds": call_s,
               "round_to_field_wall_seconds": wall_s, "field_relations_lll_wall_seconds": lll_s, "worst_rung_bits": int(r.rung.max()),
               "most_rungs": int(r.rungs.max()), "most_exchanges": int(r.exchanges.max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "rounding.round_to_field and field_relations_lll, one MI355X; device times by device events, the best of %d after a warm-up" % args.repeats,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

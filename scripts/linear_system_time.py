"""Time of the low-rank system assembly on the device (clrs_amd.rounding.lowrank_system -> clrs_zz_lowrank_system).  Per case
(n', R, r, digits): a block of n' rows after the basis change, R constraints of r terms each, operands of `digits` base-2^24 digits, the full triangle of
n' (n' + 1) / 2 columns.

  kernel / whole   one raw call of clrs_zz_lowrank_system: k_lrsys_tile, k_lrsys_carry and the whole call from the first upload to the last download by
                   device events (clrs_zz_lowrank_system_times), the best of `--repeats` after one warm-up call
  lowrank_system   the same through `lowrank_system`, Python included (digit conversion both ways)
  per_row_zz       the same entries by one `zz_matmul` per row, U[:, row] W[:, row]^T with inner extent r -- what the package could do before this kernel;
                   a few rows, multiplied up (`per_row_zz_rows` of them were run)
  fractions        the same entries by Python integers on the host, a few rows, multiplied up

The rows that the host formed are compared with the device result.  Writes profiles/rounding/linear_system_times.json.  A record, no time is a pass
criterion.

    python scripts/linear_system_time.py [--out profiles/rounding/linear_system_times.json] [--repeats 3]
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
CASES = ((16, 64, 1, 4), (64, 256, 1, 4), (64, 256, 4, 9), (128, 512, 2, 9), (256, 128, 1, 4), (128, 128, 5, 30))
ROWS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "linear_system_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    L = _lib.load()
    pi = lambda a: a.ctypes.data_as(_lib.p_i32)
    out = {}
    for n, R, r, nd in CASES:
        rng = np.random.default_rng(n + R + r + nd)
        T = R * r
        Ud = rng.integers(-(1 << 23), 1 << 23, size=(nd, n, T)).astype(np.int32)
        Wd = rng.integers(-(1 << 23), 1 << 23, size=(nd, n, T)).astype(np.int32)
        rowptr = np.arange(0, T + 1, r, dtype=np.int32)
        pairs = [(a, b) for a in range(n) for b in range(a, n)]
        ca, cb = (np.ascontiguousarray(v, dtype=np.int32) for v in zip(*pairs))
        ndc = 2 * nd + 2
        Cd, info = np.zeros((ndc, R, len(pairs)), np.int32), np.zeros(4, np.int32)
        best = None
        for it in range(args.repeats + 1):
            _lib.check(L.clrs_zz_lowrank_system(0, n, T, R, pi(rowptr), nd, pi(Ud), nd, pi(Wd), len(pairs), pi(ca), pi(cb), ndc, pi(Cd), pi(info)))
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            assert L.clrs_zz_lowrank_system_times(C.byref(a), C.byref(b), C.byref(c)) == 0
            if it > 0 and (best is None or c.value < best[2]):
                best = (a.value, b.value, c.value)
        assert info[0] == 0 and info[3] == 0
        products = float(R) * len(pairs) * r * nd * nd
        rec = dict(n=n, R=R, r=r, digits=nd, columns=len(pairs), chunks=int(info[1]), workgroups=int(info[2]), tile_ms=best[0], carry_ms=best[1], whole_ms=best[2],
                   digit_products=products, tile_digit_products_per_second=products / (best[0] * 1e-3))
        U, W = rounding.planes_to_ints(Ud), rounding.planes_to_ints(Wd)
        t = time.perf_counter()
        G = rounding.lowrank_system(U, W, rowptr, pairs)
        rec["lowrank_system_seconds"] = time.perf_counter() - t
        rows = min(ROWS, R)
        t = time.perf_counter()
        per_row = [rounding.zz_matmul(U[:, rowptr[i]:rowptr[i + 1]], np.ascontiguousarray(W[:, rowptr[i]:rowptr[i + 1]].T)) for i in range(rows)]
        rec["per_row_zz_seconds"] = (time.perf_counter() - t) / rows * R
        rec["per_row_zz_rows"] = rows
        t = time.perf_counter()
        host = [U[:, rowptr[i]:rowptr[i + 1]].dot(W[:, rowptr[i]:rowptr[i + 1]].T) for i in range(rows)]
        rec["fractions_seconds"] = (time.perf_counter() - t) / rows * R
        rec["verified"] = bool(all(int(G[i, c]) == (1 if a == b else 2) * int(host[i][a, b]) == (1 if a == b else 2) * int(per_row[i][a, b])
                                   for i in range(rows) for c, (a, b) in enumerate(pairs)))
        out[f"n{n}_R{R}_r{r}_d{nd}"] = rec
        print(json.dumps({f"n{n}_R{R}_r{r}_d{nd}": rec}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

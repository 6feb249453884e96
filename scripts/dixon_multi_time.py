"""Time of the exact inverse over QQ on the device (clrs_amd.rounding.inverse_qq -> clrs_modp_dixon_lift_multi).  Per size n, for a
random n x n matrix with one-digit entries (|a| <= 99) and the identity as right-hand sides, K = dixon_steps at p = 8388593:

  lift_multi      one raw call of clrs_modp_dixon_lift_multi, all n columns: k_liftm_x, k_zz_gemm, k_liftm_r over all steps and the whole call from the first
                  upload to the last download by device events (clrs_modp_dixon_lift_multi_times), the best of `--repeats` after one warm-up call
  lift_single     the same lifting by the single-column clrs_modp_dixon_lift, which has no event times: wall-clock time of COLUMNS = 4 calls (columns e_0 ...
                  e_3), the best of `--repeats` after a warm-up, multiplied up to n columns (`*_extrapolated`); the lifted residues of those columns are
                  compared with the matrix call's
  inverse_qq      the whole front end, Python included (digit conversion, device reconstruction in pieces, Fractions), without the checks, for n up to
                  `--full-max-n` (the host side of it grows with n^2 K-digit integers and is not what this script is about)

Writes profiles/rounding/dixon_multi_times.json.  No time is a pass criterion.

    python scripts/dixon_multi_time.py [--out profiles/rounding/dixon_multi_times.json] [--sizes 64 256 1024] [--repeats 3] [--full-max-n 256]
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
P = 8388593
COLUMNS = 4


def best_of(fn, repeats):
    fn()                                                          # warm-up
    best = None
    for _ in range(repeats):
        out = fn()
        best = out if best is None or out["whole"] < best["whole"] else best
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "dixon_multi_times.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--full-max-n", type=int, default=256)
    args = ap.parse_args()
    from clrs_amd import _lib, rounding
    L = _lib.load()
    results = []
    for n in args.sizes:
        rng = np.random.default_rng(n)
        A = rng.integers(-99, 100, size=(n, n))
        eye = np.eye(n, dtype=np.int64)
        K = rounding.dixon_steps(A, eye[:, 0], P)[0]
        Ad, Bl = rounding.ints_to_planes(A), rounding.ints_to_planes(eye)
        keep = {}

        def multi():
            t0 = time.perf_counter()
            X, R, info = rounding._dixon_lift_multi_digits(Ad, Bl, P, K)
            wall = time.perf_counter() - t0
            assert info.tolist()[0] == n and info.tolist()[2:4] == [0, 0] and info[5] == 0, info
            t = [C.c_double() for _ in range(4)]
            _lib.check(L.clrs_modp_dixon_lift_multi_times(*[C.byref(v) for v in t]))
            keep["X"], keep["chunks"] = X[:, :, :COLUMNS].copy(), int(info[4])
            return {"k_liftm_x_ms": t[0].value, "k_zz_gemm_ms": t[1].value, "k_liftm_r_ms": t[2].value, "whole": t[3].value, "wall_ms": 1e3 * wall}

        def single():
            t0 = time.perf_counter()
            for j in range(COLUMNS):
                X, r, info = rounding._dixon_lift_digits(Ad, np.ascontiguousarray(Bl[:, :, j]), P, K)
                assert info.tolist() == [n, K, 0, 0] and np.array_equal(X, keep["X"][:, :, j])
            return {"whole": 1e3 * (time.perf_counter() - t0)}

        m = best_of(multi, args.repeats)
        s = best_of(single, args.repeats)
        row = {"n": n, "m": n, "steps": K, "chunks": keep["chunks"],
               "lift_multi": {"k_liftm_x_ms": m["k_liftm_x_ms"], "k_zz_gemm_ms": m["k_zz_gemm_ms"], "k_liftm_r_ms": m["k_liftm_r_ms"], "whole_ms": m["whole"],
                              "wall_ms": m["wall_ms"]},
               "lift_single": {"columns_timed": COLUMNS, "wall_ms_of_those": s["whole"], "wall_ms_extrapolated": s["whole"] * n / COLUMNS,
                               "note": "wall-clock time of %d single-column calls multiplied by n / %d" % (COLUMNS, COLUMNS)}}
        row["single_over_multi"] = row["lift_single"]["wall_ms_extrapolated"] / m["wall_ms"]
        if n <= args.full_max_n:
            def full():
                t0 = time.perf_counter()
                rounding.inverse_qq(A, check=False, reconstruct=rounding.dixon_reconstruct)
                return {"whole": 1e3 * (time.perf_counter() - t0)}
            row["inverse_qq_wall_ms"] = best_of(full, args.repeats)["whole"]
        print(json.dumps(row), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"p": P, "entries": "uniform in [-99, 99]", "repeats": args.repeats, "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

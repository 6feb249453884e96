"""Time of the multi-word SPD solve (clrs_amd.mw.posv -> clrs_mw_posv) at 5 limbs on random symmetric positive definite systems
with one right-hand side, n = 64, 256, 1024.  Per size, the best of `--repeats` after a warm-up call:

  posv            the launches of one call by device events (clrs_mw_posv_times): all of them, the diagonal launches (k_mw_posv_diag, n / 16 of them, one
                  workgroup each), and the rest (the k_mw_gemm launches); beside it the wall time of `mw.posv` (conversions, copies and the call)
  rank_reveal     what the library could do before: `mw.rank_reveal` on the bordered matrix [[M, r], [r^T, 0]] with ncand = n (one workgroup eliminates the
                  whole matrix; W = M^-1 r), for n <= `--rank-reveal-max-n`: device events around the call on the null stream (copies included) and its wall time
  mpmath          `mpmath.cholesky_solve` at 53 bits per limb, for n <= `--mpmath-max-n`, wall time

The two device solutions must agree to 2^-200 of the largest entry (asserted).  Writes profiles/rounding/posv_times.json.  No time is a pass criterion.

    python scripts/posv_time.py [--out profiles/rounding/posv_times.json] [--sizes 64 256 1024] [--mpmath-max-n 256] [--rank-reveal-max-n 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_system(seed, n, limbs):
    """planar (limbs, n, n) SPD and (limbs, n, 1): G^T G / n + I from an fp64 G, formed in double-double and padded with zero limbs (exactly representable
    inputs: the three solvers see the same matrix)"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    M = G.T @ G / n + np.eye(n)
    M = (M + M.T) / 2
    A, B = np.zeros((limbs, n, n)), np.zeros((limbs, n, 1))
    A[0], B[0, :, 0] = M, rng.standard_normal(n)
    A[1] = (rng.standard_normal((n, n)) * 2.0 ** -60 * np.abs(M))
    A[1] = (A[1] + A[1].T) / 2
    return A, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limbs", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--mpmath-max-n", type=int, default=256)
    ap.add_argument("--rank-reveal-max-n", type=int, default=256, help="one workgroup eliminates the whole bordered matrix: n^3 / 3 steps on one compute unit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "posv_times.json"))
    args = ap.parse_args()
    import mpmath as mp
    import torch
    import clrs_amd  # noqa: F401
    from clrs_amd import mw
    K = args.limbs
    mw.posv_times()                                             # from here on this thread's calls record the events around the diagonal launches
    rows = []
    for n in args.sizes:
        A, B = random_system(n, n, K)
        mw.posv(A, B, K)                                        # warm-up
        best = None
        for _ in range(args.repeats):
            t = time.perf_counter()
            X, info = mw.posv(A, B, K)
            wall = time.perf_counter() - t
            d, g, w = mw.posv_times()
            if best is None or w < best[2]:
                best = (d, g, w, wall)
        row = {"n": n, "limbs": K, "panels": int(info[1]), "posv_launches_ms": best[2], "posv_diag_ms": best[0], "posv_gemm_ms": best[1],
               "posv_diag_ms_per_panel": best[0] / int(info[1]), "posv_wall_seconds": best[3], "rank_reveal_event_ms": None, "rank_reveal_wall_seconds": None,
               "mpmath_wall_seconds": None}
        # the bordered matrix, column-major (symmetric: row-major is the same)
        Gb = np.zeros((K, n + 1, n + 1))
        Gb[:, :n, :n], Gb[:, :n, n:], Gb[:, n:, :n] = A, B, np.transpose(B, (0, 2, 1))
        Gp = np.ascontiguousarray(np.transpose(Gb, (0, 2, 1)).reshape(K, -1))
        if n > args.rank_reveal_max_n:
            row["rank_reveal_skipped"] = "n above --rank-reveal-max-n"
        else:
            mw.rank_reveal(Gp, [n + 1], [n], [1e-300], K)      # warm-up
            rr = None
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                e0.record()
                (perm, r, W, resid), = mw.rank_reveal(Gp, [n + 1], [n], [1e-300], K)
                e1.record()
                e1.synchronize()
                wall = time.perf_counter() - t
                ms = e0.elapsed_time(e1)
                if rr is None or ms < rr[0]:
                    rr = (ms, wall)
            assert r == n and list(perm[:n]) != [] and int(perm[n]) == n
            xr = np.zeros((K, n))
            xr[:, np.asarray(perm[:n], dtype=int)] = W[:, :n]
            diff = np.max(np.abs(mw.from_limbs(xr - X[:, :, 0]).astype(float)))
            assert diff <= 2.0 ** -200 * np.max(np.abs(X[0])), diff
            row["rank_reveal_event_ms"], row["rank_reveal_wall_seconds"] = rr
        if n <= args.mpmath_max_n:
            with mp.workprec(53 * K):
                Am = mp.matrix(n, n)
                for i in range(n):
                    for j in range(n):
                        Am[i, j] = mp.mpf(float(A[0, i, j])) + mp.mpf(float(A[1, i, j]))
                bm = mp.matrix([mp.mpf(float(v)) for v in B[0, :, 0]])
                t = time.perf_counter()
                xm = mp.cholesky_solve(Am, bm)
                row["mpmath_wall_seconds"] = time.perf_counter() - t
                got = mw.from_limbs(np.ascontiguousarray(X[:, :, 0]))
                assert max(abs(got[i] - xm[i]) for i in range(n)) <= mp.mpf(2) ** (-53 * K + 40) * max(abs(v) for v in xm)
        rows.append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"what": "mw.posv against mw.rank_reveal on the bordered matrix and mpmath.cholesky_solve, %d limbs, one right-hand side, one MI355X; "
                               "the best of %d after a warm-up; posv_*_ms by device events inside the call (clrs_mw_posv_times)" % (K, args.repeats),
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

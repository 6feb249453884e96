"""Wall time of the exact solve by Dixon's p-adic lifting on the device (clrs_amd.rounding -> clrs_modp_dixon_lift): random systems
of n = 256, 1024, 2048 with two-digit entries (|a| < 2^46) at p = 8388593, K steps from the bound (`dixon_steps`).  Per system, separately:

  inverse         one whole call with steps = 0 (`steps0_call_seconds`): the host's scan of the digits, the upload of the digit planes, [A mod p | I], the
                  elimination, the gather of A^-1 mod p and the copies back
  lifting loop    one whole call with steps = K (`stepsK_call_seconds`) minus the above (`lifting_seconds_by_difference`), in total and per step (two
                  launches per step); a difference of two best-of-three calls, not a timed loop
  reconstruction  what `solve_dixon` does on the host per entry: Horner over the K digits and the half-extended Euclid, in Python integers; at n > 256 timed
                  on three entries and multiplied up (`reconstruction_entries_timed` says on how many)

each the best of three after one warm-up call.  The lifted integers are checked with A x == b - p^K r (x by a pairwise Horner, not timed).  Beside these
the Python restatement of the tests (tests/dixon_util.lift): timed on sixteen steps, and run in full where that predicts less than a minute.  Writes
profiles/rounding/dixon_times.json.  No time is a pass criterion.

    python scripts/dixon_time.py [--out profiles/rounding/dixon_times.json] [--sizes 256 1024 2048]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = 8388593
BITS = 46
HOST_LIMIT = 60.0


def best_of(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def horner_pairwise(X, p):
    """sum_k X[k] p^k per column as Python integers, pairing neighbours level by level (large products instead of K small ones)"""
    vals, q = [X[k].astype(object) for k in range(X.shape[0])], p
    while len(vals) > 1:
        if len(vals) % 2:
            vals.append(np.zeros(X.shape[1], dtype=object))
        vals = [vals[i] + q * vals[i + 1] for i in range(0, len(vals), 2)]
        q = q * q
    return vals[0] if vals else np.zeros(X.shape[1], dtype=object)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "dixon_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import rounding
    from tests import dixon_util as du
    out = {}
    for n in args.sizes:
        rng = np.random.default_rng(n)
        while True:                                             # redrawn until invertible mod p (the device says)
            A = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=(n, n), dtype=np.int64)
            b = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=n, dtype=np.int64)
            Ad, bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(b)
            if int(rounding._dixon_lift_digits(Ad, bl, P, 0)[2][0]) == n:          # (also the warm-up: the first call loads the code objects)
                break
        Ao, bo = A.astype(object), b.astype(object)
        K, N, D = rounding.dixon_steps(Ao, bo, P)
        rounding._dixon_lift_digits(Ad, bl, P, min(K, 8))                            # warm-up of the lifting kernels
        t_inv, _ = best_of(lambda: rounding._dixon_lift_digits(Ad, bl, P, 0), args.repeats)
        t_all, (X, r, info) = best_of(lambda: rounding._dixon_lift_digits(Ad, bl, P, K), args.repeats)
        assert info.tolist() == [n, K, 0, 0]
        rec = dict(n=n, p=P, digits=int(Ad.shape[0]), steps=K, steps0_call_seconds=t_inv, stepsK_call_seconds=t_all, lifting_seconds_by_difference=t_all - t_inv,
                   lifting_seconds_per_step_by_difference=(t_all - t_inv) / K, launches=2 * K)
        m = P ** K
        x = horner_pairwise(X, P)
        rK = rounding.from_balanced_digits(r)
        rec["lifted_integers_verified"] = bool(all(int(v) == int(w) for v, w in zip(Ao.dot(x), bo - m * rK)))
        # the host's reconstruction as solve_dixon does it
        entries = list(range(n)) if n <= 256 else [0, n // 2, n - 1]
        t = time.perf_counter()
        sol = {}
        for i in entries:
            v = 0
            for k in range(K - 1, -1, -1):
                v = v * P + int(X[k, i])
            assert v == int(x[i])
            sol[i] = rounding.rational_reconstruction(v, m, N, D)
        dt = time.perf_counter() - t
        rec.update(reconstruction_entries_timed=len(entries), reconstruction_seconds_per_entry=dt / len(entries),
                   reconstruction_seconds_all_entries=dt / len(entries) * n, reconstruction_extrapolated=len(entries) < n,
                   reconstructed=bool(all(v is not None for v in sol.values())))
        if len(entries) == n:                                   # every entry in hand: the solution itself
            L = 1                                               # A sol == b in every row, cleared of the denominators: A (sol L) == b L
            for v in sol.values():
                L = L * v.denominator // math.gcd(L, v.denominator)
            y = np.array([sol[j].numerator * (L // sol[j].denominator) for j in range(n)], dtype=object)
            rec["solution_verified"] = bool(all(int(v) == int(w) * L for v, w in zip(Ao.dot(y), bo)))
        # the restatement of the tests
        if n <= 1024:
            t = time.perf_counter()
            _, rank = du.inverse_mod_p(Ao, P)
            t_rinv = time.perf_counter() - t
            t = time.perf_counter()
            X4 = du.lift(Ao, bo, P, 16)[0]                      # (its own inverse again, then sixteen steps)
            t4 = max(time.perf_counter() - t - t_rinv, 0.0) / 16
            rec.update(restatement_inverse_seconds=t_rinv, restatement_seconds_per_step=t4, restatement_first_steps_equal=bool(np.array_equal(X4, X[:16])))
            if t_rinv + t4 * K < HOST_LIMIT:
                t = time.perf_counter()
                Xr, rr, _ = du.lift(Ao, bo, P, K)
                rec["restatement_seconds"] = time.perf_counter() - t
                rec["restatement_equal"] = bool(np.array_equal(Xr, X) and [int(v) for v in rK] == rr)
            else:
                rec["restatement_seconds"] = None
                rec["restatement_estimate_seconds"] = t_rinv + t4 * K
        else:
            rec["restatement_seconds"] = None                   # its inverse alone (numpy, n^3) is past the minute
        out[f"n{n}"] = rec
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

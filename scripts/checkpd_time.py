"""Time of the exact positive-definiteness check (clrs_amd.rounding.checkpd -> clrs_modp_minors) on blocks B^T B + I, B a random integer
matrix: n = 16, 64, 128 with entries of about 500 and 2000 bits.  Per block:

  primes          how many primes below 2^23 the Hadamard bound of the last minor asks for (`primes`), and the bits of that bound
  device          one raw call of clrs_modp_minors with those primes: the residue kernel, the L D L^T kernel and the whole call from the first upload to
                  the last download by device events (clrs_modp_minors_times), the best of `--repeats` after one warm-up call; beside it the wall time of
                  `leading_minors_mod` (digit conversion on the host included)
  host            `minor_bounds`, and `crt_tree` on all n minors over one product tree (`crt_seconds`)
  whole           `checkpd(A)` as a whole, wall time
  bareiss         the exact leading minors by Bareiss' fraction-free elimination on Python integers in the same run, for comparison.  It is stopped after
                  `--bareiss-budget` seconds; the figure is then EXTRAPOLATED (`bareiss_extrapolated: true`) from the steps done by the operation count,
                  step k weighing (n - k - 1)^2 (k + 1)^1.585 (entries of k + 1 times the bits, Karatsuba products)

Where Bareiss ran to the end its minors must equal those of the certificate (asserted); the certificate must say `pd` for every block.  Writes
profiles/rounding/checkpd_times.json.  No time is a pass criterion.

    python scripts/checkpd_time.py [--out profiles/rounding/checkpd_times.json] [--sizes 16 64 128] [--bits 500 2000]
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


def block(seed, n, bits):
    rng = np.random.default_rng(seed)
    half = bits // 2
    B = [[int.from_bytes(rng.bytes((half + 7) // 8), "little") % (1 << half) - (1 << (half - 1)) for _ in range(n)] for _ in range(n)]
    return [[sum(B[k][i] * B[k][j] for k in range(n)) + (1 if i == j else 0) for j in range(n)] for i in range(n)]


def bareiss(M, budget):
    """(minors or None, seconds, extrapolated)"""
    n = len(M)
    a = [row[:] for row in M]
    out, prev = [], 1
    weight = lambda k: (n - k - 1) ** 2 * (k + 1) ** 1.585
    t0 = time.perf_counter()
    for k in range(n):
        out.append(a[k][k])
        ak = a[k]
        for i in range(k + 1, n):
            ai, f = a[i], a[i][k]
            for j in range(k + 1, n):
                ai[j] = (ai[j] * ak[k] - f * ak[j]) // prev
        prev = ak[k]
        dt = time.perf_counter() - t0
        if dt > budget and k + 1 < n - 1:
            return None, dt * sum(weight(j) for j in range(n)) / sum(weight(j) for j in range(k + 1)), True
    return out, time.perf_counter() - t0, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 64, 128])
    ap.add_argument("--bits", type=int, nargs="*", default=[500, 2000])
    ap.add_argument("--bareiss-budget", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "checkpd_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    L = _lib.load()
    rows = []
    for n in args.sizes:
        for bits in args.bits:
            M = block(1000 * n + bits, n, bits)
            t = time.perf_counter()
            H = rounding.minor_bounds(M)
            t_bounds = time.perf_counter() - t
            primes, prod = [], 1
            for p in rounding._primes_descending():
                if prod > 2 * H[-1]:
                    break
                primes.append(int(p))
                prod *= int(p)
            rounding.leading_minors_mod(M, primes)                                      # warm-up
            best = None
            for _ in range(args.repeats):
                t = time.perf_counter()
                minors, brk = rounding.leading_minors_mod(M, primes)
                wall = time.perf_counter() - t
                a, b, c = C.c_double(), C.c_double(), C.c_double()
                assert L.clrs_modp_minors_times(C.byref(a), C.byref(b), C.byref(c)) == 0
                if best is None or c.value < best[2]:
                    best = (a.value, b.value, c.value, wall)
            info = list(rounding.leading_minors_mod.last_info)
            clean = [q for q in range(len(primes)) if brk[q] == 0]
            t = time.perf_counter()
            values, _ = rounding.crt_tree(minors[clean].astype(np.int64), [primes[q] for q in clean])
            t_crt = time.perf_counter() - t
            t = time.perf_counter()
            cert = rounding.checkpd(M)
            t_whole = time.perf_counter() - t
            assert cert.pd and len(cert.minors) == n
            if len(clean) == len(primes):
                assert values == cert.minors
            exact, t_bareiss, extrapolated = bareiss(M, args.bareiss_budget)
            if exact is not None:
                assert exact == cert.minors
            row = {"n": n, "entry_bits": max(int(v).bit_length() for r in M for v in r), "bound_bits": int(H[-1]).bit_length(), "primes": len(primes),
                   "primes_of_checkpd": len(cert.primes), "discarded": len(cert.discarded), "lds_bytes": info[0], "workgroups": info[1],
                   "residue_kernel_seconds": best[0] / 1e3, "ldl_kernel_seconds": best[1] / 1e3, "raw_call_seconds": best[2] / 1e3,
                   "leading_minors_mod_wall_seconds": best[3], "minor_bounds_seconds": t_bounds, "crt_seconds": t_crt, "checkpd_wall_seconds": t_whole,
                   "bareiss_seconds": t_bareiss, "bareiss_extrapolated": extrapolated, "bareiss_equal": exact is not None}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "rounding.checkpd on blocks B^T B + I, one MI355X; device times by device events, the best of %d after a warm-up" % args.repeats,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

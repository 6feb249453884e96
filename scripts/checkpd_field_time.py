"""Time of the exact positive-definiteness check over a number field (clrs_amd.rounding.checkpd_field -> clrs_modp_minors_field, clrs_modp_field_frobenius;
DESIGN.md section 24) on blocks B^T B + I, B a random matrix over Z[g] with coefficients of about 20 bits: n = 16, 64, 128 over QQ(sqrt 5) (degree 2, half
of the primes split) and QQ(g), g^4 = g + 1 (degree 4, one prime in 24 splits).  Per block:

  primes          how many split primes the coefficient bound of `field_minor_bounds` asks for, and the bits of that bound
  scan            `split_primes` for that many primes: on the host (x^p on Python integers, prime by prime) and on the device (`field_frobenius`, 4096 primes
                  per call), the roots by Cantor-Zassenhaus on the host in both; the two must return the same primes and roots (asserted)
  device          one raw call of clrs_modp_minors_field with those primes: the residue kernel, the L D L^T kernel and the whole call by device events
                  (clrs_modp_minors_field_times), the best of `--repeats` after a warm-up call; beside it the wall time of `leading_minors_field_mod`
  host            `field_minor_bounds`; inside one `checkpd_field` with the primes at hand: the seconds in `crt_tree` and the rest of the host's work
                  (Vandermonde solves, signs by interval arithmetic), and the wall time of the whole call
  stand-in        the same raw call through the host stand-in of the tests (tests/pd_field_util.host_field_minors: M(r) mod p and the elimination on Python
                  integers), measured on `--stand-in-primes` primes and EXTRAPOLATED to all of them by the pair count (`stand_in_extrapolated: true`)

Per field, once: every prime below 2^23 (564163) through `field_frobenius` in one call (wall time) beside the host's rate measured in the scan above and
extrapolated to the same count.  The certificate must say `pd` for every block.  Writes profiles/rounding/checkpd_field_times.json.  No time is a pass criterion.

    python scripts/checkpd_field_time.py [--out profiles/rounding/checkpd_field_times.json] [--sizes 16 64 128]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = {"x2-5": ([-5, 0, 1], "sqrt(5)"), "x4-x-1": ([-1, -1, 0, 0, 1], "findroot(lambda x: x**4 - x - 1, 1.2)")}


def block(seed, f, n, bits=20):
    """the d coefficient matrices (int64) of B^T B + I, B = sum_j B_j g^j with random B_j below 2^bits, f monic"""
    d = len(f) - 1
    rng = np.random.default_rng(seed)
    B = [rng.integers(-(1 << bits), 1 << bits, size=(n, n), dtype=np.int64) for _ in range(d)]
    T = [np.zeros((n, n), np.int64) for _ in range(2 * d - 1)]
    for i in range(d):
        for j in range(d):
            T[i + j] += B[i].T @ B[j]
    for k in range(2 * d - 2, d - 1, -1):                             # g^k = -sum_j f_j g^(k - d + j)
        for j in range(d):
            T[k - d + j] -= T[k] * f[j]
    T[0] += np.eye(n, dtype=np.int64)
    return [t.astype(object) for t in T[:d]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 64, 128])
    ap.add_argument("--stand-in-primes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "checkpd_field_times.json"))
    args = ap.parse_args()
    import mpmath as mp
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    from tests import pd_field_util as fu
    L = _lib.load()
    rows, scans = [], []
    every = [int(p) for p in rounding._primes_descending()]
    for name, (f, root) in FIELDS.items():
        d = len(f) - 1
        with mp.workprec(700):
            fld = rounding.NumberField(f, eval("mp." + root, {"mp": mp}))
        host_rate = None
        for n in args.sizes:
            M = block(1000 * n + d, f, n)
            A = [[tuple(Fraction(int(M[c][i, j])) for c in range(d)) for j in range(n)] for i in range(n)]
            t = time.perf_counter()
            bounds = rounding.field_minor_bounds(M, fld)
            t_bounds = time.perf_counter() - t
            count = -(-(2 * max(bounds)).bit_length() // 22)
            t = time.perf_counter()
            dev_scan = rounding.split_primes(fld, count, frobenius=rounding.field_frobenius)
            t_dev_scan = time.perf_counter() - t
            t = time.perf_counter()
            host_scan = rounding.split_primes(fld, count)
            t_host_scan = time.perf_counter() - t
            assert dev_scan == host_scan
            primes, roots = host_scan
            tested = every.index(primes[-1]) + 1                    # primes the host scan had to test
            host_rate = tested / t_host_scan
            rounding.leading_minors_field_mod(M, primes, roots)     # warm-up
            best = None
            for _ in range(args.repeats):
                t = time.perf_counter()
                minors, brk = rounding.leading_minors_field_mod(M, primes, roots)
                wall = time.perf_counter() - t
                a, b, c = C.c_double(), C.c_double(), C.c_double()
                assert L.clrs_modp_minors_field_times(C.byref(a), C.byref(b), C.byref(c)) == 0
                if best is None or c.value < best[2]:
                    best = (a.value, b.value, c.value, wall)
            info = list(rounding.leading_minors_field_mod.last_info)
            spent = {"crt": 0.0, "minors": 0.0}
            real_crt = rounding.crt_tree

            def timed_crt(*a_, **k_):
                t0 = time.perf_counter()
                try:
                    return real_crt(*a_, **k_)
                finally:
                    spent["crt"] += time.perf_counter() - t0

            def timed_minors(*a_, **k_):
                t0 = time.perf_counter()
                try:
                    return rounding.leading_minors_field_mod(*a_, **k_)
                finally:
                    spent["minors"] += time.perf_counter() - t0

            def at_hand(field, cnt, start=None):
                at = 0 if start is None else primes.index(start) + 1
                if at + cnt <= len(primes):
                    return primes[at:at + cnt], roots[at:at + cnt]
                return rounding.split_primes(field, cnt, start, frobenius=rounding.field_frobenius)
            rounding.crt_tree = timed_crt
            try:
                t = time.perf_counter()
                cert = rounding.checkpd_field(A, fld, minors=timed_minors, primes=at_hand)
                t_whole = time.perf_counter() - t
            finally:
                rounding.crt_tree = real_crt
            assert cert.pd and len(cert.minors) == n
            k = min(args.stand_in_primes, len(primes))
            t = time.perf_counter()
            sm, sb = fu.host_field_minors(M, primes[:k], roots[:k])
            t_stand = time.perf_counter() - t
            assert np.array_equal(sm, minors[:k]) and np.array_equal(sb, brk[:k])
            row = {"field": name, "degree": d, "n": n, "entry_bits": max(int(abs(v)).bit_length() for m in M for v in m.flat),
                   "bound_bits": int(max(bounds)).bit_length(), "primes": len(primes), "primes_of_checkpd_field": len(cert.primes), "discarded_pairs": len(cert.discarded),
                   "lds_bytes": info[0], "workgroups": info[1], "scan_primes_tested": tested, "scan_host_seconds": t_host_scan, "scan_device_seconds": t_dev_scan,
                   "residue_kernel_seconds": best[0] / 1e3, "ldl_kernel_seconds": best[1] / 1e3, "raw_call_seconds": best[2] / 1e3,
                   "leading_minors_field_mod_wall_seconds": best[3], "field_minor_bounds_seconds": t_bounds, "crt_seconds": spent["crt"],
                   "host_rest_seconds": t_whole - spent["crt"] - spent["minors"] - t_bounds, "checkpd_field_wall_seconds": t_whole,
                   "stand_in_primes_measured": k, "stand_in_seconds_measured": t_stand, "stand_in_seconds": t_stand * len(primes) / k, "stand_in_extrapolated": k < len(primes)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        rounding.field_frobenius(f, every[:4096])                    # warm-up
        t = time.perf_counter()
        got = rounding.field_frobenius(f, every)
        t_all = time.perf_counter() - t
        split = int(np.count_nonzero(np.all(got == np.array([0, 1] + [0] * (d - 2), np.int32), axis=1)))
        scan = {"field": name, "degree": d, "primes_below_2^23": len(every), "with_x^p_equal_x": split, "share": split / len(every),
                "device_seconds_one_call_wall": t_all, "host_primes_per_second_measured": host_rate, "host_seconds": len(every) / host_rate, "host_extrapolated": True}
        scans.append(scan)
        print(json.dumps(scan), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"what": "rounding.checkpd_field on blocks B^T B + I over Z[g], one MI355X; device times by device events, the best of %d after a warm-up; "
                           "scans and host parts by wall clock" % args.repeats, "rows": rows, "whole_range_scans": scans}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

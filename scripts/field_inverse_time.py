"""Time of the exact inverse over a number field (clrs_amd.rounding.inverse_field -> clrs_modp_field_adjugate) on random square
matrices over Z[g] with coefficients of 64 bits: n = 16, 64, 128 over QQ(sqrt 5) (degree 2) and QQ(g), g^4 = g + 1 (degree 4).  Per matrix:

  primes          how many split primes the coefficient bound of `field_adjugate_bounds` asks for (the fewest whose product exceeds twice the bound), and the
                  bits of that bound; they are drawn once, on the device (`split_primes(frobenius=field_frobenius)`), outside every time below
  device          one raw call of clrs_modp_field_adjugate with those primes: the residue kernel, the Gauss-Jordan kernel and the whole call by device
                  events (clrs_modp_field_adjugate_times), the best of `--repeats` after a warm-up call; beside it the wall time of `field_adjugate_mod`,
                  the Gauss-Jordan kernel's time divided by the pairs (throughput), and its time in a call with ONE prime (the latency of a pair)
  inverse_field   the wall time of one `inverse_field(B, field, matmul=zz_matmul)` with the primes at hand, and inside it the seconds in the device call, in
                  `crt_tree` and in the exact check M adj M = det M I
  inverse_qq      the wall time of `inverse_qq(..., reconstruct=dixon_reconstruct, matmul=zz_matmul)` on the n d x n d regular representation of the same
                  matrix (every entry its d x d multiplication matrix), where n d <= `--qq-max-n`; the two inverses must agree (asserted)

Writes profiles/rounding/field_inverse_times.json.  No time is a pass criterion.

    python scripts/field_inverse_time.py [--out profiles/rounding/field_inverse_times.json] [--sizes 16 64 128] [--qq-max-n 128]
"""
import argparse
import ctypes as C
import functools
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = {"x2-5": ([-5, 0, 1], "sqrt(5)"), "x4-x-1": ([-1, -1, 0, 0, 1], "findroot(lambda x: x**4 - x - 1, 1.2)")}


def random_planes(seed, d, n, bits):
    """d random integer matrices (object arrays), entries below 2^bits in size"""
    rng = np.random.default_rng(seed)
    draw = lambda: (int.from_bytes(rng.bytes(bits // 8), "little") >> 1) * (1 if rng.integers(2) else -1)
    return [np.array([[draw() for _ in range(n)] for _ in range(n)], dtype=object) for _ in range(d)]


def regular_representation(M, f):
    """the n d x n d rational matrix of the n x n matrix sum_c M_c g^c: every entry its matrix of multiplication on the basis 1, g, .., g^(d-1) (f monic)"""
    d, n = len(M), M[0].shape[0]
    comp = np.zeros((d, d), dtype=object)                             # the companion matrix of f: column j the coordinates of g g^j
    for j in range(d - 1):
        comp[j + 1, j] = 1
    for i in range(d):
        comp[i, d - 1] = -f[i]
    powers = [np.array([[int(i == j) for j in range(d)] for i in range(d)], dtype=object)]
    for _ in range(d - 1):
        powers.append(comp.dot(powers[-1]))
    out = np.zeros((n * d, n * d), dtype=object)
    for c in range(d):
        out += np.kron(M[c], powers[c])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 64, 128])
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--qq-max-n", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "field_inverse_times.json"))
    args = ap.parse_args()
    import mpmath as mp
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    L = _lib.load()
    rows = []
    for name, (f, root) in FIELDS.items():
        d = len(f) - 1
        with mp.workprec(700):
            fld = rounding.NumberField(f, eval("mp." + root, {"mp": mp}))
        scan = functools.partial(rounding.split_primes, frobenius=rounding.field_frobenius)
        for n in args.sizes:
            M = random_planes(1000 * n + d, d, n, args.bits)
            B = [[tuple(Fraction(int(M[c][i, j])) for c in range(d)) for j in range(n)] for i in range(n)]
            t = time.perf_counter()
            bound = rounding.field_adjugate_bounds(M, fld)
            t_bound = time.perf_counter() - t
            count = max(1, -(-(2 * bound).bit_length() // 23))
            primes, roots = scan(fld, count)
            while rounding._product(primes) <= 2 * bound:
                primes, roots = scan(fld, len(primes) + 1)
            rounding.field_adjugate_mod(M, primes, roots)            # warm-up
            best = None
            for _ in range(args.repeats):
                t = time.perf_counter()
                adj, det, brk = rounding.field_adjugate_mod(M, primes, roots)
                wall = time.perf_counter() - t
                a, b, c = C.c_double(), C.c_double(), C.c_double()
                assert L.clrs_modp_field_adjugate_times(C.byref(a), C.byref(b), C.byref(c)) == 0
                if best is None or c.value < best[2]:
                    best = (a.value, b.value, c.value, wall)
            info = list(rounding.field_adjugate_mod.last_info)
            alone = None                                             # one prime: its d workgroups run side by side, the kernel's time is that of one pair
            for _ in range(args.repeats):
                rounding.field_adjugate_mod(M, primes[:1], roots[:1])
                a, b, c = C.c_double(), C.c_double(), C.c_double()
                assert L.clrs_modp_field_adjugate_times(C.byref(a), C.byref(b), C.byref(c)) == 0
                alone = b.value if alone is None else min(alone, b.value)
            spent = {"crt": 0.0, "adjugate": 0.0, "check": 0.0}

            def timed(key, fn):
                def wrapped(*a_, **k_):
                    t0 = time.perf_counter()
                    try:
                        return fn(*a_, **k_)
                    finally:
                        spent[key] += time.perf_counter() - t0
                return wrapped

            def at_hand(field, cnt, start=None):
                at = 0 if start is None else primes.index(start) + 1
                if at + cnt <= len(primes):
                    return primes[at:at + cnt], roots[at:at + cnt]
                return scan(field, cnt, start)
            real_crt, real_matmul = rounding.crt_tree, rounding.field_matmul
            rounding.crt_tree, rounding.field_matmul = timed("crt", real_crt), timed("check", real_matmul)
            try:
                t = time.perf_counter()
                result = rounding.inverse_field(B, fld, adjugate=timed("adjugate", rounding.field_adjugate_mod), primes=at_hand, matmul=rounding.zz_matmul)
                t_whole = time.perf_counter() - t
            finally:
                rounding.crt_tree, rounding.field_matmul = real_crt, real_matmul
            row = {"field": name, "degree": d, "n": n, "entry_bits": max(int(abs(v)).bit_length() for m in M for v in m.flat),
                   "bound_bits": int(bound).bit_length(), "primes": len(primes), "primes_of_inverse_field": len(result.primes), "discarded_primes": len(result.discarded),
                   "pairs": info[1], "singular_pairs": info[2], "lds_bytes": info[0],
                   "residue_kernel_seconds": best[0] / 1e3, "gj_kernel_seconds": best[1] / 1e3, "gj_kernel_seconds_over_pairs": best[1] / 1e3 / info[1],
                   "gj_kernel_seconds_one_prime_alone": alone / 1e3,
                   "raw_call_seconds": best[2] / 1e3, "field_adjugate_mod_wall_seconds": best[3], "field_adjugate_bounds_seconds": t_bound,
                   "inverse_field_wall_seconds": t_whole, "inverse_field_device_call_seconds": spent["adjugate"], "inverse_field_crt_seconds": spent["crt"],
                   "inverse_field_check_seconds": spent["check"], "inverse_qq_regular_n": n * d, "inverse_qq_wall_seconds": None}
            if n * d <= args.qq_max_n:
                regular = regular_representation(M, f)
                t = time.perf_counter()
                over_qq = np.asarray(rounding.inverse_qq(regular, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul))
                row["inverse_qq_wall_seconds"] = time.perf_counter() - t
                for i in range(n):                                   # column 0 of the d x d block (i, j): the coordinates of the entry of the inverse
                    for j in range(n):
                        assert tuple(Fraction(over_qq[i * d + c, j * d]) for c in range(d)) == result.inverse[i, j], (n, name, i, j)
            rows.append(row)
            print(json.dumps(row), flush=True)
            write(args, rows)


def write(args, rows):
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"what": "rounding.inverse_field on random matrices over Z[g] with %d-bit coefficients, one MI355X; device times by device events, the best of %d "
                           "after a warm-up; the rest by wall clock; inverse_qq on the regular representation up to n d = %d" % (args.bits, args.repeats, args.qq_max_n),
                   "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

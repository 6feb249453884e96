"""Time of the exact integer matrix product on the device (clrs_amd.rounding.zz_matmul -> clrs_zz_gemm).  Per size n, separately:

  gram            one raw call of clrs_zz_gemm, A (n x 1.05 n, two-digit entries |a| < 2^46) times its transpose: the GEMM kernel, the combine and carry
                  kernels and the whole call from the first upload to the last download by device events (clrs_zz_gemm_times), the best of `--repeats`
                  after one warm-up call; the GEMM kernel's rate in fp64 flop/s (2 (nda m) k (ndb n) per call) beside the 78.6 TF matrix peak
  check           the same for the check product of solve_dixon: n x n, two digits, times a vector of K 23-bit integers, K = dixon_steps at p = 8388593
                  (the systems of scripts/dixon_time.py)
  zz_matmul       both products through `zz_matmul`, Python included (digit conversion both ways), and the share of the conversions
  host            the same products as the default path forms them (`A.dot(B)` on object arrays): in full where a first few rows predict less than a
                  minute, otherwise those rows multiplied up (`*_extrapolated`)
  pseudoinverse   `solve_system_pseudoinverse` as a whole on an n x 1.05 n system with `matmul=zz_matmul` (device lift and reconstruction in both runs);
                  the products of the default path -- Gram, `Ai x`, `A solution == b` in Fractions, the back-substitution in Fractions -- timed on the
                  operands of that very solve, a few rows each, and multiplied up; the default path as a whole where that predicts less than a minute

Entries of the products are verified against Python integers on the rows that the host formed.  Writes profiles/rounding/zz_gemm_times.json.  No time is a
pass criterion.

    python scripts/zz_gemm_time.py [--out profiles/rounding/zz_gemm_times.json] [--sizes 256 1024 2048] [--solve-sizes 128 256 512]
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
P = 8388593
BITS = 46
HOST_LIMIT = 60.0
PEAK_TF = 78.6
ROWS = 4


def best_of(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def raw_call(L, lib, Ad, Bd, ndc, repeats):
    """(record, C planes): clrs_zz_gemm on digit planes, the best whole-call time of `repeats` after one warm-up, with that call's kernel times"""
    (nda, m, k), (ndb, _, n) = Ad.shape, Bd.shape
    Cd, info = np.zeros((ndc, m, n), np.int32), np.zeros(4, np.int32)
    pi = lambda a: a.ctypes.data_as(lib.p_i32)
    best = None
    for it in range(repeats + 1):
        t = time.perf_counter()
        lib.check(L.clrs_zz_gemm(0, m, k, n, nda, pi(Ad), ndb, pi(Bd), ndc, pi(Cd), pi(info)))
        wall = time.perf_counter() - t
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        assert L.clrs_zz_gemm_times(C.byref(a), C.byref(b), C.byref(c)) == 0
        if it > 0 and (best is None or c.value < best[2]):
            best = (a.value, b.value, c.value, wall)
    assert info[0] == 0 and info[3] == 0
    flops = 2.0 * nda * m * k * ndb * n
    rec = dict(m=m, k=k, n=n, nda=nda, ndb=ndb, ndc=ndc, ranges=int(info[1]), workgroups=int(info[2]), gemm_ms=best[0], combine_carry_ms=best[1], whole_ms=best[2],
               call_wall_seconds=best[3], gemm_tflops=flops / (best[0] * 1e-3) / 1e12, gemm_fraction_of_matrix_peak=flops / (best[0] * 1e-3) / 1e12 / PEAK_TF,
               operand_bytes_fp64=8 * (nda * m * k + ndb * k * n), lo_hi_bytes=16 * nda * m * ndb * n)
    return rec, Cd


def host_rows(A, B, rows_total):
    """(seconds for all rows, extrapolated?, the rows formed as {row: values}): `A[r].dot(B)` on object arrays, in full when the first rows predict < a minute"""
    t = time.perf_counter()
    first = {r: A[r].dot(B) for r in range(min(ROWS, rows_total))}
    dt = time.perf_counter() - t
    est = dt / len(first) * rows_total
    if est >= HOST_LIMIT or len(first) == rows_total:
        return est, len(first) < rows_total, first
    t = time.perf_counter()
    full = A.dot(B)
    return time.perf_counter() - t, False, {r: full[r] for r in range(rows_total)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 2048])
    ap.add_argument("--solve-sizes", type=int, nargs="*", default=[128, 256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "zz_gemm_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    L = _lib.load()
    out = {}

    def save(key, rec):
        out[key] = rec
        print(json.dumps({key: rec}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)

    for n in args.sizes:
        rng = np.random.default_rng(n)
        cols = int(round(1.05 * n))
        A = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=(n, cols), dtype=np.int64)
        Ao = A.astype(object)
        # ---- the Gram product
        Ad, Bd = rounding.to_balanced_digits(A), rounding.to_balanced_digits(np.ascontiguousarray(A.T))
        ndc = ((cols << (2 * BITS)).bit_length() + 25) // 24
        rec, Cd = raw_call(L, _lib, Ad, Bd, ndc, args.repeats)
        t_host, extrapolated, rows = host_rows(Ao, np.ascontiguousarray(Ao.T), n)
        G = rounding.planes_to_ints(Cd)
        rec.update(verified_rows=len(rows), verified=bool(all((G[r] == v).all() for r, v in rows.items())), host_seconds=t_host, host_extrapolated=extrapolated)
        t_mm, Gm = best_of(lambda: rounding.zz_matmul(A, np.ascontiguousarray(A.T)), args.repeats)
        t_conv = best_of(lambda: (rounding.ints_to_planes(A), rounding.ints_to_planes(np.ascontiguousarray(A.T)), rounding.planes_to_ints(Cd)), 1)[0]
        rec.update(zz_matmul_seconds=t_mm, zz_matmul_conversion_seconds=t_conv, zz_matmul_equal=bool((Gm == G).all()))
        save(f"gram_n{n}", rec)
        # ---- the check product: the square system of scripts/dixon_time.py and a vector of K 23-bit integers
        S = A[:, :n]
        b = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=n, dtype=np.int64)
        K = rounding.dixon_steps(S.astype(object), b.astype(object), P)[0]
        nbytes = (23 * K + 7) // 8
        x = np.array([int.from_bytes(rng.bytes(nbytes), "little") >> (8 * nbytes - 23 * K) for _ in range(n)], dtype=object)
        t = time.perf_counter()
        xd = rounding.ints_to_planes(x.reshape(n, 1))
        t_xd = time.perf_counter() - t
        Sd = rounding.to_balanced_digits(S)
        ndc = ((n << (BITS + 23 * K)).bit_length() + 25) // 24
        rec, Cd = raw_call(L, _lib, Sd, xd, ndc, args.repeats)
        t_host, extrapolated, rows = host_rows(S.astype(object), x, n)
        t = time.perf_counter()
        y = rounding.planes_to_ints(Cd).reshape(n)
        t_back = time.perf_counter() - t
        rec.update(steps=K, vector_bits=23 * K, verified_rows=len(rows), verified=bool(all(y[r] == v for r, v in rows.items())), host_seconds=t_host,
                   host_extrapolated=extrapolated, vector_to_planes_seconds=t_xd, result_to_ints_seconds=t_back)
        t_mm, ym = best_of(lambda: rounding.zz_matmul(S, x), args.repeats)
        rec.update(zz_matmul_seconds=t_mm, zz_matmul_equal=bool((ym == y).all()))
        save(f"check_n{n}", rec)

    for n in args.solve_sizes:
        rng = np.random.default_rng(7 * n)
        cols = int(round(1.05 * n))
        A = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=(n, cols), dtype=np.int64).astype(object)
        b = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=n, dtype=np.int64).astype(object)
        calls = []

        def recording(M, N, device=0):
            t = time.perf_counter()
            res = rounding.zz_matmul(M, N, device=device)
            calls.append((np.asarray(M, dtype=object), np.asarray(N, dtype=object), time.perf_counter() - t))
            return res
        found = []

        def reconstructing(X, p, N, D, device=0, want_x=False):
            res = rounding.dixon_reconstruct(X, p, N, D, device=device, want_x=want_x)
            found.append(res[0] if want_x else res)
            return res
        rounding.zz_matmul(A[:8], A[:8].T)                                       # warm-up
        t = time.perf_counter()
        v = rounding.solve_system_pseudoinverse(A, b, reconstruct=reconstructing, matmul=recording)
        t_dev = time.perf_counter() - t
        assert len(calls) == 4 and len(found) == 1                              # Gram, Ai x, Ai y == L bi, A^T (Dr y)
        rec = dict(nrows=n, ncols=cols, device_path_seconds=t_dev, device_products_seconds=[c[2] for c in calls])
        # the products of the default path on the operands of this solve, a few rows each
        Gs, xl, sol = calls[1][0], calls[1][1], found[0]
        t_gram = host_rows(A, np.ascontiguousarray(A.T), n)[0]
        t_ax = host_rows(Gs, xl, n)[0]
        t = time.perf_counter()
        for i in range(ROWS):                                                   # `A solution == b` as solve_dixon forms it
            sum(Fraction(int(Gs[i, j])) * sol[j] for j in range(n))
        t_check = (time.perf_counter() - t) / ROWS * n
        t = time.perf_counter()
        for c in range(ROWS):                                                   # `A^T (Dr y)`; y = the solution itself here (Dr divides by small gcds only)
            sum((int(A[r, c]) * sol[r] for r in range(n)), Fraction(0))
        t_back = (time.perf_counter() - t) / ROWS * cols
        rec.update(host_gram_seconds=t_gram, host_lifted_check_seconds=t_ax, host_fraction_check_seconds_extrapolated=t_check,
                   host_back_substitution_seconds_extrapolated=t_back, host_products_seconds=t_gram + t_ax + t_check + t_back, rows_timed=ROWS)
        estimate = t_dev - sum(c[2] for c in calls) + rec["host_products_seconds"]
        rec["default_path_estimate_seconds"] = estimate
        if estimate < HOST_LIMIT:
            t = time.perf_counter()
            vh = rounding.solve_system_pseudoinverse(A, b, reconstruct=rounding.dixon_reconstruct)
            rec["default_path_seconds"] = time.perf_counter() - t
            rec["paths_equal"] = bool(vh == v)
        else:
            rec["default_path_seconds"] = None
        save(f"pseudoinverse_n{n}", rec)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Wall time of the rational reconstruction of Dixon solutions on the device (clrs_amd.rounding.dixon_reconstruct -> clrs_modp_dixon_reconstruct,
DESIGN.md section 16) beside the host path of `solve_dixon`: the systems of scripts/dixon_time.py (n = 256, 1024, 2048, two-digit entries, p = 8388593,
K steps from the bound), lifted on the device.  Per system:

  device          `dixon_reconstruct(X, p, N, D)` as a whole, conversion to `Fraction`s included: the best of three after one warm-up call; of that the
                  raw call (`raw_call_seconds`), inside it the two kernels by device events (`horner_kernel_seconds`, `euclid_kernel_seconds`, from
                  clrs_modp_dixon_reconstruct_times), and what is left for Python (`python_conversion_seconds` and its share)
  host            what `solve_dixon` does today per entry, Horner over the K digits and `rational_reconstruction`, in Python integers: every entry at
                  n = 256, three entries multiplied up above that (`host_entries_timed` says how many)
  counters        `info` of the call: the limbs of p^K, the most quotient steps of an entry, their total

At n = 256 the two results must be equal (asserted); above that the three host entries must equal the device's.  Writes
profiles/rounding/reconstruct_times.json.  No time is a pass criterion.

    python scripts/reconstruct_time.py [--out profiles/rounding/reconstruct_times.json] [--sizes 256 1024 2048]
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
BITS = 46


def best_of(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounding", "reconstruct_times.json"))
    args = ap.parse_args()
    import clrs_amd  # noqa: F401
    from clrs_amd import _lib, rounding
    L = _lib.load()
    out = {}
    for n in args.sizes:
        rng = np.random.default_rng(n)
        while True:                                             # the systems of scripts/dixon_time.py: redrawn until invertible mod p
            A = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=(n, n), dtype=np.int64)
            b = rng.integers(-(1 << BITS) + 1, 1 << BITS, size=n, dtype=np.int64)
            Ad, bl = rounding.to_balanced_digits(A), rounding.to_balanced_digits(b)
            if int(rounding._dixon_lift_digits(Ad, bl, P, 0)[2][0]) == n:
                break
        K, N, D = rounding.dixon_steps(A.astype(object), b.astype(object), P)
        X, _, info = rounding._dixon_lift_digits(Ad, bl, P, K)
        assert info.tolist() == [n, K, 0, 0]
        rounding.dixon_reconstruct(X[:, :4], P, N, D)            # warm-up: the code objects
        rounding.dixon_reconstruct(X, P, N, D)
        t_dev, sol = best_of(lambda: rounding.dixon_reconstruct(X, P, N, D), args.repeats)
        rinfo = list(rounding.dixon_reconstruct.last_info)
        h, e = C.c_double(0.0), C.c_double(0.0)
        assert L.clrs_modp_dixon_reconstruct_times(C.byref(h), C.byref(e)) == 0
        # the raw call alone, on the arrays dixon_reconstruct builds
        Nd, Dd = rounding.to_digits24(N), rounding.to_digits24(D)
        nl = max(Nd.size, Dd.size)
        num, den = np.zeros((n, nl), np.int32), np.zeros((n, nl), np.int32)
        neg, status, ri = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(4, np.int32)
        ptr = lambda a: a.ctypes.data_as(_lib.p_i32)
        raw = lambda: _lib.check(L.clrs_modp_dixon_reconstruct(0, n, P, K, ptr(X), Nd.size, ptr(Nd), Dd.size, ptr(Dd), nl, ptr(num), ptr(den), ptr(neg), ptr(status), 0,
                                                               None, ptr(ri)))
        t_raw, _ = best_of(raw, args.repeats)
        rec = dict(n=n, p=P, steps=K, limbs_of_m=rinfo[0], most_quotient_steps=rinfo[1], total_quotient_steps=rinfo[2], impossibilities=rinfo[3],
                   device_seconds=t_dev, raw_call_seconds=t_raw, horner_kernel_seconds=h.value / 1e3, euclid_kernel_seconds=e.value / 1e3,
                   python_conversion_seconds=max(t_dev - t_raw, 0.0), python_conversion_share=max(t_dev - t_raw, 0.0) / t_dev,
                   reconstructed=bool(all(v is not None for v in sol)))
        # the host path that exists today
        entries = list(range(n)) if n <= 256 else [0, n // 2, n - 1]
        m = P ** K
        t = time.perf_counter()
        host = {}
        for i in entries:
            v = 0
            for k in range(K - 1, -1, -1):
                v = v * P + int(X[k, i])
            host[i] = rounding.rational_reconstruction(v, m, N, D)
        dt = time.perf_counter() - t
        assert all(host[i] == sol[i] for i in entries), "the device and the host reconstruction differ"
        rec.update(host_entries_timed=len(entries), host_seconds_per_entry=dt / len(entries), host_seconds_all_entries=dt / len(entries) * n,
                   host_extrapolated=len(entries) < n, results_equal_on_the_timed_entries=True, host_over_device=dt / len(entries) * n / t_dev)
        out[f"n{n}"] = rec
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

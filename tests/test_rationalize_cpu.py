"""CPU side of the rounding of kernel vectors to rationals (clrs_mw_rational.hip.h, clrs_amd.rounding): mw_cf_round compiled for the host at every limb
count against its restatement with Fractions on the exact value of the limbs, the Python layer with a host stand-in for the device call (the package has no
CPU implementation of it), the binding of both symbols, and the 320-bit oracle's solution of delsarte_exact(8, 3, 1/2)."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib
from clrs_amd.rounding import BlockKernel, KernelVectorError, RoundingSettings, kernel_vectors, rationalize, vectors_to_fractions
from tests import kernel_vectors_util as ku
from tests import rationalize_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3)


class _Sol:
    def __init__(self, X, Y):
        self.X, self.Y = X, Y


def check_against_restatement(K, values, errbound):
    """host build == restatement for every number of the planar pool; asserts that no examined |q x - p| is within a relative 2^-40 of the bound (where
    the head the device compares and the exact value the restatement compares could fall on different sides).  Returns the restatement's triples."""
    num, den, status, vq = ru.host_rationalize(values, K, errbound)
    eps, out = Fraction(errbound), []
    for i in range(values.shape[1]):
        rn, rd, rs, seen = ru.cf_reference(ru.exact_value(values[:, i]), errbound)
        assert all(abs(e - eps) > eps / 2 ** 40 for e in seen), (K, i, float(values[0, i]), "a convergent within 2^-40 of the bound: choose another seed")
        assert (num[i], den[i], int(status[i])) == (rn, rd, rs), (K, i, float(values[0, i]), (num[i], den[i], int(status[i])), (rn, rd, rs))
        assert float(int(num[i])) == num[i] and float(int(den[i])) == den[i]
        if rs == 0:
            assert rd >= 1 and abs(rn) < ru.CAP and rd < ru.CAP
            # num / den in K limbs: the limbs sum to the quotient within the arithmetic's 2^-(52 K - K) of it
            assert abs(ru.exact_value(vq[:, i]) - Fraction(rn, rd)) <= abs(Fraction(rn, rd)) / 2 ** (51 * K)
        else:
            assert np.all(vq[:, i] == 0)
        out.append((rn, rd, rs))
    return out


@pytest.mark.parametrize("K", ru.LIMBS)
def test_host_build_against_the_fraction_restatement(K):
    for seed in SEEDS:
        for name, values in ru.input_classes(K, seed):
            got = check_against_restatement(K, values, ru.EPS)
            st = [g[2] for g in got]
            if name in ("ratio plus noise", "negative", "integer", "irrational", "zero", "pure noise"):
                assert st == [0] * len(st), (K, name, st)
            if name in ("zero", "pure noise"):
                assert all(g[:2] == (0, 1) for g in got), (K, name, got)
            if name == "ratio plus noise":
                assert all(0 < g[1] <= 10 ** 6 and g[0] >= 0 for g in got) and got[-1][:2] == (7, 2)
            if name == "negative":
                assert all(g[0] < 0 for g in got) and got[-2][:2] == (-3, 1) and got[-1][:2] == (-1, 3)
            if name == "integer":
                assert all(g[1] == 1 and 1 <= g[0] < 2 ** 53 for g in got) and got[-3][0] == 2 ** 52
            if name == "beyond the cap":
                assert st == [1] * len(st) and all(g[:2] == (0, 0) for g in got)
            if name == "irrational":
                assert all(g[1] > 10 ** 14 for g in got), (K, got)                 # |q sqrt(2) - p| ~ 1 / (2.8 q) < 1e-15
                assert got[0][0] == -got[2][0] and got[0][1] == got[2][1]         # round(-v) = -round(v)
            if name == "not finite":
                assert st == [2, 2, 2] and all(g[:2] == (0, 0) for g in got)


def test_irrationals_beyond_the_cap_at_ten_limbs():
    """sqrt(2) and the golden ratio at errbound = 1e-40: a convergent that good has q ~ 1e39, the cap of 2^53 comes first"""
    values = dict(ru.input_classes(10, 1))["irrational"]
    assert check_against_restatement(10, values, 1e-40) == [(0, 0, 1)] * 3


def test_sign_symmetry_and_the_same_answer_at_every_limb_count():
    ref = None
    for K in ru.LIMBS:
        v = dict(ru.input_classes(K, 2))["ratio plus noise"]
        a, b = ru.host_rationalize(v, K), ru.host_rationalize(-v, K)
        assert np.array_equal(a[0], -b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], -b[3])
        ref = a[:3] if ref is None else ref
        assert all(np.array_equal(x, y) for x, y in zip(ref, a[:3])), K


# ---- the Python layer with a host stand-in ---------------------------------------------------------------------------------------------------

def test_rationalize_false_returns_what_it_returned():
    X, Y = np.diag([1.0, 0.0]).reshape(-1), np.diag([0.0, 1.0]).reshape(-1)
    calls = []

    def never(*a, **kw):
        calls.append(a)
        raise AssertionError("the rounding call must not be made")
    out = kernel_vectors([2], _Sol(X, Y), limbs=5, batch=ku.host_batch, round_batch=never)
    again = kernel_vectors([2], _Sol(X, Y), limbs=5, batch=ku.host_batch)
    assert not calls and [k.count for k in out] == [1]
    for k, k2 in zip(out, again):
        assert k.num is None and k.den is None and k.round_status is None and k.vectors_rounded is None and k.round_resid_max is None
        assert np.array_equal(k.vectors, k2.vectors) and np.array_equal(k.resid_max, k2.resid_max) and list(k.perm) == list(k2.perm)
    # the new fields are appended with defaults: the positional construction of before still works
    k = BlockKernel("dual", 1, 1, np.zeros(2, np.int32), np.zeros((5, 2, 1)), np.zeros(1), np.zeros(1), np.zeros((5, 1)))
    assert k.num is None and k.max_num == 0 and k.max_den == 0
    with pytest.raises(ValueError, match="not rounded"):
        vectors_to_fractions(k)


def test_rounded_fields_fractions_and_maxima():
    # X = u u^T with u = (3, 2), Y = w w^T with w = (2, -3): the kernel vector of Y is (1, 2/3), over the pivot 0 of X and over the non-pivot 0 of Y alike
    u, w = np.array([3.0, 2.0]), np.array([2.0, -3.0])
    sol = _Sol(np.outer(u, u).reshape(-1), np.outer(w, w).reshape(-1))
    for settings, want in ((RoundingSettings(), [Fraction(1), Fraction(2, 3)]), (RoundingSettings(kernel_use_dual=False), [Fraction(1), Fraction(2, 3)])):
        (k,) = kernel_vectors([2], sol, limbs=4, settings=settings, rationalize=True, round_batch=ru.host_round_batch, batch=ku.host_batch,
                              check_dimensions=True)
        assert vectors_to_fractions(k) == [want]
        assert k.num.shape == k.den.shape == k.round_status.shape == (2, 1) and k.vectors_rounded.shape == (4, 2, 1)
        assert (k.max_num, k.max_den) == (max(f.numerator for f in want), max(f.denominator for f in want))
        assert np.all(k.round_status == 0) and k.round_resid_max.shape == (1,) and k.round_resid_max[0] <= 1e-10
    assert clrs_amd.rationalize is rationalize and clrs_amd.vectors_to_fractions is vectors_to_fractions


def _rank_one_pair(t_of_mp, scale, K):
    """X = u u^T, Y = scale * w w^T with u = (1, t), w = (t, -1) in K limbs (X Y = 0 to the last limb): the kernel of Y is spanned by u"""
    import mpmath as mp
    from clrs_amd.mw import to_limbs
    with mp.workprec(64 * K + 128):
        t = t_of_mp()
        u, w = [mp.mpf(1), t], [t, mp.mpf(-1)]
        X = to_limbs([u[i] * u[j] for j in range(2) for i in range(2)], K)
        Y = to_limbs([scale * w[i] * w[j] for j in range(2) for i in range(2)], K)
    return _Sol(X, Y)


def test_irrational_kernel_under_a_scaled_primal_block_is_a_wrong_vector():
    """The kernel of Y is spanned by (1, t), t = 1 + sqrt(2) 2^-51: irrational, and within kernel_round_errbound = 1e-15 of 1, so the vector rounds to (1, 1),
    which misses the kernel by 6e-16.  Under Y scaled by 1e8 that is a residual of 6e-8 > kernel_errbound: the vector before rounding passes the first check
    (it is in the kernel to the last limb), the rounded one fails the second."""
    import mpmath as mp
    sol = _rank_one_pair(lambda: 1 + mp.sqrt(2) * mp.mpf(2) ** -51, mp.mpf(10) ** 8, 5)
    out = kernel_vectors([2], sol, limbs=5, batch=ku.host_batch)
    assert out[0].count == 1 and out[0].resid_max[0] < 1e-40
    seen = []

    def spy(*a, **kw):
        seen.extend(ru.host_round_batch(*a, **kw))
        return seen
    with pytest.raises(KernelVectorError, match="wrong vector detected: block 0, rounded vector 0"):
        kernel_vectors([2], sol, limbs=5, rationalize=True, round_batch=spy)
    assert vectors_to_fractions(seen[0]) == [[Fraction(1), Fraction(1)]] and 1e-8 < seen[0].round_resid_max[0] < 1e-7


def test_entry_without_a_relation_raises_the_clindep_message():
    """the kernel vector (1 / sqrt(2), 1) at kernel_round_errbound = 1e-40: a convergent that good has q ~ 1e39, the cap comes first (status 1)"""
    import mpmath as mp
    sol = _rank_one_pair(lambda: mp.sqrt(2), mp.mpf(1), 5)
    tight = RoundingSettings(kernel_round_errbound=1e-40)
    with pytest.raises(KernelVectorError, match=r"clindep failed to find a relation: block 0, vector 0, entry 0 \(status 1\)"):
        kernel_vectors([2], sol, limbs=5, settings=tight, rationalize=True, round_batch=ru.host_round_batch)
    # at the default bound the same vector rounds (q ~ 1e15) and stays in the kernel to 1e-30
    (k,) = kernel_vectors([2], sol, limbs=5, rationalize=True, round_batch=ru.host_round_batch)
    assert k.round_status.tolist() == [[0], [0]] and k.den[1, 0] == 1 and k.den[0, 0] > 1e14 and k.round_resid_max[0] < 1e-25


def test_lib_binds_both_symbols_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "double": C.c_double, "const double *": _lib.p_d, "double *": _lib.p_d, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    names = {"clrs_mw_rationalize": ["device", "limbs", "count", "v", "plane", "errbound", "num", "den", "status", "vq"],
             "clrs_mw_kernel_vectors_rational": ["device", "limbs", "nblk", "n", "X", "Y", "plane", "tau", "use_dual", "dual_max", "round_errbound", "branch", "perm",
                                                 "rank", "count", "V", "resid_max", "v_max", "pivot_resid", "num", "den", "status", "Vq", "round_resid_max"]}
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    for sym, want_names in names.items():
        ret, args = re.search(r"^\s*(\w+)\s+" + sym + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")] == want_names
        want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]        # KeyError: a type the Julia table lacks
        assert ret == "int" and _lib.SYMBOLS[sym] == (C.c_int, want)
        assert ":" + sym in jl
    # the shared part of the two kernel-vector prototypes is the same list
    assert [n for n in names["clrs_mw_kernel_vectors_rational"] if n not in ("round_errbound", "num", "den", "status", "Vq", "round_resid_max")] == \
        ["device", "limbs", "nblk", "n", "X", "Y", "plane", "tau", "use_dual", "dual_max", "branch", "perm", "rank", "count", "V", "resid_max", "v_max", "pivot_resid"]
    assert "function rationalize(" in jl and "rationalize::Bool" in jl


# ---- the 320-bit oracle's solution of delsarte_exact(8, 3, 1/2) ------------------------------------------------------------------------------

def test_oracle_solution_of_delsarte_exact_rounds_to_zero_and_plus_minus_one(oracle_built):
    from oracle.oracle import Oracle
    from clrs_amd import problems as P
    f = clrs_amd.flatten(P.delsarte_exact(8, 3, 0.5))
    assert [int(n) for n in f.block_n] == [1] * 7 + [4, 3] and f.n_free == 0
    r = Oracle(f, mp_bits=320).solvesdp(duality_gap_threshold=1e-40)
    print("delsarte_exact(8, 3, 1/2), 320-bit oracle:", r["iterations"], "iterations, objectives", r["p_obj"], r["d_obj"], "gap", r["gap"])
    assert r["error_code"] == 0 and abs(r["p_obj"] - 240) <= 1e-12 and abs(r["d_obj"] - 240) <= 1e-12
    sol = _Sol(r["X"], r["Y"])
    for settings in (RoundingSettings(), RoundingSettings(kernel_use_dual=False)):
        blocks = kernel_vectors(f, sol, limbs=5, settings=settings, check_dimensions=True, rationalize=True, round_batch=ru.host_round_batch,
                                batch=ku.host_batch)
        assert all(k.branch == ("dual" if settings.kernel_use_dual else "primal") for k in blocks)
        ru.check_delsarte_exact_kernel(blocks)

"""CPU side of the exact positive-definiteness check (rounding.checkpd, is_valid_solution, clrs_modp_minors): the host layer through
the `minors=` stand-in (tests/pd_util.py: the per-prime elimination restated on Python integers) against Bareiss' exact minors with `==`, the binding and
the refusals of the C function, which happen before any device call."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import pd_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pi = pu._pi


# ---- the oracles agree with each other ---------------------------------------------------------------------------------------------------------------------------
def test_oracles_agree():
    for seed, n in ((1, 1), (2, 2), (3, 7), (4, 18)):
        M = pu.random_symmetric(seed, n, 40)
        exact = pu.bareiss_minors(M)
        assert exact == [pu.det([row[:k] for row in M[:k]]) for k in range(1, n + 1)]
        for p in (2, 3, 10007, pu.PMAX):
            assert pu.minors_mod(M, p) == pu.minors_from_exact(exact, p) == pu.minors_mod_np(M, p)
    M, _, k = pu.planted("zero minor 17 of 33")
    exact = pu.bareiss_minors(M)
    assert len(exact) == 33 and exact[16] == 0 and all(v > 0 for v in exact[:16]) and pu.minors_mod(M, 10007)[1] == 17


# ---- minor_bounds and crt_tree ------------------------------------------------------------------------------------------------------------------------------------
def test_minor_bounds_hold_and_are_hadamard():
    for seed, n, bits in ((1, 1, 5), (2, 6, 3), (3, 17, 60), (4, 9, 300)):
        M = pu.random_symmetric(seed, n, bits)
        H, exact = rounding.minor_bounds(M), pu.bareiss_minors(M)
        assert len(H) == n and all(isinstance(h, int) and h >= abs(v) for h, v in zip(H, exact))
        for k in (1, n):                                             # the definition: the product of the rounded-up row norms of the leading part
            want = 1
            for i in range(k):
                s = sum(M[i][j] ** 2 for j in range(k))
                r = rounding._isqrt(s)
                want *= r if r * r == s else r + 1
            assert H[k - 1] == want
    assert rounding.minor_bounds([[3, 4], [4, 0]]) == [3, 20]        # exact square roots are not rounded further
    assert rounding.minor_bounds([[0, 0], [0, 5]]) == [0, 0]
    with pytest.raises(ValueError):
        rounding.minor_bounds([[1, 2], [3, 4]])
    with pytest.raises(ValueError):
        rounding.minor_bounds([[1, 2, 3], [2, 4, 5]])


def test_crt_tree_against_int_arithmetic():
    rng = np.random.default_rng(8)
    sched = [int(p) for p in rounding._primes_descending()[:70]]
    chain = [rounding.prev_prime(1 << 23)]
    for _ in range(3):
        chain.append(rounding.prev_prime(chain[-1]))
    assert sched[:4] == chain and chain[0] == pu.PMAX                # the schedule is what repeated prev_prime gives
    for primes in ([pu.PMAX], [2], [2, 3], [7, 2, 5], sched[:5], sched[:64], sched[:65] + [2, 10007], sched):
        P = 1
        for p in primes:
            P *= p
        half = P // 2
        vals = [0, 1, -1, half, -((P - 1) // 2), 12345 % (half + 1), -(10 ** 40) % (half + 1)] + [pu_big(rng, half) for _ in range(6)] + [-pu_big(rng, (P - 1) // 2) for _ in range(6)]
        vals = [v for v in vals if -P < 2 * v <= P]
        res = np.array([[v % p for v in vals] for p in primes], dtype=np.int64)
        got, modulus = rounding.crt_tree(res, primes)
        assert modulus == P and got == vals and all(isinstance(v, int) for v in got)
        one, _ = rounding.crt_tree(res[:, 2], primes)               # a single vector of residues
        assert one == vals[2]
    with pytest.raises(ValueError):
        rounding.crt_tree([[1], [1]], [7, 7])
    with pytest.raises(ValueError):
        rounding.crt_tree(np.zeros((0, 1)), [])


def pu_big(rng, bound):
    """a random integer in [0, bound]"""
    return int.from_bytes(rng.bytes(bound.bit_length() // 8 + 2), "little") % (bound + 1)


# ---- checkpd through the stand-in ---------------------------------------------------------------------------------------------------------------------------------
def scaled(A):
    """(scale, integer matrix) as checkpd forms them"""
    from math import gcd
    scale = 1
    for row in A:
        for v in row:
            scale = scale * F(v).denominator // gcd(scale, F(v).denominator)
    return scale, [[int(F(v) * scale) for v in row] for row in A]


def check_certificate(A, cert):
    """the certificate against Bareiss' exact minors of the scaled matrix"""
    scale, M = scaled(A)
    exact = pu.bareiss_minors(M)
    first_bad = next((k + 1 for k, v in enumerate(exact) if v <= 0), None)
    assert cert.scale == scale and cert.pd == (first_bad is None) and bool(cert) == cert.pd
    assert cert.failed_order == first_bad
    assert cert.minors == exact[:first_bad if first_bad else len(exact)]
    assert all(isinstance(v, int) for v in cert.minors)
    assert len(set(cert.primes)) == len(cert.primes) and cert.primes == [int(p) for p in rounding._primes_descending()[:len(cert.primes)]]
    for p, k in cert.discarded:                                      # a discarded prime divides the minor it broke down at, and none before it
        assert p in cert.primes and exact[k - 1] % p == 0 and all(v % p for v in exact[:k - 1])
    return exact


@pytest.mark.parametrize("name", pu.PLANTED)
def test_planted_matrices(name):
    A, pd, order = pu.planted(name)
    assert all(A[i][i] > 0 for i in range(len(A)))                   # nothing here is decided by the diagonal
    pu.host_minors.calls.clear()
    cert = rounding.checkpd(A, minors=pu.host_minors)
    exact = check_certificate(A, cert)
    assert cert.pd == pd and (order is None or cert.failed_order == order) and len(pu.host_minors.calls) >= 1
    if name == "singular psd":
        assert cert.failed_order == len(A) and cert.minors[-1] == 0 and all(v > 0 for v in cert.minors[:-1])
        assert len(cert.discarded) == len(cert.primes)               # every prime breaks down where the minor is zero, and the zero is proven all the same
    if name == "zero minor 17 of 33":
        assert cert.minors[-1] == 0 and len(cert.minors) == 17
    if name == "negative minor 9 of 20":
        assert cert.minors[-1] < 0 and len(cert.minors) == 9
    if name == "first prime planted at 5 of 12":
        assert exact[4] == pu.PMAX and cert.discarded == [(pu.PMAX, 5)] and cert.primes[0] == pu.PMAX and len(cert.minors) == 12


def test_hilbert_needs_an_exact_certificate():
    """fp64 Cholesky cannot factor the Hilbert matrix of order 20, let alone tell it from the same matrix minus a multiple of I that fp64 cannot see.  The
    smallest eigenvalue of that matrix is about 7.8e-29, so H - 10^-40 I is still positive definite and H - 10^-28 I is not: three matrices with one and the
    same fp64 image and two different answers, both decided exactly (and equal to Bareiss' minors, test_planted_matrices)"""
    H = pu.hilbert(20)
    image = lambda A: np.array([[float(v) for v in row] for row in A])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(image(H))
    near, far = pu.planted("hilbert20 minus 1e-40")[0], pu.planted("hilbert20 minus 1e-28")[0]
    assert np.array_equal(image(H), image(near)) and np.array_equal(image(H), image(far))
    a, b, c = (rounding.checkpd(A, minors=pu.host_minors) for A in (H, near, far))
    assert a.pd and a.failed_order is None and len(a.minors) == 20 and b.pd and len(b.minors) == 20
    assert not c.pd and c.failed_order is not None and c.minors[-1] < 0 and all(v > 0 for v in c.minors[:-1])


def test_breakdowns_that_leave_too_few_primes_draw_more():
    """every prime of the first call divides minor 2, so order 3 needs a further call"""
    M = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    first = [int(p) for p in rounding._primes_descending()[:1]]
    M[1][1] = first[0]
    pu.host_minors.calls.clear()
    cert = rounding.checkpd(M, minors=pu.host_minors)
    check_certificate(M, cert)
    assert cert.pd and cert.minors == [1, first[0], first[0]] and cert.discarded == [(first[0], 2)] and len(pu.host_minors.calls) == 2 and len(cert.primes) >= 2


def test_small_and_degenerate_inputs():
    assert rounding.checkpd([], minors=pu.host_minors) == rounding.PDCertificate(True, [], None, 1, [], [])
    assert rounding.checkpd(np.zeros((0, 0)), minors=pu.host_minors).pd
    pu.host_minors.calls.clear()
    c = rounding.checkpd([[F(1, 2), 0], [0, F(-1, 3)]], minors=pu.host_minors)          # a diagonal entry <= 0: the host answers
    assert not c.pd and c.failed_order == 2 and c.minors == [] and c.scale == 6 and pu.host_minors.calls == []
    assert not rounding.checkpd([[0]], minors=pu.host_minors).pd and pu.host_minors.calls == []
    c = rounding.checkpd([[F(3, 7)]], minors=pu.host_minors)
    assert c.pd and c.minors == [3] and c.scale == 7
    c = rounding.checkpd([[1, 2], [2, 1]], minors=pu.host_minors)
    assert not c.pd and c.failed_order == 2 and c.minors == [1, -3]
    for seed in range(6):                                            # random symmetric matrices with a positive diagonal, mostly indefinite
        M = pu.random_symmetric(seed, 6, 8)
        for i in range(6):
            M[i][i] = abs(M[i][i]) + 300
        check_certificate(M, rounding.checkpd(M, minors=pu.host_minors))
    M = pu.random_spd(7, 9, 200)
    assert check_certificate(M, rounding.checkpd(M, minors=pu.host_minors))[-1] > 0


def test_asymmetric_and_non_square_inputs_are_refused():
    for bad in ([[1, 2], [3, 4]], [[1, 2, 3], [2, 4, 5]], [1, 2, 3], [[F(1, 2), F(1, 3)], [F(1, 4), 1]]):
        with pytest.raises(ValueError):
            rounding.checkpd(bad, minors=pu.host_minors)
    with pytest.raises(ValueError, match="128"):
        rounding.checkpd(np.eye(129, dtype=np.int64), minors=pu.host_minors)


def test_is_valid_solution():
    good, bad = [[2, 1], [1, 2]], [[1, 2], [2, 1]]
    A, x = [[1, F(1, 2), 0], [0, 1, 1]], [F(1, 3), 2, -1]
    b = [F(4, 3), 1]
    assert rounding.is_valid_solution([good, pu.hilbert(5)], A, b, x, minors=pu.host_minors) == (True, [])
    ok, failures = rounding.is_valid_solution([good, bad, good, [[-1]]], A, [F(4, 3), 2], x, minors=pu.host_minors)
    assert not ok and failures == [("constraint", 1, F(-1)), ("block", 1, 2), ("block", 3, 1)]
    assert rounding.is_valid_solution([good], check_slacks=False, minors=pu.host_minors) == (True, [])
    assert rounding.is_valid_solution([], A, b, x, minors=pu.host_minors) == (True, [])
    with pytest.raises(ValueError):
        rounding.is_valid_solution([good], minors=pu.host_minors)
    with pytest.raises(ValueError):
        rounding.is_valid_solution([good], A, b, x[:2], minors=pu.host_minors)


# ---- the binding and the refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbol_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32, "double *": _lib.p_d}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_minors\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "n", "nd", "digits", "nprimes", "primes", "minors", "breakdown", "info"]
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_minors"] == (C.c_int, [table[re.sub(r"\w+$", "", a).strip()] for a in args])
    assert _lib.SYMBOLS["clrs_modp_minors_times"] == (C.c_int, [_lib.p_d] * 3)
    assert re.search(r"^#define CLRS_MODP_MINORS_MAX_N 128$", hdr, flags=re.M) and rounding.MINORS_MAX_N == 128
    L = _lib.load()
    assert hasattr(L, "clrs_modp_minors") and hasattr(L, "clrs_modp_minors_times")
    for name in ("leading_minors_mod", "minor_bounds", "crt_tree", "checkpd", "PDCertificate", "is_valid_solution"):
        assert name in rounding.__all__ and hasattr(rounding, name)


def test_refusals_need_no_device():
    """what clrs_modp_minors refuses, it refuses before it touches a device, and it writes nothing"""
    L = _lib.load()
    D = np.array([[[2, 1], [1, 3]], [[0, -1], [-1, 0]]], np.int32)  # nd = 2, n = 2
    P = np.array([pu.PMAX, 10007, 2], np.int32)
    minors, brk, info = np.full((3, 2), pu.SENTINEL, np.int32), np.full(3, pu.SENTINEL, np.int32), np.full(4, pu.SENTINEL, np.int32)

    def call(n=2, nd=2, D=D, nprimes=3, P=P, minors=minors, brk=brk, info=info):
        return L.clrs_modp_minors(0, n, nd, _pi(D), nprimes, _pi(P), _pi(minors), _pi(brk), _pi(info))
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=129) == -1 and b"128" in L.clrs_last_error()
    assert call(nd=0) == -1 and call(nd=32768) == -1 and call(nprimes=0) == -1 and call(nprimes=65536) == -1
    for name in ("D", "P", "minors", "brk", "info"):
        assert call(**{name: None}) == -1 and b"null" in L.clrs_last_error()
    for v in ((1 << 23) + 1, -(1 << 23) - 1):
        bad = D.copy()
        bad[1, 0, 0] = v
        assert call(D=bad) == -1 and b"digit" in L.clrs_last_error()
    bad = D.copy()
    bad[1, 0, 1] = 5
    assert call(D=bad) == -1 and b"symmetric" in L.clrs_last_error()
    for p in (1, 0, -7, 4, 10005, 1 << 23, (1 << 23) + 9):
        assert call(P=np.array([pu.PMAX, p, 2], np.int32)) == -1 and b"prime" in L.clrs_last_error()
    assert call(P=np.array([10007, 2, 10007], np.int32)) == -1 and b"repeated" in L.clrs_last_error()
    assert all(int(v) == pu.SENTINEL for a in (minors, brk, info) for v in a.flat)
    assert L.clrs_modp_minors_times(None, None, None) == -1
    assert L.clrs_config_set(b"modp_minors_chunk_bytes", 4096) == 0 and L.clrs_config_set(b"modp_minors_chunk_bytes", 0) == 0
    with pytest.raises(ValueError):
        rounding.leading_minors_mod([[1, 2], [3, 4]], [7])
    with pytest.raises(ValueError):
        rounding.leading_minors_mod(np.eye(129, dtype=np.int64), [7])
    with pytest.raises(ValueError):
        rounding.leading_minors_mod([[1]], [])
    with pytest.raises(ValueError):
        rounding.leading_minors_mod([[1]], [1 << 23])


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    if torch.cuda.is_available():
        m, b = rounding.leading_minors_mod([[2, 1], [1, 2]], [7])
        assert m.tolist() == [[2, 3]] and b.tolist() == [0]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.leading_minors_mod([[2, 1], [1, 2]], [7])
        with pytest.raises(_lib.ClrsError):
            rounding.checkpd([[2, 1], [1, 2]])

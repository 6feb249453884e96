"""CPU side of the rational reconstruction on the device (clrs_modp_dixon_reconstruct, rounding.dixon_reconstruct): the limb arithmetic
of csrc/clrs_modp_rec_arith.h compiled for the host against Python integers, a whole Euclid built from its pieces against rounding.rational_reconstruction on
the cases of the GPU tests, the linear digit conversion, `reconstruct=` in the Python layer with a stand-in (no device), the binding and the refusals."""
import ctypes as C
import os
import re
from fractions import Fraction as F
from math import gcd

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_util as du
from tests import modp_util as mu
from tests import reconstruct_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pi = ru._pi


# ---- the host build of clrs_modp_rec_arith.h -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (2, 3, 10007, ru.PMAX))
def test_host_horner_steps(p):
    """v <- v p + d fully carried, limb for limb against Python integers, with the carry out of a row that is too short; then K lazy steps and one
    normalisation: the same integer, and no limb ever reaches 2^25"""
    L, rng = ru.host_lib(), np.random.default_rng(p)
    for n in (1, 2, 5):
        for _ in range(50):
            v = ru.big_random(rng, 1 << (24 * n))
            d = int(rng.integers(0, p))
            limbs, carry = ru.digits(v, n), C.c_longlong(0)
            assert L.rec_horner_host(n, p, d, _pi(limbs), C.byref(carry)) == 0
            assert ru.value(limbs) + (carry.value << (24 * n)) == v * p + d and 0 <= int(limbs.min()) and int(limbs.max()) < ru.BASE
    for K in (1, 2, 24, 25, 67):
        X = rng.integers(0, p, size=K).astype(np.int32)
        X[K // 2] = p - 1
        n = ru.length(p ** K)
        v, big, carry = np.zeros(n, np.int32), np.zeros(1, np.int32), C.c_longlong(0)
        assert L.rec_horner_lazy_host(n, p, K, _pi(X), _pi(v), _pi(big), C.byref(carry)) == 0
        assert carry.value == 0 and ru.value(v) == ru.horner(X.reshape(K, 1), p)[0] and int(big[0]) < 1 << 25 and int(v.max()) < ru.BASE


def test_host_horner_lazy_at_the_largest_digits():
    """every digit p - 1 at the largest prime: x = p^K - 1, the limbs as large as the lazy steps make them"""
    L, p, K = ru.host_lib(), ru.PMAX, 134
    X = np.full(K, p - 1, np.int32)
    n = ru.length(p ** K)
    v, big, carry = np.zeros(n, np.int32), np.zeros(1, np.int32), C.c_longlong(0)
    assert n == 129 and L.rec_horner_lazy_host(n, p, K, _pi(X), _pi(v), _pi(big), C.byref(carry)) == 0
    assert carry.value == 0 and ru.value(v) == p ** K - 1 and int(big[0]) < 1 << 25


def test_host_length_and_comparison():
    L = ru.host_lib()
    for v, n in ((0, 0), (1, 1), (ru.BASE - 1, 1), (ru.BASE, 2), (ru.BASE ** 3, 4), (ru.BASE ** 3 - 1, 3)):
        assert L.rec_length_host(_pi(ru.digits(v, 6)), 6) == n == ru.length(v)
    rng = np.random.default_rng(5)
    vals = [0, 1, ru.BASE - 1, ru.BASE, ru.BASE + 1, ru.BASE ** 2 - 1, ru.BASE ** 2, 5 * ru.BASE ** 2 + 7, 5 * ru.BASE ** 2 + 8] + [ru.big_random(rng, 1 << 70) for _ in range(20)]
    for a in vals:
        for b in vals:
            assert L.rec_compare_host(_pi(ru.digits(a)), ru.length(a), _pi(ru.digits(b)), ru.length(b)) == (a > b) - (a < b)


def test_host_top_bits():
    L, rng = ru.host_lib(), np.random.default_rng(6)
    vals = [1, 2, ru.BASE - 1, ru.BASE, (1 << 62) - 1, 1 << 62, (1 << 63) + 12345, (1 << 96) - 1, 1 << 120] + [ru.big_random(rng, 1 << int(b)) + 1 for b in rng.integers(1, 200, 200)]
    for v in vals:
        for nbits in (31, 62):
            out, e = C.c_longlong(0), C.c_int(0)
            assert L.rec_top_bits_host(_pi(ru.digits(v)), ru.length(v), nbits, C.byref(out), C.byref(e)) == 0
            assert e.value == max(v.bit_length() - nbits, 0) and out.value == v >> e.value


def _adversarial_pairs():
    """(r0, r1): equal in their top limbs, equal altogether, one apart, powers of the base and their neighbours, a short r1 under a long r0"""
    B = ru.BASE
    top = [1, 2, B - 1, 1 << 23, (1 << 23) - 1]
    out = []
    for n in (1, 2, 3, 4, 7):
        for t in top:
            a = t * B ** (n - 1)
            for lo in (0, 1, B ** (n - 1) - 1) if n > 1 else (0,):
                out += [(a + lo, a + lo), (a + lo + 1, a + lo), (a + lo, a + lo + 1), (a + lo, a), (a + (B ** (n - 1) - 1 if n > 1 else 0), a)]
    for n0 in (1, 2, 3, 5, 9):
        for n1 in range(1, n0 + 1):
            for r0 in (B ** n0 - 1, B ** (n0 - 1), B ** (n0 - 1) + 1, (1 << 23) * B ** (n0 - 1)):
                for r1 in (B ** n1 - 1, B ** (n1 - 1), B ** (n1 - 1) + 1, 3 * B ** (n1 - 1) - 1):
                    out.append((r0, r1))
    out += [(3 * B ** 8 + 5, 3), (B ** 64 + 1, 1), (B ** 64 - 1, 2 ** 30 + 12345), (2 ** 62 - 1, 2 ** 31), (2 ** 62, 2 ** 31 - 1), (2 ** 62 + 1, 2 ** 62 + 1)]
    return [(a, b) for a, b in out if b > 0]


def _check_estimate(r0, r1):
    c, s = ru.host_estimate(r0, r1)
    assert 0 <= c < ru.BASE and s >= 0
    assert c * ru.BASE ** s * r1 <= r0                              # never above the true quotient
    assert (c >= 1) == (r0 >= r1)                                    # at least 1 whenever r0 >= r1, and 0 below
    cw, sw = ru.host_estimate(r0, r1, window=True)
    assert cw * ru.BASE ** sw * r1 <= r0 and (cw == 0 or (cw, sw) == (c, s))
    return c, s


def test_host_quotient_estimate_guarantees():
    rng = np.random.default_rng(7)
    for r0, r1 in _adversarial_pairs():
        _check_estimate(r0, r1)
    for _ in range(3000):
        b0, b1 = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        r0, r1 = ru.big_random(rng, 1 << b0), ru.big_random(rng, 1 << b1) + 1
        c, s = _check_estimate(r0, r1)
        if r0 >= r1:                                                # and close: a quotient below 2^24 is met to two, a longer one in its top bit at least
            q = r0 // r1
            assert 2 * c * ru.BASE ** s >= q - 2
            if q < ru.BASE:
                assert s == 0 and q - 2 <= c <= q
    for _ in range(500):                                            # equal in the top limbs, different below
        n = int(rng.integers(2, 9))
        head = (ru.big_random(rng, ru.BASE - 1) + 1) * ru.BASE ** (n - 1)
        for k in (1, 2):
            if n > k:
                head2 = head + ru.big_random(rng, ru.BASE ** k) * ru.BASE ** (n - 1 - k)
                lo = ru.BASE ** (n - 1 - k)
                _check_estimate(head2 + ru.big_random(rng, lo), head2 + ru.big_random(rng, lo))


@pytest.mark.parametrize("s", (0, 1, 3))
@pytest.mark.parametrize("c", (1, 2 ** 24 - 1))
def test_host_multiply_subtract_and_add(s, c):
    rng = np.random.default_rng(100 * s + (c & 7))
    for l1 in (1, 2, 5):
        for _ in range(40):
            r1 = ru.big_random(rng, ru.BASE ** l1 - 1) + 1
            prod = c * ru.BASE ** s * r1
            for r0 in (prod, prod + 1, prod + ru.big_random(rng, ru.BASE ** (l1 + s)), prod * 3 + 5, prod + ru.BASE ** (l1 + s + 3)):
                got, n = ru.host_submul(r0, c, s, r1)
                assert got == r0 - prod and n == ru.length(r0 - prod)
            for r0 in (prod - 1, prod // 2, 0):                     # a negative result is reported
                assert ru.host_submul(r0, c, s, r1) == (None, -1)
            cap = l1 + s + 6
            for u0 in (0, 1, ru.big_random(rng, ru.BASE ** (l1 + s)), ru.BASE ** (l1 + s + 2) - 1, ru.BASE ** (cap - 1)):
                got, n = ru.host_addmul(u0, c, s, r1, cap, junk=12345)           # (what lies above the length of u0 is not read)
                assert got == u0 + prod and n == ru.length(u0 + prod)
            full = ru.BASE ** (l1 + s + 1) - 1                      # a sum that needs one limb more than the row has
            assert ru.host_addmul(full, c, s, ru.BASE ** l1 - 1, l1 + s + 1) == (None, -1)
    got, n = ru.host_addmul(5, c, 3, 7, 8, junk=999)                # the shift above the length: the limbs between become zeros
    assert got == 5 + c * ru.BASE ** 3 * 7 and n == ru.length(got)


@pytest.mark.parametrize("p", (2, 3, 10007, ru.PMAX))
def test_host_residue_and_power(p):
    L, rng = ru.host_lib(), np.random.default_rng(p + 1)
    for n in (1, 2, 5, 70):
        for v in [0, ru.BASE ** n - 1] + [ru.big_random(rng, ru.BASE ** n) for _ in range(30)]:
            assert L.rec_residue_host(_pi(ru.digits(v, n)), ru.length(v), p) == v % p
    for K in (0, 1, 2, 3, 24, 25, 65, 66, 67, 134, 1000):
        bound = L.rec_power_bound_host(p, K)
        m = np.zeros(2 * bound + 2, np.int32)
        n = L.rec_power_host(p, K, _pi(m))
        assert n == ru.length(p ** K) <= bound and ru.value(m[:n]) == p ** K


def test_the_limb_counts_the_gpu_cases_rely_on():
    assert [ru.length(ru.PMAX ** K) for K in (1, 2, 3, 65, 66, 67, 134)] == [1, 2, 3, 63, 64, 65, 129]


# ---- a whole Euclid from the pieces -----------------------------------------------------------------------------------------------------------------------------
GPU_SHAPES = [(ru.PMAX, K, 5) for K in (1, 2, 3, 65, 66, 67, 134)] + [(2, 1, 5), (2, 24, 5), (2, 25, 5), (10007, 2, 5), (10007, 40, 5), (ru.PMAX, 67, 1), (ru.PMAX, 67, 130)]


@pytest.mark.parametrize("p,K,n", GPU_SHAPES)
def test_host_euclid_equals_the_oracle_on_the_gpu_cases(p, K, n):
    X, kinds, N, D = ru.mixed_case(p, K, n)
    m = p ** K
    x = ru.horner(X, p)
    steps = []
    for i, a in enumerate(x):
        got, out = ru.host_euclid(a, p, K, N, D)
        assert got == rounding.rational_reconstruction(a, m, N, D) and out[3] == 0
        if kinds[i] == "fraction" and D > 0:                        # (p = 2, one step: m = 2 and D = 0, nothing has a denominator within the bound)
            assert got is not None
        steps.append(out[2])
    assert "fraction" in kinds and (n == 1 or "random" in kinds)
    if (p, K, n) == (ru.PMAX, 67, 130):
        rnd = [s for s, k in zip(steps, kinds) if k == "random"]
        print("steps of the random entries at Lm = 65:", min(rnd), "to", max(rnd))
        assert 350 < min(rnd) and max(rnd) < 600                    # about 0.29 quotients per bit of m (Knuth 4.5.3: 0.584 per bit of the halfway point)


@pytest.mark.parametrize("name", list(ru.named_cases()))
def test_host_euclid_on_the_named_entries(name):
    a, N, D, want = ru.named_cases()[name]
    assert want == rounding.rational_reconstruction(a, ru.P67, N, D)
    got, out = ru.host_euclid(a, ru.PMAX, 67, N, D)
    assert got == want and out[3] == 0
    if name == "a=3, N=1":
        assert want is not None and (ru.P67 // 3).bit_length() == 1540 and out[4] == 64    # the first quotient: 1540 bits, taken from shift 64 down
    if name == "a=2^30+12345, N=2^20":
        assert (ru.P67 // a).bit_length() == 1511 and out[4] == 62
    if name in ("a=p", "D one below"):
        assert want is None


def test_coprimality_is_decided_by_p_alone():
    """gcd(r, t) at the stopping point is a power of p: `p divides both` is `gcd != 1` (sampled; DESIGN.md section 16 has the argument)"""
    rng = np.random.default_rng(11)
    for p, K in ((2, 12), (3, 9), (5, 7), (10007, 3)):
        m = p ** K
        for _ in range(400):
            a, N = int(rng.integers(0, m)), int(rng.integers(0, m))
            r0, r1, t0, t1 = m, a, 0, 1
            while r1 > N:
                q = r0 // r1
                r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
            assert (gcd(r1, abs(t1)) != 1) == (r1 % p == 0 and t1 % p == 0)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------------------------------
def test_linear_digit_conversion_round_trips():
    rng = np.random.default_rng(12)
    vals = [0, 1, ru.BASE - 1, ru.BASE, ru.BASE ** 2 - 1, 10 ** 40, ru.P67, ru.P67 - 1] + [ru.big_random(rng, 1 << int(b)) for b in rng.integers(1, 3000, 40)]
    for v in vals:
        d = rounding.to_digits24(v)
        assert d.dtype == np.int32 and d.tolist() == ru.digits(v).tolist() and rounding.from_digits24(d) == v
        assert rounding.from_digits24(rounding.to_digits24(v, d.size + 3)) == v
    rows = np.stack([ru.digits(v, 130) for v in vals])
    assert rounding.from_digits24(rows) == vals
    assert rounding.from_digits24(np.zeros((0, 4), np.int32)) == [] and rounding.from_digits24(np.zeros(3, np.int32)) == 0
    assert [int(v) for v in rounding.from_balanced_digits(rows.T)] == vals          # non-negative digits are balanced digits of one bit more: the Horner loop agrees
    with pytest.raises(ValueError):
        rounding.to_digits24(ru.BASE, 1)
    with pytest.raises(ValueError):
        rounding.to_digits24(-1)
    with pytest.raises(ValueError):
        rounding.from_digits24(np.array([1 << 24], np.int32))
    with pytest.raises(ValueError):
        rounding.from_digits24(np.array([-1], np.int32))


def test_fraction_without_a_second_gcd():
    f = rounding._coprime_fraction(-22, 7)
    assert f == F(-22, 7) and (f.numerator, f.denominator) == (-22, 7) and hash(f) == hash(F(-22, 7)) and f + F(1, 7) == -3
    assert rounding._coprime_fraction(0, 1) == 0


def host_reconstruct(X, p, N, D, device=0, want_x=False):
    """the stand-in for rounding.dixon_reconstruct: the same interface, Python integers"""
    host_reconstruct.calls.append(bool(want_x))
    x = ru.horner(np.asarray(X), p)
    out = [rounding.rational_reconstruction(v, p ** len(X), N, D) for v in x]
    return (out, x) if want_x else out


host_reconstruct.calls = []


def test_solve_dixon_with_a_reconstruct_stand_in():
    A = [[F(1, 2), F(1, 3), 0], [F(2, 5), 1, F(1, 7)], [0, F(3, 4), -2]]
    b = [F(3, 4), F(1, 2), 5]
    want = rounding.solve_dixon(A, b, lift=du.lift)
    host_reconstruct.calls.clear()
    got = rounding.solve_dixon(A, b, lift=du.lift, reconstruct=host_reconstruct)
    assert list(got) == list(want) == du.gauss_solve(A, b) and (got.p, got.primes, got.steps) == (want.p, want.primes, want.steps)
    assert host_reconstruct.calls == [True]                          # one call, and with check the integers are asked for
    assert list(rounding.solve_dixon(A, b, lift=du.lift, reconstruct=host_reconstruct, check=False)) == list(want) and host_reconstruct.calls == [True, False]
    A2, b2 = du.random_system(5, 9, 30, ru.PMAX)
    assert list(rounding.solve_dixon(A2, b2, lift=du.lift, reconstruct=host_reconstruct)) == list(rounding.solve_dixon(A2, b2, lift=du.lift))

    # the identity of the lifted integers is checked on what reconstruct returned
    def wrong_x(X, p, N, D, device=0, want_x=False):
        out, x = host_reconstruct(X, p, N, D, want_x=True)
        return (out, [x[0] + 1] + x[1:]) if want_x else out
    with pytest.raises(ArithmeticError, match="A x != b"):
        rounding.solve_dixon(A, b, lift=du.lift, reconstruct=wrong_x)
    assert list(rounding.solve_dixon(A, b, lift=du.lift, reconstruct=wrong_x, check=False)) == list(want)

    # an entry without a reconstruction is an error as on the host path
    def none(X, p, N, D, device=0, want_x=False):
        out, x = host_reconstruct(X, p, N, D, want_x=True)
        out[1] = None
        return (out, x) if want_x else out
    with pytest.raises(ArithmeticError, match="entry 1"):
        rounding.solve_dixon(A, b, lift=du.lift, reconstruct=none)


def test_pseudoinverse_and_projection_pass_reconstruct_down():
    A = [[1, 2, F(1, 2)], [0, 1, -1]]
    b = [F(3, 2), 4]
    host_reconstruct.calls.clear()
    assert rounding.solve_system_pseudoinverse(A, b, lift=du.lift, reconstruct=host_reconstruct) == rounding.solve_system_pseudoinverse(A, b, lift=du.lift)
    assert host_reconstruct.calls == [True]
    WA = [[F(1, 2), F(1, 3), 0, 1, 2, 1, 0, 3], [0, F(2, 5), 1, F(1, 7), 0, 2, 1, 1], [1, 0, 2, 0, 1, F(1, 3), 5, 0]]
    Wb = [F(3, 4), F(1, 2), 2]
    for s in (None, rounding.RoundingSettings(pseudo=False), rounding.RoundingSettings(pseudo_columnfactor=1.7)):
        host_reconstruct.calls.clear()
        want = rounding.project_to_affine_space(WA, Wb, settings=s, rng=np.random.default_rng(4), batch=mu.host_batch, lift=du.lift)
        got = rounding.project_to_affine_space(WA, Wb, settings=s, rng=np.random.default_rng(4), batch=mu.host_batch, lift=du.lift, reconstruct=host_reconstruct)
        assert got == want and got[1] and len(host_reconstruct.calls) == 1


# ---- the binding and the refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_symbol_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    table = {"int": C.c_int, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32, "double *": _lib.p_d}
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_dixon_reconstruct\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    args = [a.strip() for a in args.split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["device", "n", "p", "steps", "X", "nN", "N_limbs", "nD", "D_limbs", "nl", "num", "den", "neg", "status",
                                                                  "nx", "x_limbs", "info"]
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_dixon_reconstruct"] == (C.c_int, [table[re.sub(r"\w+$", "", a).strip()] for a in args])
    ret, args = re.search(r"^\s*(\w+)\s+clrs_modp_dixon_reconstruct_times\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    assert ret == "int" and _lib.SYMBOLS["clrs_modp_dixon_reconstruct_times"] == (C.c_int, [table[re.sub(r"\w+$", "", a.strip()).strip()] for a in args.split(",")])
    L = _lib.load()
    assert hasattr(L, "clrs_modp_dixon_reconstruct") and hasattr(L, "clrs_modp_dixon_reconstruct_times")
    for name in ("dixon_reconstruct", "to_digits24", "from_digits24"):
        assert name in rounding.__all__ and hasattr(rounding, name)


def test_refusals_need_no_device():
    """what clrs_modp_dixon_reconstruct refuses, it refuses before it touches a device, and it writes nothing"""
    L = _lib.load()
    X = np.array([[1, 2], [3, 4], [5, 6]], np.int32)                # steps = 3, n = 2, p = 13: m = 2197, one limb
    Nl, Dl = np.array([33], np.int32), np.array([33, 0], np.int32)
    num, den, neg, status, xl, info = (np.full(s, ru.SENTINEL, np.int32) for s in ((2, 1), (2, 1), (2,), (2,), (2, 1), (4,)))

    def call(n=2, p=13, steps=3, X=X, nN=1, N=Nl, nD=2, D=Dl, nl=1, num=num, den=den, neg=neg, status=status, nx=1, xl=xl, info=info):
        return L.clrs_modp_dixon_reconstruct(0, n, p, steps, _pi(X), nN, _pi(N), nD, _pi(D), nl, _pi(num), _pi(den), _pi(neg), _pi(status), nx, _pi(xl), _pi(info))
    for p in (1, 4, 10005, 2 ** 23 + 9, -7):
        assert call(p=p) == -1
    assert call(n=-1) == -1 and call(n=32768) == -1 and call(steps=0) == -1 and call(steps=-2) == -1
    assert call(X=np.array([[1, 2], [3, 13], [5, 6]], np.int32)) == -1 and b"residue" in L.clrs_last_error()
    assert call(X=np.array([[1, 2], [3, -1], [5, 6]], np.int32)) == -1
    assert call(N=np.array([1 << 24], np.int32)) == -1 and call(D=np.array([3, -1], np.int32)) == -1 and b"digit" in L.clrs_last_error()
    assert call(nN=0) == -1 and call(nD=0) == -1 and call(nl=0) == -1
    assert call(D=np.array([33, 1], np.int32)) == -1 and b"nl" in L.clrs_last_error()            # D needs two limbs, nl = 1
    assert call(nx=0) == -1 and b"nx" in L.clrs_last_error()
    assert call(p=8388593, steps=40000) == -1                       # more than 32767 limbs (refused before X is read)
    for name in ("X", "N", "D", "num", "den", "neg", "status", "info"):
        assert call(**{name: None}) == -1 and b"null" in L.clrs_last_error()
    assert all(int(v) == ru.SENTINEL for a in (num, den, neg, status, xl, info) for v in a.flat)
    assert L.clrs_modp_dixon_reconstruct(0, 0, 13, 3, None, 1, None, 1, None, 1, None, None, None, None, 0, None, _pi(info)) == 0 and info.tolist() == [0, 0, 0, 0]
    assert L.clrs_modp_dixon_reconstruct(0, 0, 13, 3, None, 1, None, 1, None, 1, None, None, None, None, 0, None, None) == 0
    assert L.clrs_modp_dixon_reconstruct_times(None, None) == -1
    with pytest.raises(ValueError):
        rounding.dixon_reconstruct(X, 4, 33, 33)
    with pytest.raises(ValueError):
        rounding.dixon_reconstruct(X[0], 13, 33, 33)
    with pytest.raises(ValueError):
        rounding.dixon_reconstruct(X, 13, -1, 33)
    assert rounding.dixon_reconstruct(np.zeros((3, 0), np.int32), 13, 33, 33) == [] and rounding.dixon_reconstruct(np.zeros((3, 0), np.int32), 13, 33, 33, want_x=True) == ([], [])


def test_no_cpu_fallback_without_a_device():
    """without a device the call raises; with one it computes (this test never skips)"""
    import torch
    X = ru.padic_digits(pow(3, -1, 13 ** 3), 13, 3)
    if torch.cuda.is_available():
        assert rounding.dixon_reconstruct(X, 13, 33, 33) == [F(1, 3)]
    else:
        with pytest.raises(_lib.ClrsError):
            rounding.dixon_reconstruct(X, 13, 33, 33)

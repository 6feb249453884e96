"""CPU side of the batched LLL reduction and of the reduced, unimodular basis change (clrs_zz_lll, clrs_amd.rounding): the arithmetic of
csrc/clrs_zz_lll_arith.h compiled for the host against Python integers, whole reductions by the host restatement of the kernel, the embedding of the kernel
lattice, the ladder, and `basis_transformations` / `exact_solution` with `reduce=`.  Every comparison is exact.  The kernel's parameters are
(delta, eta) = (0.99, 0.51); what is asserted is exact (0.98, 0.52)-reducedness (tests/lll_util.py)."""
import functools
from fractions import Fraction as F

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib, rounding
from clrs_amd import problems as P
from tests import dixon_multi_util as dm
from tests import lll_util as lu
from tests import lrsys_util as lru
from tests import modp_util as mu

HOOKS = dict(lift=dm.lift_columns, batch=mu.host_batch)
OVERFLOWING = [[1401898, -1844243], [7980587, 7964023]]          # one digit per entry; the first row operation leaves it


def _limb_sum(col):
    return sum((F(float(v)) for v in col), F(0))


# ---- the pieces ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limbs", rounding.LLL_LIMBS)
def test_conversion_at_digit_boundaries(limbs):
    nd = 20
    conv = dict(zip(rounding.LLL_LIMBS, lu.host_constants()[5:8]))[limbs]
    assert conv == (53 * limbs + 23) // 24 + 2
    rng = np.random.default_rng(limbs)
    values = [0, 1, -1, 1 << 23, -(1 << 23), (1 << 23) - 1, 1 - (1 << 23), (1 << 23) + 1]
    for k in (1, 2, 3, 7, 11, 19):
        values += [1 << (24 * k), -(1 << (24 * k)), (1 << (24 * k)) + 1, (1 << (24 * k)) - 1, -(1 << (24 * k)) - 1, (1 << (24 * k - 1)), -(1 << (24 * k - 1)) + 1]
    values += [int.from_bytes(rng.bytes(int(b)), "little") * (-1) ** i for i, b in enumerate(rng.integers(1, 59, size=40))]
    got = lu.host_entries(values, limbs, nd)
    digits = rounding.ints_to_planes(np.array(values, dtype=object), nd)
    for e, v in enumerate(values):
        col = [int(x) for x in digits[:, e]]
        top = max([s for s in range(nd) if col[s]], default=-1)
        kept = sum(col[s] << (24 * s) for s in range(max(top - conv + 1, 0), top + 1))          # the top `conv` digits, exactly
        assert abs(v - kept) < (1 << (24 * max(top - conv + 1, 0))) or v == kept
        total = _limb_sum(got[:, e])
        if abs(kept).bit_length() <= 53 * limbs - limbs:
            assert total == kept, (v, limbs)
        else:
            assert abs(total - kept) <= F(abs(kept), 1 << (53 * limbs - limbs - 2)), (v, limbs)
        assert all(abs(got[l + 1, e]) <= abs(got[l, e]) * 2.0 ** -52 for l in range(limbs - 1))          # non-overlapping limbs


def test_quotient_split_from_below_one_to_2_200():
    rng = np.random.default_rng(3)
    mus = [0.0, 0.3, -0.49, 0.5, -0.5, 0.51, 0.75, 1.5, -2.5, 2.0 ** 23, 2.0 ** 23 + 0.5, -(2.0 ** 24) - 1, 2.0 ** 52 + 1, 2.0 ** 53, -(2.0 ** 53) - 2, 3 * 2.0 ** 60,
           2.0 ** 76 - 2.0 ** 24, 2.0 ** 200, -(2.0 ** 200) * (1 + 2.0 ** -52), (2.0 ** 53 - 1) * 2.0 ** 147]
    mus += [float(np.ldexp(rng.uniform(0.5, 1.0) * (-1) ** e, int(e))) for e in range(0, 201, 3)]
    X, xd, sh, bad = lu.host_split(mus)
    for i, m in enumerate(mus):
        want = int(np.rint(m))                       # ties to even, as the kernel's rint
        assert int(bad[i]) == 0 and int(X[i]) == want
        assert all(abs(int(v)) <= 1 << 23 for v in xd[i]) and int(sh[i]) >= 0
        assert sum(int(xd[i][t]) << (24 * (t + int(sh[i]))) for t in range(4)) == want, m
    assert [int(b) for b in lu.host_split([float("nan"), float("inf"), -float("inf")])[3]] == [1, 1, 1]


def test_row_update_with_carries_and_a_planted_overflow():
    rng = np.random.default_rng(9)
    nd = 6
    big = lambda bits: int.from_bytes(rng.bytes(bits // 8), "little") * (-1) ** int(rng.integers(2))
    rows = lu._obj([[big(64) for _ in range(7)] for _ in range(4)])
    for X in ([3.0, -2.0, 0.0], [2.0 ** 40, -(2.0 ** 24) - 5, 1.0], [float(2 ** 53 + 2), 0.0, -(2.0 ** 30)]):
        got, over, _ = lu.host_update(rows, 3, X, nd)
        want = rows.copy()
        want[3] = rows[3] - sum(int(x) * rows[j] for j, x in enumerate(X))
        assert over == 0 and (got == want).all()
    # into the top digit: the result needs all nd digits, and one more bit does not fit
    edge = lu._obj([[1, 0], [0, 0]])
    edge[1, 0] = (1 << (24 * nd - 2))
    got, over, _ = lu.host_update(edge, 1, [-float(2 ** 30)], nd)                       # 2^142 + 2^30: fits
    assert over == 0 and got[1, 0] == (1 << 142) + (1 << 30)
    edge[0, 0] = 1 << 100
    got, over, _ = lu.host_update(edge, 1, [-float(2 ** 43)], nd)                       # 2^142 + 2^143 leaves six balanced digits
    assert over == 1 and got is None
    got, over, _ = lu.host_update(edge, 1, [-float(2 ** 100)], nd)                      # 2^200: the product lies wholly above the planes
    assert over == 1


# ---- whole reductions by the host restatement -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reduced(name):
    """(A, cols_gram, out, U or None, info) of a case, through rounding.lll_batch on the host build"""
    A, g = next((a, g) for n, a, g in lu.whole_cases() + lu.boundary_cases() if n == name)
    transform = A.shape[1] + A.shape[0] <= rounding.LLL_MAX_COLS
    res = rounding.lll_batch([A], transform=transform, cols_gram=None if g is None else [g], call=lu.host_call)[0]
    out, U = res if transform else (res, None)
    return A, g, out, U, rounding.lll_batch.last_info[0]


@pytest.mark.parametrize("name", [n for n, _, _ in lu.whole_cases() + lu.boundary_cases()])
def test_whole_reductions(name):
    A, g, out, U, info = _reduced(name)
    lu.assert_properties(A, out, U, cols_gram=g)
    assert info["status"] == 0 and info["launches"] >= 1 and info["swaps"] >= 0 and info["passes"] >= 0
    assert info["limbs"] == rounding.lll_first_rung(max(abs(int(v)).bit_length() for v in A.flat), A.shape[0])
    if U is None:                        # too wide for the identity: the same lattice by its Gram determinant (out is made of integer row operations)
        assert lu.det_fraction(lu.matmul_int(out, out.T)) == lu.det_fraction(lu.matmul_int(A, A.T))
    if name in ("identity", "d1"):
        assert info["swaps"] == 0 and info["passes"] == 0 and (out == A).all()
    if name == "big-quotient":
        assert info["swaps"] == 0 and info["passes"] >= 2 and [list(r) for r in out] == [[1, 0], [0, 1]]          # 2^100 + 3 takes two quotients of 53 bits
    if name == "swaps-all-the-way-back":
        assert info["swaps"] == 15 and [list(r) for r in out] == [[int(i == j) << (i + 1) for j in range(5, -1, -1)] for i in range(6)]
    if name == "knapsack":
        x = lu.knapsack()[1] + [0]
        assert any(list(r) in (x, [-v for v in x]) for r in out)


def test_the_result_does_not_depend_on_the_launches():
    A = lu.scrambled(117, 17)
    digits = rounding.ints_to_planes(A, 3)
    runs = [lu.host_call([17], [17], [17], 3, digits, lu.DELTA, lu.ETA, 2, 1 << 20, launch_swaps=n) for n in (1, 7, lu.LAUNCH_SWAPS)]
    swaps = int(runs[0][1][0][1])
    assert swaps > 100
    for (out, info), n in zip(runs, (1, 7, lu.LAUNCH_SWAPS)):
        assert (out == runs[0][0]).all() and [int(v) for v in info[0][:3]] == [0, swaps, int(runs[0][1][0][2])]
        assert int(info[0][3]) == swaps // n + 1


def test_every_rung_on_one_input():
    A = lu.scrambled(108, 8)
    for K in rounding.LLL_LIMBS:
        out, U = rounding.lll(A, transform=True, limbs=K, call=lu.host_call)
        lu.assert_properties(A, out, U)
        assert rounding.lll_batch.last_info[0]["rungs"] == [(K, 2, 0)]


def test_status_3_leaves_the_output_untouched_and_lll_batch_takes_more_digits():
    A = lu._obj(OVERFLOWING)
    out, info = lu.host_call([2], [2], [2], 1, rounding.ints_to_planes(A, 1), lu.DELTA, lu.ETA, 2, 1000)
    assert int(info[0][0]) == 3 and (out == lu.SENTINEL).all()
    calls = []

    def one_digit_first(rows, cols, cols_gram, nd, digits, *a, **kw):
        calls.append(nd)
        if len(calls) == 1:
            return np.zeros_like(digits), np.array([[3, 0, 1, 1, 1, 0, 0, 0]], np.int32)
        return lu.host_call(rows, cols, cols_gram, nd, digits, *a, **kw)

    red, U = rounding.lll(A, transform=True, call=one_digit_first)
    lu.assert_properties(A, red, U)
    assert calls == [3, 5] and [r[2] for r in rounding.lll_batch.last_info[0]["rungs"]] == [3, 0]
    with pytest.raises(rounding.ReductionError, match="digits"):
        rounding.lll(A, call=lambda rows, cols, g, nd, digits, *a, **kw: (np.zeros_like(digits), np.array([[3, 0, 0, 1, 0, 0, 0, 0]], np.int32)))


def test_the_ladder_escalates_one_lattice_and_gives_up_past_the_last_rung():
    A, small = lu.ladder_input(), lu.scrambled(103, 3)
    (out, U), (out2, U2) = rounding.lll_batch([A, small], transform=True, limbs=2, call=lu.host_call)
    lu.assert_properties(A, out, U)
    lu.assert_properties(small, out2, U2)
    rungs = [i["rungs"] for i in rounding.lll_batch.last_info]
    print("ladder:", rungs)
    assert rungs[0][0][0] == 2 and rungs[0][0][2] in (1, 2) and rungs[0][-1][2] == 0 and rungs[0][-1][0] > 2
    assert len(rungs[1]) == 1 and rungs[1][0][0] == 2 and rungs[1][0][2] == 0                # the other lattice of the batch is not repeated
    assert rounding.lll_first_rung(max(abs(int(v)).bit_length() for v in A.flat), 16) == 6     # the rule itself starts this input on the last rung
    tried = []

    def never(rows, cols, g, nd, digits, delta, eta, limbs, max_swaps, device=0):
        tried.append(limbs)
        return np.zeros_like(digits), np.array([[2, 0, 0, 1, 0, 0, 0, 0]] * len(rows), np.int32)

    with pytest.raises(rounding.ReductionError, match="last rung"):
        rounding.lll(small, call=never)
    assert tried == [2, 4, 6]


def test_lll_batch_refuses_what_the_entry_would():
    with pytest.raises(ValueError):
        rounding.lll_batch([lu.identity(3)], limbs=3, call=lu.host_call)
    with pytest.raises(ValueError):
        rounding.lll_batch([np.zeros((2, 255), dtype=object)], transform=True, call=lu.host_call)
    with pytest.raises(ValueError):
        rounding.lll_batch([[[0.5, 1.0]]], call=lu.host_call)
    assert rounding.lll_batch([], call=lu.host_call) == [] and rounding.lll_batch.last_info == []
    assert rounding.lll_first_rung(10, 8) == 2 and rounding.lll_first_rung(40, 9) == 2 and rounding.lll_first_rung(41, 9) == 4 and rounding.lll_first_rung(100, 24) == 6 and rounding.lll_first_rung(9999, 3) == 6


# ---- the embedding ---------------------------------------------------------------------------------------------------------------------------------------------
def test_kernel_lattice_and_its_lambda():
    M = lu._obj([[3, -1, 2, 0]])
    rows, q = rounding.kernel_lattice(4, 3, M, 2 ** 20)
    assert q == 1 and rows.shape == (4, 5) and [int(v) for v in rows[:, 0]] == [3 << 24, -(1 << 24), 2 << 24, 0] and (rows[:, 1:] == lu.identity(4)).all()
    assert rounding.kernel_lattice(4, 3, M, 2 ** 20 + 1)[1] == 2                                 # 24 q >= ceil(3 / 2) + 21 + 2
    assert rounding.kernel_lattice(4, 3, M, 2 ** 20, q_extra=1)[1] == 2
    with pytest.raises(ValueError):
        rounding.kernel_lattice(4, 2, M, 5)


@pytest.mark.parametrize("name", [n for n, _ in lu.kernel_sets()])
def test_reduced_basis_transformations_on_the_host_build(name):
    kernels = dict(lu.kernel_sets())[name]
    rec = lu.Recording(lu.host_reduce)
    out = rounding.basis_transformations(kernels, rounding.RoundingSettings(), reduce=rec, **HOOKS)
    assert list(out) == list(kernels)
    it = iter(zip(rec.blocks, rec.U))
    for key, (N, vectors) in kernels.items():
        Bt, Binv, s = out[key]
        assert s == len(vectors) and Bt.shape == Binv.shape == (N, N)
        assert all(v.denominator == 1 for v in Binv.flat) and all(v.denominator == 1 for v in Bt.flat)
        assert dm.frac_matmul(Bt.T, Binv) == dm.identity(N)
        if s in (0, N):
            assert [list(r) for r in Bt] == dm.identity(N)
            continue
        (bN, bs, M, R), U = next(it)
        assert (bN, bs) == (N, s) and M.shape == (N - s, N) and (np.asarray(Bt, dtype=object) == U).all()
        assert all(v == 0 for v in lu.matmul_int(M, U[:s].T).flat)                              # the first s rows lie in the kernel of M
        assert abs(lu.det_fraction(U)) == 1 and lu.is_lll_reduced(U[:s])
        assert lu.rank_fraction(np.array([list(v) for v in vectors] + [list(r) for r in Bt[:s]], dtype=object)) == s       # the same Q-space
        assert all(i["status"] == 0 for i in rounding.reduce_kernel_vectors.last_info)
    if name in ("hand-made", "delsarte-dual", "delsarte-primal", "echelon-8-3", "echelon-12-5"):
        want = rounding.basis_transformations(kernels, rounding.RoundingSettings(), reduce=lu.fraction_reduce, **HOOKS)
        for key in kernels:                                                                      # the Fraction stand-in: the same kernel lattice, reduced too
            s = out[key][2]
            assert want[key][2] == s and all(v.denominator == 1 for v in want[key][1].flat) and dm.frac_matmul(want[key][0].T, want[key][1]) == dm.identity(kernels[key][0])
            assert lu.is_lll_reduced(np.asarray(want[key][0], dtype=object)[:s])
            both = np.array([list(r) for r in want[key][0][:s]] + [list(r) for r in out[key][0][:s]], dtype=object)
            assert s == 0 or lu.rank_fraction(both) == s


def test_reduce_kernel_vectors_on_blocks_given_directly():
    blocks, vectors = zip(*(lu.echelon_block(2000 + N, N, s) for N, s in lu.ECHELON_SIZES[:3]))
    Us = lu.host_reduce(list(blocks))
    for (N, s, M, R), U, vec in zip(blocks, Us, vectors):
        assert all(v == 0 for v in lu.matmul_int(M, U[:s].T).flat) and abs(lu.det_fraction(U)) == 1 and lu.is_lll_reduced(U[:s])
        assert lu.rank_fraction(np.array([list(v) for v in vec] + [list(r) for r in U[:s]], dtype=object)) == s
    with pytest.raises(ValueError):
        lu.host_reduce([(4, 0, np.zeros((4, 4), dtype=object), 1)])


def test_a_failed_verification_escalates_and_never_returns():
    (block, _), calls = lu.echelon_block(2008, 8, 3), []

    def wrong_twice(lattices, limbs=None, device=0):
        calls.append((limbs, int(lattices[0][0, 0]).bit_length() if lattices[0][0, 0] else None, lattices[0].shape))
        out = lu.host_lll_batch(lattices, limbs=limbs, device=device)
        if len(calls) <= 2:
            out = [o.copy() for o in out]
            out[0][0], out[0][7] = out[0][7].copy(), out[0][0].copy()                        # a row outside the kernel among the first s
        return out

    U = rounding.reduce_kernel_vectors([block], lll=wrong_twice)[0]
    assert all(v == 0 for v in lu.matmul_int(block[2], U[:3].T).flat)
    assert [c[0] for c in calls] == [None, None, 4]                                           # lambda 2^24 times as large, then the next rung
    with pytest.raises(rounding.ReductionError, match="verification"):
        rounding.reduce_kernel_vectors([block], lll=lambda lattices, limbs=None, device=0: [lu.identity(8 + 5)[:8] for _ in lattices])


def test_basis_transformations_with_a_stand_in_and_without():
    out = rounding.basis_transformations(lu.HAND_MADE, rounding.RoundingSettings(), reduce=lu.fraction_reduce, **HOOKS)
    for key, (N, vectors) in lu.HAND_MADE.items():
        Bt, Binv, s = out[key]
        assert s == len(vectors) and all(v.denominator == 1 for v in Binv.flat) and dm.frac_matmul(Bt.T, Binv) == dm.identity(N)
    assert [list(r) for r in out["full"][0]] == dm.identity(2) and out["full"][2] == 2 and out["none"][2] == 0
    for settings in (None, rounding.RoundingSettings()):
        with pytest.raises(NotImplementedError, match="reduce_kernelvectors.*(HNF|LLL)"):
            rounding.basis_transformations(lu.HAND_MADE, settings, **HOOKS)
    unreduced = rounding.RoundingSettings(reduce_kernelvectors=False)
    never = lambda *a, **kw: pytest.fail("reduce= is not called when the settings switch the reduction off")
    plain, hooked = rounding.basis_transformations(lu.HAND_MADE, unreduced, **HOOKS), rounding.basis_transformations(lu.HAND_MADE, unreduced, reduce=never, **HOOKS)
    assert all((plain[k][0] == hooked[k][0]).all() and (plain[k][1] == hooked[k][1]).all() for k in plain)


def test_verbose_prints_the_largest_entry(capsys):
    out = rounding.basis_transformations({"f": lu.HAND_MADE["fractions"]}, rounding.RoundingSettings(), reduce=lu.host_reduce, verbose=True, **HOOKS)
    largest = max(abs(v) for v in out["f"][0].flat)
    assert f"After reduction, the maximum number of the basis transformation matrix is {largest}" in capsys.readouterr().out
    out = rounding.basis_transformations({"e": (8, lu.echelon_kernels(1008, 8, 3))}, rounding.RoundingSettings(unimodular_transform=False), reduce=lu.host_reduce,
                                         verbose=True, **HOOKS)
    largest = max(abs(v) for v in out["e"][0].flat)                      # normalised: B holds fractions, and the largest ENTRY is printed, not a numerator
    assert f"matrix is {largest}\n" in capsys.readouterr().out


def test_unimodular_transform_false_replaces_the_vectors_only():
    settings = rounding.RoundingSettings(unimodular_transform=False)
    assert rounding.RoundingSettings().unimodular_transform is True
    kernels = {"f": lu.HAND_MADE["fractions"], "e": (8, lu.echelon_kernels(1008, 8, 3)), "none": (3, [])}
    rec = lu.Recording(lu.host_reduce)
    out = rounding.basis_transformations(kernels, settings, reduce=rec, **HOOKS)
    want = rounding.basis_transformations({k: (N, [[F(int(x)) for x in row] for row in dict(zip(["f", "e"], rec.U))[k][:len(v)]] if v else []) for k, (N, v) in kernels.items()},
                                          rounding.RoundingSettings(reduce_kernelvectors=False), **HOOKS)
    for key, (N, vectors) in kernels.items():
        Bt, Binv, s = out[key]
        assert s == len(vectors) and dm.frac_matmul(Bt.T, Binv) == dm.identity(N) and all(v.denominator == 1 for v in Binv.flat)
        assert (Bt == want[key][0]).all() and (Binv == want[key][1]).all()                     # the unreduced branch on the reduced vectors, normalised
    U = rec.U[0]
    plain = rounding.basis_transformations({"f": kernels["f"]}, rounding.RoundingSettings(unimodular_transform=False, normalize_transformation=False), reduce=lu.host_reduce, **HOOKS)
    assert [list(r) for r in plain["f"][0][:2]] == [[F(int(x)) for x in row] for row in U[:2]]
    assert all(sum(1 for x in r if x != 0) == 1 for r in plain["f"][0][2:])                       # completed by standard basis vectors


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_solution_with_the_default_settings_on_the_host(oracle_built):
    from tests.test_linear_system_cpu import _oracle_solution
    problem = P.delsarte_exact_problem(8, 3, F(1, 2))
    sol = rounding.exact_solution(problem, _oracle_solution(), rounding.RoundingSettings(), limbs=5, reduce=lu.host_reduce, **lru.host_hooks())
    lru.check_delsarte_exact_solution(problem, sol)
    assert sol.objective == 240 and [sol.Bs[k][2] for k in range(9)] == [1, 0, 0, 0, 0, 0, 0, 4, 2]
    assert all(v.denominator == 1 for k in range(9) for v in sol.Bs[k][1].flat)                # unimodular basis changes: nothing left to normalise
    with pytest.raises(NotImplementedError):
        rounding.exact_solution(problem, _oracle_solution(), limbs=5, **lru.host_hooks())


# ---- the entry: refusals before any device call, and the binding ------------------------------------------------------------------------------------------------
def _entry(rows=(2,), cols=(2,), gram=(2,), nd=1, digits=None, delta=0.99, eta=0.51, limbs=2, max_swaps=10, null=()):
    rows, cols, gram = (np.array(a, np.int32) for a in (rows, cols, gram))
    digits = np.array([1, 0, 0, 1], np.int32) if digits is None else np.ascontiguousarray(digits, np.int32)
    out, info = np.full(max(digits.size, 1), lu.SENTINEL, np.int32), np.full((max(rows.size, 1), 8), lu.SENTINEL, np.int32)
    ptr = lambda name, a: _lib.p_i32() if name in null else a.ctypes.data_as(_lib.p_i32)
    code = _lib.load().clrs_zz_lll(0, rows.size, ptr("rows", rows), ptr("cols", cols), ptr("gram", gram), nd, ptr("in", digits), ptr("out", out), delta, eta, limbs,
                                   max_swaps, ptr("info", info))
    return code, out, info


def test_refusals_need_no_device():
    INVALID = -1
    assert _lib.load().clrs_strerror(INVALID) != b"ok"
    refused = [dict(rows=(129,), cols=(2,), gram=(2,), digits=np.zeros(258)), dict(cols=(257,), gram=(2,), digits=np.zeros(514)), dict(rows=(-1,)), dict(cols=(-2,)),
               dict(gram=(3,)), dict(gram=(0,)), dict(gram=(-1,)), dict(nd=0), dict(nd=21, digits=np.zeros(84)), dict(limbs=3), dict(limbs=8), dict(limbs=0),
               dict(delta=0.25), dict(delta=1.5), dict(eta=0.4), dict(eta=0.995), dict(delta=float("nan")), dict(max_swaps=-1),
               dict(digits=[1, 0, 0, (1 << 23) + 1]), dict(digits=[1, 0, -(1 << 23) - 1, 1]),
               dict(null=("rows",)), dict(null=("cols",)), dict(null=("gram",)), dict(null=("in",)), dict(null=("out",)), dict(null=("info",))]
    for kw in refused:
        code, out, info = _entry(**kw)
        assert code == INVALID and (out == lu.SENTINEL).all() and (info == lu.SENTINEL).all(), kw
        assert b"zz_lll" in _lib.load().clrs_last_error()
    # 2^31 elements or more: 20 digits of 128 x 256, 3277 lattices
    n = 3277
    code = _lib.load().clrs_zz_lll(0, n, *(np.full(n, v, np.int32).ctypes.data_as(_lib.p_i32) for v in (128, 256, 256)), 20, _lib.p_i32(), _lib.p_i32(), 0.99, 0.51, 2, 10,
                                   np.zeros((n, 8), np.int32).ctypes.data_as(_lib.p_i32))
    assert code == INVALID and b"2^31" in _lib.load().clrs_last_error()
    assert _lib.load().clrs_zz_lll(-1, -1, *([_lib.p_i32()] * 3), 1, _lib.p_i32(), _lib.p_i32(), 0.99, 0.51, 2, 10, _lib.p_i32()) == INVALID
    # nothing to do: no device is touched (there is none here), the digits at +-2^23 are accepted
    assert _lib.load().clrs_zz_lll(0, 0, *([_lib.p_i32()] * 3), 1, _lib.p_i32(), _lib.p_i32(), 0.99, 0.51, 2, 10, _lib.p_i32()) == 0
    code, out, info = _entry(rows=(0, 0), cols=(3, 0), gram=(0, 0), digits=np.zeros(0))
    assert code == 0 and [list(r) for r in info] == [[0] * 8] * 2
    t = np.full(2, -1.0)
    assert _lib.load().clrs_zz_lll_times(t[0:].ctypes.data_as(_lib.p_d), t[1:].ctypes.data_as(_lib.p_d)) == 0 and list(t) == [0.0, 0.0]
    assert _lib.load().clrs_zz_lll_times(_lib.p_d(), _lib.p_d()) == INVALID


def test_binding_and_knob():
    import ctypes as C
    assert _lib.SYMBOLS["clrs_zz_lll"] == (C.c_int, [C.c_int, C.c_int, _lib.p_i32, _lib.p_i32, _lib.p_i32, C.c_int, _lib.p_i32, _lib.p_i32, C.c_double, C.c_double, C.c_int,
                                                     C.c_int, _lib.p_i32])
    assert _lib.SYMBOLS["clrs_zz_lll_times"] == (C.c_int, [_lib.p_d, _lib.p_d])
    L = _lib.load()
    assert L.clrs_config_set(b"lll_launch_swaps", 7) == 0 and L.clrs_config_set(b"lll_launch_swaps", 0) == 0
    assert any(unit[1] == "clrs_zz_lll.hip" and "-ffp-contract=off" in unit[2] for unit in _lib._UNITS)
    assert {"lll", "lll_batch", "reduce_kernel_vectors", "ReductionError"} <= set(rounding.__all__)
    jl = open(_lib.os.path.join(_lib._HERE, "..", "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    assert ":clrs_zz_lll," in jl and "function lll(" in jl

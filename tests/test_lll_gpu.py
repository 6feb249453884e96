"""GPU tests of the batched LLL reduction clrs_zz_lll and of the reduced, unimodular basis change on the device.  Outputs are filled
with sentinels before every call; the digits and the counters are compared with `==` against the host build of the same arithmetic
(tests/mw_host/lll_host.cpp), and what is asserted of every reduced lattice is exact (tests/lll_util.py)."""
import functools
from fractions import Fraction as F

import numpy as np
import pytest

from clrs_amd import _lib, rounding
from tests import dixon_multi_util as dm
from tests import lll_util as lu
from tests import lrsys_util as lru
from tests import modp_util as mu

pytestmark = pytest.mark.gpu
MAX_SWAPS = 1 << 22


def _both(lattices, grams, nd, limbs, max_swaps=MAX_SWAPS):
    """one batch through the device and through the host build: (digits, device out, device info, host out, host info, shapes)"""
    planes = [rounding.ints_to_planes(A, nd) for A in lattices]
    digits = np.concatenate([p.reshape(-1) for p in planes])
    rows, cols = [A.shape[0] for A in lattices], [A.shape[1] for A in lattices]
    dev = lu.device_call(rows, cols, grams, nd, digits, lu.DELTA, lu.ETA, limbs, max_swaps)
    host = lu.host_call(rows, cols, grams, nd, digits, lu.DELTA, lu.ETA, limbs, max_swaps)
    return digits, dev, host, [p.shape for p in planes]


def _case_args(A, g):
    """the lattice with the identity beside it where it fits, its Gram columns, digits and rung as rounding.lll_batch chooses them"""
    d, c = A.shape
    wide = np.concatenate([A, lu.identity(d)], axis=1) if c + d <= rounding.LLL_MAX_COLS else A
    bits = max(abs(int(v)).bit_length() for v in wide.flat)
    return wide, (c if g is None else g), (bits + 40) // 24 + 1, rounding.lll_first_rung(bits, d)


@pytest.mark.parametrize("name", [n for n, _, _ in lu.whole_cases() + lu.boundary_cases()])
def test_whole_reductions_equal_the_host_build(name):
    A, g = next((a, g) for n, a, g in lu.whole_cases() + lu.boundary_cases() if n == name)
    wide, gram, nd, limbs = _case_args(A, g)
    digits, (out, info), (hout, hinfo), shapes = _both([wide], [gram], nd, limbs)
    assert int(info[0][0]) == 0 and (info == hinfo).all() and (out == hout).all()                    # digit for digit, counter for counter
    again, info2 = lu.device_call([wide.shape[0]], [wide.shape[1]], [gram], nd, digits, lu.DELTA, lu.ETA, limbs, MAX_SWAPS)
    assert (again == out).all() and (info2 == info).all()                                            # two runs identical
    red = rounding.planes_to_ints(out.reshape(shapes[0]))
    c = A.shape[1]
    if wide.shape[1] > c:
        lu.assert_properties(A, red[:, :c], red[:, c:], cols_gram=g)
    else:
        assert lu.is_lll_reduced(red) and lu.det_fraction(lu.matmul_int(red, red.T)) == lu.det_fraction(lu.matmul_int(A, A.T))
    if name == "identity":
        assert int(info[0][1]) == 0 and int(info[0][3]) == 1
    t = np.zeros(2)
    assert _lib.load().clrs_zz_lll_times(t[0:].ctypes.data_as(_lib.p_d), t[1:].ctypes.data_as(_lib.p_d)) == 0 and 0 < t[0] <= t[1]


def _embedded_lattices():
    """(blocks, vectors): the echelon blocks given directly and the blocks basis_transformations forms of the hand-made and golden kernels, each with the
    rational kernel vectors it came from"""
    blocks, vectors = (list(t) for t in zip(*(lu.echelon_block(2000 + N, N, s) for N, s in lu.ECHELON_SIZES)))
    rec = lu.Recording(lu.host_reduce)
    for _, kernels in lu.kernel_sets()[:3]:
        rounding.basis_transformations(kernels, rounding.RoundingSettings(), reduce=rec, lift=dm.lift_columns, batch=mu.host_batch)
        vectors += [vec for N, vec in kernels.values() if 0 < len(vec) < N]
    return blocks + rec.blocks, vectors


def test_embedded_kernel_lattices_equal_the_host_build():
    blocks, vectors = _embedded_lattices()
    lattices = [rounding.kernel_lattice(*b)[0] for b in blocks]
    rows, cols = [L.shape[0] for L in lattices], [L.shape[1] for L in lattices]
    nd = max((max(abs(int(v)).bit_length() for v in L.flat) + 40) // 24 + 1 for L in lattices)
    for limbs in (2, 6):
        digits, (out, info), (hout, hinfo), shapes = _both(lattices, cols, nd, limbs)
        assert (info[:, 0] == 0).all() and (info == hinfo).all() and (out == hout).all()
        again, info2 = lu.device_call(rows, cols, cols, nd, digits, lu.DELTA, lu.ETA, limbs, MAX_SWAPS)
        assert (again == out).all() and (info2 == info).all()                                          # two runs identical
        off = 0
        for (N, s, M, R), vec, shape in zip(blocks, vectors, shapes):
            count = int(np.prod(shape))
            red = rounding.planes_to_ints(out[off:off + count].reshape(shape))
            off += count
            left, U = red[:, :N - s], red[:, N - s:]
            assert all(v == 0 for v in left[:s].flat) and all(any(v != 0 for v in left[i]) for i in range(s, N))
            assert all(v == 0 for v in lu.matmul_int(M, U[:s].T).flat) and abs(lu.det_fraction(U)) == 1 and lu.is_lll_reduced(U[:s])
            assert lu.rank_fraction(np.array([list(v) for v in vec] + [list(r) for r in U[:s]], dtype=object)) == s          # the same Q-space
            if limbs == 2:                                                                                 # B = U^T: its inverse over QQ is an integer matrix
                Binv = rounding.inverse_qq(U.T, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul)
                assert all(v.denominator == 1 for v in np.asarray(Binv).flat) and (lu.matmul_int(U.T, np.asarray(Binv)) == lu.identity(N)).all()


def test_a_batch_of_mixed_sizes_equals_the_single_calls():
    sizes = [(1 + (5 * i) % 13, 0) for i in range(70)]
    lattices = [np.concatenate([lu.scrambled(300 + i, d), lu.identity(d)], axis=1) for i, (d, _) in enumerate(sizes)]
    lattices[3], lattices[40] = np.zeros((0, 0), dtype=object), np.zeros((0, 5), dtype=object)              # lattices without rows inside the batch
    grams = [L.shape[1] - L.shape[0] for L in lattices]
    nd = 3
    digits, (out, info), (hout, hinfo), shapes = _both(lattices, grams, nd, 2)
    assert (info[:, 0] == 0).all() and (info == hinfo).all() and (out == hout).all()
    off = 0
    for i, (L, shape) in enumerate(zip(lattices, shapes)):
        count = int(np.prod(shape))
        if count:                                                                                          # every lattice against its own call
            single, sinfo = lu.device_call([L.shape[0]], [L.shape[1]], [grams[i]], nd, digits[off:off + count], lu.DELTA, lu.ETA, 2, MAX_SWAPS)
            assert (single == out[off:off + count]).all() and (sinfo[0] == info[i]).all(), i
            if i % 7 == 0:                                                                                 # the exact properties on every seventh
                red = rounding.planes_to_ints(single.reshape(shape))
                d = L.shape[0]
                lu.assert_properties(L[:, :d], red[:, :d], red[:, d:])
        off += count
    assert [int(v) for v in info[3]] == [0] * 8 and [int(v) for v in info[40]] == [0] * 8


def test_launches_of_1_and_7_exchanges_and_the_default():
    A = lu.scrambled(117, 17)
    digits = rounding.ints_to_planes(A, 3)
    L = _lib.load()
    runs = []
    try:
        for n in (1, 7, 0):
            assert L.clrs_config_set(b"lll_launch_swaps", n) == 0
            runs.append(lu.device_call([17], [17], [17], 3, digits, lu.DELTA, lu.ETA, 2, MAX_SWAPS))
    finally:
        L.clrs_config_set(b"lll_launch_swaps", 0)
    swaps = int(runs[0][1][0][1])
    for (out, info), n in zip(runs, (1, 7, lu.LAUNCH_SWAPS)):
        assert (out == runs[0][0]).all() and int(info[0][0]) == 0 and int(info[0][1]) == swaps and int(info[0][2]) == int(runs[0][1][0][2])
        assert int(info[0][3]) == swaps // n + 1
        hout, hinfo = lu.host_call([17], [17], [17], 3, digits, lu.DELTA, lu.ETA, 2, MAX_SWAPS, launch_swaps=n)
        assert (hout == out).all() and (hinfo == info).all()
    assert swaps > 100 and lu.is_lll_reduced(rounding.planes_to_ints(runs[0][0].reshape(3, 17, 17)))


def test_every_rung_on_one_input():
    A = np.concatenate([lu.scrambled(108, 8), lu.identity(8)], axis=1)
    for limbs in rounding.LLL_LIMBS:
        digits, (out, info), (hout, hinfo), shapes = _both([A], [8], 2, limbs)
        assert int(info[0][0]) == 0 and (info == hinfo).all() and (out == hout).all()
        red = rounding.planes_to_ints(out.reshape(shapes[0]))
        lu.assert_properties(A[:, :8], red[:, :8], red[:, 8:])


def test_caps_and_overflow_leave_the_output_untouched():
    over = lu._obj([[1401898, -1844243], [7980587, 7964023]])
    digits, (out, info), (hout, hinfo), _ = _both([over], [2], 1, 2)
    assert int(info[0][0]) == 3 and (out == lu.SENTINEL).all() and (info == hinfo).all()
    A = lu.scrambled(117, 17)
    digits, (out, info), (hout, hinfo), _ = _both([A, lu.identity(4)], [17, 4], 3, 2, max_swaps=50)
    assert [int(v) for v in info[:, 0]] == [1, 0] and int(info[0][1]) == 50 and (info == hinfo).all() and (out == hout).all()
    assert (out[:3 * 17 * 17] == lu.SENTINEL).all() and (rounding.planes_to_ints(out[3 * 17 * 17:].reshape(3, 4, 4)) == lu.identity(4)).all()


def test_lll_and_the_ladder_on_the_device():
    A = lu.ladder_input()
    out, U = rounding.lll(A, transform=True, limbs=2)
    lu.assert_properties(A, out, U)
    rungs = rounding.lll_batch.last_info[0]["rungs"]
    hout, _ = rounding.lll(A, transform=True, limbs=2, call=lu.host_call)
    assert rungs == rounding.lll_batch.last_info[0]["rungs"] and rungs[0][2] in (1, 2) and rungs[-1][2] == 0 and (hout == out).all()


@functools.lru_cache(maxsize=None)
def _delsarte_solution():
    from tests.test_linear_system_gpu import _delsarte_solution as solve
    return solve()


def test_basis_transformations_of_the_device_solve_equal_the_host_stand_in():
    problem, res = _delsarte_solution()
    kernels = rounding.kernel_vectors(problem.block_n, res, res, rationalize=True)
    kernels = {bi: (int(n), rounding.vectors_to_fractions(k)) for bi, (n, k) in enumerate(zip(problem.block_n, kernels))}
    got = rounding.basis_transformations(kernels, rounding.RoundingSettings(), reduce=rounding.reduce_kernel_vectors, reconstruct=rounding.dixon_reconstruct,
                                         matmul=rounding.zz_matmul)
    assert all(i["status"] == 0 for i in rounding.reduce_kernel_vectors.last_info)
    want = rounding.basis_transformations(kernels, rounding.RoundingSettings(), reduce=lu.host_reduce, reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul)
    for key, (N, vectors) in kernels.items():
        assert got[key][2] == want[key][2] == len(vectors) and (got[key][0] == want[key][0]).all() and (got[key][1] == want[key][1]).all()
        assert all(v.denominator == 1 for v in got[key][1].flat) and dm.frac_matmul(got[key][0].T, got[key][1]) == dm.identity(N)


def test_exact_solution_with_the_default_settings_on_the_device():
    problem, res = _delsarte_solution()
    sol = rounding.exact_solution(problem, res, rounding.RoundingSettings(), reconstruct=rounding.dixon_reconstruct, matmul=rounding.zz_matmul,
                                  reduce=rounding.reduce_kernel_vectors)
    lru.check_delsarte_exact_solution(problem, sol)
    assert sol.objective == 240 and all(v.denominator == 1 for k in sol.Bs for v in sol.Bs[k][1].flat)

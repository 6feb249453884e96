"""The multi-word SPD solve on the device (clrs_mw_posv: k_mw_posv_diag and k_mw_gemm) against its host restatement bit for bit, on the systems of
tests/posv_util.py: the shapes and limb counts of the CPU test, the planted failing pivots, the write discipline, and the independence of the columns."""
import numpy as np
import pytest

from clrs_amd import _lib, mw
from tests import posv_util as pu

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("kind,K,n,nrhs", pu.cases(), ids=lambda v: str(v))
def test_device_is_the_host_restatement_bit_for_bit(kind, K, n, nrhs):
    """the same launches in the same order, every operation an IEEE add, multiply, fma, division or square root, contraction off; the sentinels behind
    X (in every plane) and behind info[1] stay"""
    s = pu.system(kind, K, n, nrhs)
    dev, dinfo = pu.run_device(s)
    host, hinfo = pu.run_host(s)
    diff = np.argwhere(dev.view(np.uint64) != host.view(np.uint64))
    print(kind, "K", K, "n", n, "nrhs", nrhs, "entries that differ from the host restatement:", len(diff), diff[:5].tolist())
    assert len(diff) == 0
    assert dinfo.tolist() == hinfo.tolist() == [0, (n + 15) // 16] + [-77] * 5
    assert np.all(dev[:, n * nrhs:] == pu.SENTINEL)


@pytest.mark.parametrize("col", pu.PLANTS)
def test_planted_failing_pivot_on_the_device(col):
    s = pu.planted(col)
    X, info = pu.run_device(s)
    assert info.tolist() == [1 + col, 4] + [-77] * 5
    assert np.all(X[:, :s.n * s.nrhs] == 0.0) and np.all(X[:, s.n * s.nrhs:] == pu.SENTINEL)
    A3 = np.transpose(s.A.reshape(s.K, s.n, s.n), (0, 2, 1))
    B3 = np.transpose(s.B.reshape(s.K, s.nrhs, s.n), (0, 2, 1))
    with pytest.raises(ArithmeticError, match=f"column {col} "):
        mw.posv(A3, B3, s.K)


def test_three_single_right_hand_sides_give_the_columns_of_one_call():
    s = pu.system("spd", 5, 49, 3)
    n = s.n
    A3 = np.transpose(s.A.reshape(5, n, n), (0, 2, 1))
    B3 = np.transpose(s.B.reshape(5, 3, n), (0, 2, 1))
    X, info = mw.posv(A3, B3, 5)
    assert X.shape == (5, n, 3) and info.tolist() == [0, 4]
    for c in range(3):
        Xc, _ = mw.posv(A3, B3[:, :, c:c + 1], 5)
        assert _same_bits(np.ascontiguousarray(Xc[:, :, 0]), np.ascontiguousarray(X[:, :, c]))
    host, _ = pu.host_solve(A3, B3, 5)
    assert _same_bits(X, host)
    mw.posv_times()                                  # the per-panel events are recorded from this thread's first request on
    Xt, _ = mw.posv(A3, B3, 5)
    assert _same_bits(Xt, X)
    d, g, w = mw.posv_times()
    assert 0 < d <= w and abs(d + g - w) <= 1e-9 * w

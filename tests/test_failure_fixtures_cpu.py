"""The fixtures of tests/test_factor_failures.py, checked on the host: matrices whose Cholesky factorisation fails at a chosen pivot (tests/util.py::ldl_fixture,
rank1_flip), placed into a chosen block, and the status the 320-bit oracle gives them."""
import numpy as np
import pytest

import clrs_amd
from tests.util import ldl_fixture, mw_with_tails, place_block, random_simple_sdp, rank1_flip, spd_iterates

PIVOTS = [0, 1, 7, 8, 9, 15, 16, 24, 31, 32, 33, 40, 47, 48, 63]


def _chol_ok(A):
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


@pytest.mark.parametrize("n", [9, 16, 33, 64])
def test_ldl_fixture_fails_exactly_at_the_chosen_pivot(n):
    for k in [k for k in PIVOTS if k < n]:
        M = ldl_fixture(n, k, seed=n + k)
        assert np.array_equal(M, M.T)
        assert k == 0 or _chol_ok(M[:k, :k])
        assert not _chol_ok(M[:k + 1, :k + 1]), (n, k)
        T = ldl_fixture(n, k, seed=n + k, variant="tiny")
        assert _chol_ok(T), (n, k)
        assert np.linalg.cholesky(T)[k, k] ** 2 == 2.0 ** -30        # the pivot is exact: nothing cancels in front of it


def test_rank1_flip_keeps_the_leading_block_and_fails_at_the_pivot():
    import mpmath as mp
    rng = np.random.default_rng(3)
    n, K = 32, 5
    G = rng.standard_normal((n, n))
    A = (np.eye(n) + G @ G.T / n).reshape(1, -1, order="F")
    A = np.vstack([A, np.zeros((K - 1, n * n))])
    for k in (0, 7, 8, 20, 31):
        F, Dk = rank1_flip(A, k, 1e-3)
        assert F.shape == (K, n * n) and Dk > 0
        F0 = F[0].reshape(n, n, order="F")
        assert np.array_equal(F0[:k, :k], A[0].reshape(n, n, order="F")[:k, :k])
        assert k == 0 or _chol_ok(F0[:k, :k])
        # pivot k of the K-limb matrix, at 400 bits: -eps D_k
        with mp.workprec(400):
            Fm = mp.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    Fm[i, j] = mp.fsum(mp.mpf(float(F[l, i + j * n])) for l in range(K))
            Lm = mp.cholesky(Fm[:k, :k]) if k else None
            s = Fm[k, k]
            if k:
                v = [Fm[i, k] for i in range(k)]
                w = mp.matrix(k, 1)
                for i in range(k):                       # forward substitution L w = F[:k, k]
                    w[i] = (v[i] - mp.fsum(Lm[i, m] * w[m] for m in range(i))) / Lm[i, i]
                s -= mp.fsum(w[i] ** 2 for i in range(k))
            assert abs(s / Dk + mp.mpf("1e-3")) < 1e-15, (k, s, Dk)     # (D_k comes back as fp64)


@pytest.mark.parametrize("K", [4, 5])
def test_the_oracle_names_the_first_failing_block(K, oracle_built):
    from oracle.oracle import Oracle
    f = clrs_amd.flatten(random_simple_sdp(7, J=3, max_n=33, lr_blocks=2))
    X, _ = spd_iterates(f, seed=2)
    X = mw_with_tails(X, K, seed=5)
    o = Oracle(f, mp_bits=320)
    big = [b for b in range(f.n_blocks) if int(f.block_n[b]) == 33]
    assert len(big) == 6
    st, _ = o.cholesky_blocks_mw(X)
    assert st == 0
    for k in (0, 8, 31, 32):
        for b in big[1:]:
            Xf = place_block(f, X, b, ldl_fixture(33, k, seed=b + k), K, seed=b)
            st, _ = o.cholesky_blocks_mw(Xf)
            assert st == b + 1, (k, b, st)
            Xt = place_block(f, X, b, ldl_fixture(33, k, seed=b + k, variant="tiny"), K, seed=b)
            st, _ = o.cholesky_blocks_mw(Xt)
            assert st == 0, (k, b, st)
        # two failing blocks: the smaller index is the status
        b1, b2 = big[2], big[4]
        Xf = place_block(f, place_block(f, X, b2, ldl_fixture(33, 1, seed=1), K), b1, ldl_fixture(33, k, seed=k), K)
        st, _ = o.cholesky_blocks_mw(Xf)
        assert st == b1 + 1

"""The reference of the step-length eigenvalue tests on its own (no GPU): over the whole case list LAPACK's `eigvalsh` passes the inertia check at the
tolerances test_step_eig_gpu.py uses, so the reference and the tolerances leave room for a correct routine; and a planted wrong answer -- the
second-smallest eigenvalue -- is rejected, so the check can fail."""
import numpy as np
import pytest

from tests.step_eig_util import (CASE_NAMES, assert_min_eig, cases_budget, check_min_eig, count_below, eig_cases, eig_tol, limbs_to_mp,
                                 planted_second_smallest, to_mp, wilkinson)

NS_32 = (2, 3, 4, 5, 6, 8, 9, 15, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 63, 64)      # forms 0 and 2 of the hook
NS_LDS = (1, 2, 3, 17, 64, 65, 80, 100, 128)                                          # form 1
ALL_NS = tuple(sorted(set(NS_32) | set(NS_LDS)))


def test_count_below_counts_eigenvalues():
    A = np.diag([3.0, -1.0, 0.5, -4.0])
    assert [count_below(A, s) for s in (-5.0, -2.0, 0.0, 1.0, 10.0)] == [0, 1, 2, 3, 4]
    rng = np.random.default_rng(0)
    G = rng.standard_normal((9, 9))
    S = G + G.T
    w = np.linalg.eigvalsh(S)
    for k in range(9):
        assert count_below(S, 0.5 * (w[k] + (w[k + 1] if k < 8 else w[k] + 2.0))) == k + 1
    # a pencil: eigenvalues of L^-1 S L^-T through (S, M = L L^T), no factorisation on this side
    L = np.tril(rng.standard_normal((9, 9)), -1) + np.diag(rng.uniform(1, 2, 9))
    M = L @ L.T
    Li = np.linalg.inv(L)
    wp = np.linalg.eigvalsh(Li @ S @ Li.T)
    for k in range(8):
        assert count_below(S, 0.5 * (wp[k] + wp[k + 1]), B=np.tril(M) + np.tril(M, -1).T) == k + 1


def test_the_case_list_is_complete():
    names = [k for k, _ in eig_cases(17)]
    assert names == list(CASE_NAMES) and len(names) == 16
    assert [k for k, _ in eig_cases(64, limit=cases_budget(64))] == list(CASE_NAMES[:6])
    assert all(cases_budget(n) == len(CASE_NAMES) for n in NS_32 if n <= 33) and all(cases_budget(n) <= 6 for n in ALL_NS if n >= 64)
    # the close pairs the list promises
    w = np.linalg.eigvalsh(-wilkinson(21))
    assert w[1] - w[0] < 1e-10 and w[2] - w[1] > 0.1


@pytest.mark.parametrize("n", ALL_NS)
def test_eigvalsh_is_inside_the_tolerance_on_every_case(n):
    for name, A in eig_cases(n, limit=cases_budget(n)):
        got = float(np.linalg.eigvalsh(A)[0])
        if name == "zero":
            assert got == 0.0
            continue
        assert_min_eig(got, A, eig_tol(n, A), what=f"n = {n}, {name}")


def test_a_planted_second_smallest_eigenvalue_is_rejected():
    A, l1, l2 = planted_second_smallest()
    tol = eig_tol(A.shape[0], A)
    assert l2 - l1 > 0.9
    assert check_min_eig(l1, A, tol) == (True, True)
    assert check_min_eig(l2, A, tol) == (False, True)                  # too large: something lies below it
    assert check_min_eig(l1 - 1e-3, A, tol) == (True, False)           # too small: nothing below it yet
    with pytest.raises(AssertionError, match="too LARGE"):
        assert_min_eig(l2, A, tol)
    # the same through a pencil, on exact limb sums: W0 = diag(-2, -1, 1), M = diag(4, 1, 1) -> eigenvalues of (M^1/2 W0 M^1/2, M) are those of W0
    M = np.diag([4.0, 1.0, 1.0])
    dM = np.diag([-8.0, -1.0, 1.0])
    Mm, dMm = limbs_to_mp(np.stack([M.reshape(-1), np.zeros(9)]), 3), to_mp(dM)
    assert check_min_eig(-2.0, dMm, 1e-12, B=Mm) == (True, True) and check_min_eig(-1.0, dMm, 1e-12, B=Mm) == (False, True)

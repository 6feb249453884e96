"""Reference and cases for the step-length eigenvalue tests (test_step_eig_cpu.py, test_step_eig_gpu.py).

The reference is an inertia count.  By Sylvester's law the number of negative pivots of the unpivoted L D L^T of A - s B (B positive definite) is the
number of eigenvalues of the pencil (A, B) below s -- for B = M = L L^T these are the eigenvalues of L^-1 A L^-T, the matrix whose smallest
eigenvalue the step length needs (src/solver.jl:1620-1693).  So a claimed smallest eigenvalue `got` is right to within `tol` exactly when nothing
lies below got - tol and something lies below got + tol: two eliminations in mpmath on the exact values of the inputs, and no Cholesky
factorisation, triangular solve or eigenvalue solver on the reference's side."""
import numpy as np

BITS = 400


class ZeroPivot(ArithmeticError):
    pass


def _mp():
    import mpmath
    return mpmath


def to_mp(A):
    """fp64 (n, n) array -> rows of mpf, exactly (under the 400-bit context every double converts without rounding)."""
    mp = _mp()
    with mp.workprec(BITS):
        return [[mp.mpf(float(v)) for v in row] for row in np.asarray(A, dtype=np.float64)]


def limbs_to_mp(a, n):
    """planar limbs (K, n * n), column-major -> rows of mpf: the exact sums of the limbs."""
    mp = _mp()
    a = np.atleast_2d(a)
    with mp.workprec(BITS):
        return [[mp.fsum(mp.mpf(float(a[l, i + j * n])) for l in range(a.shape[0])) for j in range(n)] for i in range(n)]


def count_below(A, s, B=None):
    """Number of negative pivots of the unpivoted L D L^T of A - s B (B = identity when None) at 400 bits.  A, B: fp64 arrays (taken exactly) or
    rows of mpf; only the lower triangles are read.  Raises ZeroPivot when a pivot vanishes (s is an eigenvalue of a leading section)."""
    mp = _mp()
    if isinstance(A, np.ndarray):
        A = to_mp(A)
    if isinstance(B, np.ndarray):
        B = to_mp(B)
    n = len(A)
    with mp.workprec(BITS):
        s = mp.mpf(s)
        if B is None:
            T = [[A[i][j] - (s if i == j else 0) for j in range(i + 1)] for i in range(n)]
        else:
            T = [[A[i][j] - s * B[i][j] for j in range(i + 1)] for i in range(n)]
        # the elimination on mpmath's raw numbers (libmp: the same arithmetic at the same 400 bits without a Python object per operation, three times faster)
        from mpmath.libmp import fzero, mpf_div, mpf_mul, mpf_sub
        T = [[v._mpf_ for v in row] for row in T]
        neg = 0
        for k in range(n):
            d = T[k][k]
            if d == fzero:
                raise ZeroPivot(k)
            if d[0]:                                            # sign bit
                neg += 1
            col = [T[i][k] for i in range(k + 1, n)]
            for ii, i in enumerate(range(k + 1, n)):
                if col[ii] == fzero:
                    continue
                f = mpf_div(col[ii], d, BITS, "n")
                Ti = T[i]
                for jj in range(ii + 1):
                    if col[jj] != fzero:
                        Ti[k + 1 + jj] = mpf_sub(Ti[k + 1 + jj], mpf_mul(f, col[jj], BITS, "n"), BITS, "n")
        return neg


def _count_nudged(A, s, B, direction):
    """count_below, moving s by one part in 2^60 in `direction` (away from the claimed value: the check only gets looser by that much) on a zero pivot."""
    mp = _mp()
    with mp.workprec(BITS):
        s = mp.mpf(s)
        for _ in range(8):
            try:
                return count_below(A, s, B)
            except ZeroPivot:
                step = mp.ldexp(abs(s), -60) if s != 0 else mp.ldexp(mp.mpf(1), -1000)
                s = s + direction * step
    raise ZeroPivot("eight nudges")


def check_min_eig(got, A, tol, B=None):
    """(nothing below got - tol, something below got + tol) -- the two halves of `assert_min_eig`."""
    mp = _mp()
    with mp.workprec(BITS):
        g, t = mp.mpf(float(got)), mp.mpf(float(tol))
        return _count_nudged(A, g - t, B, -1) == 0, _count_nudged(A, g + t, B, +1) >= 1


def assert_min_eig(got, A, tol, B=None, what=""):
    lo_ok, hi_ok = check_min_eig(got, A, tol, B)
    assert lo_ok, f"{what}: an eigenvalue lies below {got!r} - {tol:.3e}: the value is too LARGE (not the smallest eigenvalue)"
    assert hi_ok, f"{what}: no eigenvalue lies below {got!r} + {tol:.3e}: the value is too small"


def assert_min_eig_all(gots, A, tol, B=None, what=""):
    """assert_min_eig for several claimed values of the same matrix with ONE pair of counts: the counts are monotone in the shift, so nothing below
    max(gots) - tol and something below min(gots) + tol is the same statement as the check of every value on its own."""
    gots = [float(g) for g in gots]
    assert all(np.isfinite(gots)), f"{what}: {gots}"
    mp = _mp()
    with mp.workprec(BITS):
        t = mp.mpf(float(tol))
        lo_ok = _count_nudged(A, mp.mpf(max(gots)) - t, B, -1) == 0
        hi_ok = _count_nudged(A, mp.mpf(min(gots)) + t, B, +1) >= 1
    assert lo_ok, f"{what}: an eigenvalue lies below max{gots} - {tol:.3e}: a value is too LARGE (not the smallest eigenvalue)"
    assert hi_ok, f"{what}: no eigenvalue lies below min{gots} + {tol:.3e}: a value is too small"


def eig_tol(n, A):
    """n 2^-47 ||A||_2 = 64 n eps ||A||: a ceiling from the backward error of Householder tridiagonalisation (a modest multiple of n eps ||A||) plus a
    multisection carried to 257^-7 of the Gershgorin interval (a few eps ||A||) -- not a fit to any routine."""
    return n * 2.0 ** -47 * float(np.linalg.norm(np.asarray(A, dtype=np.float64), 2))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _sym(A):
    return np.tril(A) + np.tril(A, -1).T


def _with_spectrum(lam, rng):
    n = len(lam)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return _sym((Q * np.asarray(lam, dtype=np.float64)) @ Q.T)


def wilkinson(n):
    return np.diag(np.abs((n - 1) / 2.0 - np.arange(n))) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)


# the order is the order of preference where only the first few cases of a size are run (n > 33: the reference dominates the test's time)
CASE_NAMES = ("pair", "wilkinson_neg", "random", "tridiag_121", "cluster_1e-15", "rank_one", "graded", "corner", "wilkinson", "c_identity", "diag_two_values",
              "posdef", "negdef", "scaled_2^200", "scaled_2^-200", "zero")


def cases_budget(n):
    """how many cases of CASE_NAMES a test of side n runs: all of them up to 33 rows, then what keeps the two eliminations per case within seconds"""
    return len(CASE_NAMES) if n <= 33 else 8 if n < 64 else 6 if n == 64 else 4 if n <= 80 else 2


def eig_cases(n, seed=0, limit=None):
    """[(name, A)]: symmetric fp64 n x n matrices (exactly symmetric) on which smallest-eigenvalue routines go wrong.  Spectra are imposed through a random
    orthogonal Q in fp64 (the eigenvalues of the rounded matrix differ from the imposed ones by rounding: the reference looks at the matrix itself)."""
    rng = np.random.default_rng(1000 * n + seed)
    G = rng.standard_normal((n, n))
    R = _sym(G + G.T)
    out = {}
    if n == 1:
        out = {"random": R, "c_identity": np.array([[-0.375]]), "posdef": np.abs(R) + 1.0, "negdef": -np.abs(R) - 1.0,
               "scaled_2^200": np.ldexp(R, 200), "scaled_2^-200": np.ldexp(R, -200), "zero": np.zeros((1, 1))}
    else:
        out["pair"] = _with_spectrum(np.concatenate([[-1.0, -1.0 + 1e-13], np.linspace(0.5, 3.0, n - 2)]), rng)      # the two smallest 1e-13 apart
        out["wilkinson_neg"] = -wilkinson(n)                                                                         # close pairs at the BOTTOM
        out["random"] = R
        out["tridiag_121"] = 2.0 * np.eye(n) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)              # tridiagonal already: zero Householder vectors
        out["cluster_1e-15"] = _with_spectrum(-1.0 + 1e-15 * np.arange(n), rng)
        out["rank_one"] = -np.ones((n, n))
        out["graded"] = _with_spectrum(10.0 ** np.linspace(-12, 4, n), rng)
        C = np.zeros((n, n))
        C[0, n - 1] = C[n - 1, 0] = 1.0
        out["corner"] = C
        out["wilkinson"] = wilkinson(n)                                                                              # close pairs at the TOP
        out["c_identity"] = -0.375 * np.eye(n)
        out["diag_two_values"] = np.diag(np.where(np.arange(n) % 3 == 1, -1.25, 2.5))
        out["posdef"] = _sym(G @ G.T / n + np.eye(n))
        out["negdef"] = -_sym(G.T @ G / n + 0.5 * np.eye(n))
        out["scaled_2^200"] = np.ldexp(R, 200)
        out["scaled_2^-200"] = np.ldexp(R, -200)
        out["zero"] = np.zeros((n, n))
    names = [k for k in CASE_NAMES if k in out]
    if limit is not None:
        names = names[:limit]
    res = [(k, np.ascontiguousarray(out[k])) for k in names]
    for k, A in res:
        assert A.shape == (n, n) and np.array_equal(A, A.T), k
    return res


def planted_second_smallest(n=12, seed=5):
    """(A, lambda_1, lambda_2): a spectrum with a clear gap above its smallest eigenvalue -- lambda_2 is the wrong answer a routine that loses the smallest gives."""
    rng = np.random.default_rng(seed)
    lam = np.concatenate([[-2.0, -1.0], np.linspace(0.5, 3.0, n - 2)])
    A = _with_spectrum(lam, rng)
    w = np.linalg.eigvalsh(A)
    return A, float(w[0]), float(w[1])


# ---- congruence pairs: M = L L^T, dM = L W0 L^T, exact to the last limb ---------------------------------------------------------------------
CONGRUENCE_KINDS = ("random", "pair", "rank_one", "wilkinson_neg", "c_identity")


def _ints_of(a):
    """fp64 array -> (object array of Python ints, shift): a = ints / 2^shift exactly."""
    a = np.asarray(a, dtype=np.float64)
    nz = a[a != 0]
    shift = 0 if nz.size == 0 else 52 - int(np.min(np.frexp(nz)[1])) + 1
    return np.vectorize(lambda v: int(np.ldexp(v, shift)), otypes=[object])(a), shift


def _limbs_of_ratio(num, shift, K):
    """the integer num / 2^shift as K limbs by successive roundings to nearest (int / int is correctly rounded; every remainder is exact)."""
    from fractions import Fraction
    out = np.zeros(K)
    den = 1 << shift
    for l in range(K):
        if num == 0:
            break
        h = num / den
        out[l] = h
        num -= int(Fraction(h) * den)
    return out


def congruence_pair(n, K, kind, seed=0, diag_bits=16):
    """(M, dM, W0, L): M = L L^T and dM = L W0 L^T as planar limbs (K, n * n), products formed in integers and rounded once to K limbs, with L = (I + a
    strictly lower triangle of multiples of 2^-10, magnitudes up to 1 / (2 sqrt n)) D, D = powers of two from 1 down to 2^-diag_bits, so that cond(M) is
    4^diag_bits times that of the unit triangle; W0 (fp64, n x n) the case `kind` of eig_cases.  The eigenvalues of the pencil (dM, M) are those of W0 up
    to the last limb."""
    rng = np.random.default_rng(7919 * n + 31 * seed + K)
    W0 = dict(eig_cases(n, seed=seed))[kind]
    Ls = np.round(np.tril(rng.uniform(-1, 1, (n, n)), -1) * 1024 / (2 * np.sqrt(n))) / 1024
    ex = rng.integers(0, diag_bits + 1, n)
    ex[rng.integers(0, n)] = 0
    ex[(np.argmin(ex) + 1 + rng.integers(0, n - 1)) % n] = diag_bits
    L = (Ls + np.eye(n)) * np.ldexp(1.0, -ex)[None, :]             # columns scaled by powers of two (exact): no diagonal scaling of M undoes this
    Li, sl = _ints_of(L)
    Wi, sw = _ints_of(W0)
    Mi = Li.dot(Li.T)
    dMi = Li.dot(Wi).dot(Li.T)
    M, dM = np.zeros((K, n * n)), np.zeros((K, n * n))
    for j in range(n):
        for i in range(j, n):
            M[:, i + j * n] = M[:, j + i * n] = _limbs_of_ratio(Mi[i, j], 2 * sl, K)
            dM[:, i + j * n] = dM[:, j + i * n] = _limbs_of_ratio(dMi[i, j], 2 * sl + sw, K)
    return M, dM, W0, L


def easy_pair(n, K, seed=0):
    """(M, dM, W0) with M = diag(powers of two) and dM = M diag(w): the eigenvalues of the pencil are the w, the eliminations of the reference cost O(n)."""
    rng = np.random.default_rng(104729 * n + seed)
    d = np.ldexp(1.0, rng.integers(-2, 3, n))
    w = rng.uniform(-1.5, 2.0, n)
    M, dM = np.zeros((K, n * n)), np.zeros((K, n * n))
    M[0] = np.diag(d).reshape(-1)
    dM[0] = np.diag(d * w).reshape(-1)
    return M, dM, np.diag(w)


def scalar_pair(K, seed=0):
    """1 x 1 blocks: (M, dM, dM / M as an mpf) with M > 0, both carrying K limbs."""
    mp = _mp()
    rng = np.random.default_rng(15485863 + seed)
    vals = []
    for lo, hi in ((0.5, 2.0), (-3.0, 3.0)):
        v = np.zeros((K, 1))
        v[0, 0] = rng.uniform(lo, hi)
        for l in range(1, K):
            v[l, 0] = 0.49 * np.spacing(abs(v[l - 1, 0])) * rng.uniform(-1, 1)
        vals.append(v)
    with mp.workprec(BITS):
        ratio = limbs_to_mp(vals[1], 1)[0][0] / limbs_to_mp(vals[0], 1)[0][0]
    return vals[0], vals[1], ratio

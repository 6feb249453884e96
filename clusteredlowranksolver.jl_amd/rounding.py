"""Step 1 of the reference's `exact_solution` (src/rounding.jl:1366): "Finding the kernel" (RoundingSettings, src/rounding.jl:4-10;
detecteigenvectors, src/rounding.jl:575-642) at the working precision, on the device (clrs_mw_kernel_vectors).

At an optimum X_b Y_b = 0 for every PSD block: the row space of the dual block X_b is the kernel of the primal block Y_b.  The reference takes the
reduced row-echelon form of a column-pivoted QR of X_b; for a symmetric PSD block that form is [I W] over the pivots of the diagonally pivoted
elimination the preprocessing already uses (`mw.rank_reveal`).  Where the reference takes an SVD of Y_b instead (kernel_use_dual = false, or X_b too
large to be trusted), Y_b itself is eliminated and the relations of its dependent columns are the kernel: the same subspace, in echelon form over
other pivot columns.

With `rationalize=True` the entries of the vectors are also rounded to the field QQ on the device (src/rounding.jl:623-628: roundx -> clindep per entry;
here the first continued-fraction convergent p / q with |q v - p| < kernel_round_errbound, clrs_mw_rationalize) and the rounded
vectors are tested against the primal block again (src/rounding.jl:630-639).  Everything after that (number fields of degree > 1, LLL, the basis
transformations, the exact solve) is exact arithmetic and stays with the caller.

The next fixed-width step of the pipeline is the first work of `project_to_affine_space` (src/rounding.jl:182-211): "Finding the pivots of A using RREF mod p"
(`find_pivots_modular`, src/rounding.jl:288-333), a reduced row-echelon form of the integer system [A b] over the integers mod a prime of about 10^4.  It runs
on the device (clrs_modp_rref): `rref_mod_p`, `find_pivots_modular`, `system_pivots`.
"""
from __future__ import annotations

import dataclasses
from fractions import Fraction
from typing import List, Optional

import numpy as np

from . import _lib

__all__ = ["RoundingSettings", "KernelVectorError", "BlockKernel", "kernel_vectors", "kernel_vectors_batch", "kernel_vectors_rational_batch", "rationalize",
           "vectors_to_mp", "vectors_to_fractions", "rref_mod_p", "next_prime", "find_pivots_modular", "system_pivots", "PivotList"]

WRONG_VECTOR_MESSAGE = "wrong vector detected"
CLINDEP_MESSAGE = "clindep failed to find a relation"          # src/rounding.jl:508
LIMBS = (4, 5, 6, 8, 10)


@dataclasses.dataclass
class RoundingSettings:
    """The kernel fields of the reference's RoundingSettings (src/rounding.jl:4-10, 60-62) with its defaults."""
    kernel_errbound: float = 1e-10          # pivots / residuals below this are zero
    kernel_round_errbound: float = 1e-15    # the dual block is used while max |X_b| <= 1 / sqrt(this)
    kernel_use_dual: bool = True


class KernelVectorError(ValueError):
    """A kernel vector failed the reference's checks (src/rounding.jl:608, 620, 636)."""


@dataclasses.dataclass
class BlockKernel:
    """The kernel vectors of one block.  `branch`: "dual" (X_b eliminated) or "primal" (Y_b eliminated); `rank`: of the eliminated matrix; `count`: vectors
    (dual: rank, primal: n - rank); `perm`: pivots in pivot order, then the rest; `vectors`: planar (limbs, n, count), one vector per column, original
    index order; `resid_max` / `v_max`: per vector max_i |head (Y_b v)_i| and max_i |head v_i|; `pivot_resid`: planar (limbs, n - rank), the remaining
    diagonal of the eliminated matrix.  After `kernel_vectors(rationalize=True)` also `num`, `den` (n, count): the entries rounded to num / den, exact
    integers in fp64, den >= 1; `round_status` (n, count): 0 found, 1 no relation below 2^53, 2 not finite; `vectors_rounded`: num / den as planes
    (limbs, n, count); `round_resid_max`: per vector max_i |head (Y_b vq)_i|."""
    branch: str
    rank: int
    count: int
    perm: np.ndarray
    vectors: np.ndarray
    resid_max: np.ndarray
    v_max: np.ndarray
    pivot_resid: np.ndarray
    num: Optional[np.ndarray] = None
    den: Optional[np.ndarray] = None
    round_status: Optional[np.ndarray] = None
    vectors_rounded: Optional[np.ndarray] = None
    round_resid_max: Optional[np.ndarray] = None

    @property
    def max_num(self) -> int:
        """the largest |numerator| of the rounded vectors (what basis_transformations prints, src/rounding.jl:799-801)"""
        return int(np.max(np.abs(self.num))) if self.num is not None and self.num.size else 0

    @property
    def max_den(self) -> int:
        """the largest denominator of the rounded vectors"""
        return int(np.max(self.den)) if self.den is not None and self.den.size else 0


def kernel_vectors_batch(block_n, X, Y, limbs: int, tau: float, use_dual: bool, dual_max: float, device: int = 0, V=None, round_errbound: Optional[float] = None,
                         rounded=None):
    """One call of clrs_mw_kernel_vectors: X, Y planar (limbs, sum n_b^2) in the xy layout.  Returns a list of `BlockKernel`.  `V` (planar, the same shape)
    is the pool the vectors are written into; what the vectors do not cover stays as passed in (V is modified in place).
    `round_errbound`: call clrs_mw_kernel_vectors_rational instead, which also rounds the entries (the further fields of `BlockKernel`); `rounded`: the pools
    (num (plane,), den (plane,), status (plane,) int32, Vq (limbs, plane)) it writes into, like `V`."""
    n = np.ascontiguousarray(block_n, np.int32).reshape(-1)
    nb = n.size
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)])
    xoff = np.concatenate([[0], np.cumsum(n.astype(np.int64))])
    limbs, plane, xlen = int(limbs), int(off[-1]), int(xoff[-1])
    X, Y = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (X, Y))
    if X.shape != (limbs, plane) or Y.shape != (limbs, plane):
        raise ValueError(f"kernel_vectors_batch: X and Y must be planar ({limbs}, {plane}), got {X.shape} and {Y.shape}")
    if V is None:
        V = np.zeros((limbs, plane))
    if V.shape != (limbs, plane) or V.dtype != np.float64 or not V.flags.c_contiguous:
        raise ValueError(f"kernel_vectors_batch: V must be a contiguous float64 array of shape ({limbs}, {plane})")
    pad = lambda a: a if a.size else np.zeros((limbs, 1))           # (a valid pointer for an empty pool)
    branch, rank, count = (np.zeros(max(nb, 1), np.int32) for _ in range(3))
    perm = np.zeros(max(xlen, 1), np.int32)
    rmax, vmax, piv = np.zeros(max(xlen, 1)), np.zeros(max(xlen, 1)), np.zeros((limbs, max(xlen, 1)))
    Xp, Yp, Vp = pad(X), pad(Y), pad(V)
    p_i = lambda a: a.ctypes.data_as(_lib.p_i32)
    p_d = lambda a: a.ctypes.data_as(_lib.p_d)
    if round_errbound is None:
        _lib.check(_lib.load().clrs_mw_kernel_vectors(int(device), limbs, nb, p_i(n), p_d(Xp), p_d(Yp), plane, float(tau), int(bool(use_dual)), float(dual_max),
                                                      p_i(branch), p_i(perm), p_i(rank), p_i(count), p_d(Vp), p_d(rmax), p_d(vmax), p_d(piv)))
    else:
        num, den, status, Vq = (np.zeros(plane), np.zeros(plane), np.zeros(plane, np.int32), np.zeros((limbs, plane))) if rounded is None else rounded
        for a, shape, dtype in ((num, (plane,), np.float64), (den, (plane,), np.float64), (status, (plane,), np.int32), (Vq, (limbs, plane), np.float64)):
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError(f"kernel_vectors_batch: the pools of the rounded vectors must be contiguous, num, den, status ({plane},) and Vq ({limbs}, {plane})")
        rmax2 = np.zeros(max(xlen, 1))
        pad1 = lambda a: a if a.size else np.zeros(1, a.dtype)
        _lib.check(_lib.load().clrs_mw_kernel_vectors_rational(int(device), limbs, nb, p_i(n), p_d(Xp), p_d(Yp), plane, float(tau), int(bool(use_dual)),
                                                               float(dual_max), float(round_errbound), p_i(branch), p_i(perm), p_i(rank), p_i(count), p_d(Vp),
                                                               p_d(rmax), p_d(vmax), p_d(piv), p_d(pad1(num)), p_d(pad1(den)), p_i(pad1(status)), p_d(pad(Vq)),
                                                               p_d(rmax2)))
    out = []
    cols = lambda a, b, nn, c: np.ascontiguousarray(np.transpose(a[..., off[b]:off[b] + nn * c].reshape(a.shape[:-1] + (c, nn)), (0, 2, 1) if a.ndim == 2 else (1, 0)))
    for b in range(nb):
        nn, r, c = int(n[b]), int(rank[b]), int(count[b])
        vec = np.ascontiguousarray(np.transpose(V[:, off[b]:off[b] + nn * c].reshape(limbs, c, nn), (0, 2, 1)))
        out.append(BlockKernel("dual" if branch[b] else "primal", r, c, perm[xoff[b]:xoff[b + 1]].copy(), vec, rmax[xoff[b]:xoff[b] + c].copy(),
                               vmax[xoff[b]:xoff[b] + c].copy(), piv[:, xoff[b]:xoff[b] + nn - r].copy()))
        if round_errbound is not None:
            k = out[-1]
            k.num, k.den, k.round_status, k.vectors_rounded = cols(num, b, nn, c), cols(den, b, nn, c), cols(status, b, nn, c), cols(Vq, b, nn, c)
            k.round_resid_max = rmax2[xoff[b]:xoff[b] + c].copy()
    return out


def kernel_vectors_rational_batch(block_n, X, Y, limbs: int, tau: float, use_dual: bool, dual_max: float, round_errbound: float, device: int = 0, V=None,
                                  rounded=None):
    """One call of clrs_mw_kernel_vectors_rational: `kernel_vectors_batch` plus, on the device, the rounding of every entry of every vector to the first
    convergent p / q with |q v - p| < round_errbound and the residual of the rounded vectors."""
    return kernel_vectors_batch(block_n, X, Y, limbs, tau, use_dual, dual_max, device=device, V=V, round_errbound=float(round_errbound), rounded=rounded)


def rationalize(values, limbs: int, errbound: float = 1e-15, device: int = 0):
    """Round numbers to rationals on the device (clrs_mw_rationalize): `values` planar (planes <= limbs, count) or fp64 (count,).  Per number the first
    continued-fraction convergent p / q of |v| with |q |v| - p| < errbound, the sign restored.  Returns (num, den, status, vq): num, den (count,) exact
    integers in fp64, status (count,) int32 (0 found; 1 no convergent with p, q < 2^53 within 96 steps; 2 not finite; num = den = 0 for 1 and 2), vq planar
    (limbs, count) = num / den."""
    limbs = int(limbs)
    if limbs not in LIMBS:
        raise ValueError(f"rationalize: limbs must be one of {LIMBS}, got {limbs}")
    a = np.asarray(values, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] > limbs:
        raise ValueError(f"rationalize: values must be fp64 (count,) or planar (planes <= {limbs}, count), got {a.shape}")
    count = a.shape[1]
    v = np.zeros((limbs, max(count, 1)))
    v[:a.shape[0], :count] = a
    num, den, status, vq = np.zeros(max(count, 1)), np.zeros(max(count, 1)), np.zeros(max(count, 1), np.int32), np.zeros((limbs, max(count, 1)))
    _lib.check(_lib.load().clrs_mw_rationalize(int(device), limbs, count, v.ctypes.data_as(_lib.p_d), v.shape[1], float(errbound), num.ctypes.data_as(_lib.p_d),
                                               den.ctypes.data_as(_lib.p_d), status.ctypes.data_as(_lib.p_i32), vq.ctypes.data_as(_lib.p_d)))
    return num[:count], den[:count], status[:count], vq[:, :count]


def _planes(a, limbs, length, what):
    """fp64 (length,) or planar (planes, length) -> planar (limbs, length), zero padded or cut, as the warm start of solvesdp_mw does"""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[1] != length:
        raise ValueError(f"kernel_vectors: {what} must hold {length} numbers per limb plane, got {a.shape}")
    out = np.zeros((limbs, length))
    out[:min(limbs, a.shape[0])] = a[:limbs]
    return out


def kernel_vectors(sdp_or_block_n, dualsol, primalsol=None, limbs: Optional[int] = None, settings: Optional[RoundingSettings] = None, device: int = 0,
                   check_dimensions: bool = False, batch=None, rationalize: bool = False, round_batch=None) -> List[BlockKernel]:
    """The kernel vectors of every PSD block of a solution: `dualsol.X` are the dual blocks, `primalsol.Y` the primal blocks (a `SolveResult` of
    `solvesdp_mw`, or anything with those attributes, fp64 or planar limbs; `primalsol=None`: both from `dualsol`).  `sdp_or_block_n`: the problem (a
    `ClusteredLowRankSDP` or `FlatSDP`) or the block sizes in block order.  `limbs`: 4, 5, 6, 8 or 10 (default: the planes of the solution, 5 for fp64).
    Raises `KernelVectorError` ("wrong vector detected") when max |Y_b v| of some vector is not below `settings.kernel_errbound`
    (src/rounding.jl:608, 631-638) and, with `check_dimensions`, when the rank found on X_b plus the rank found on Y_b is not n_b (src/rounding.jl:611-621;
    a second elimination, of the matrix the first did not take).  `batch`: the device call (default `kernel_vectors_batch`).
    `rationalize`: also round every entry to the rationals with `settings.kernel_round_errbound` (the same device call: `round_batch`, default
    `kernel_vectors_rational_batch`) and fill `num`, `den`, `round_status`, `vectors_rounded`, `round_resid_max` of every block.  Raises `KernelVectorError`
    "clindep failed to find a relation" (src/rounding.jl:508) where an entry has no relation, and "wrong vector detected" where max |Y_b vq| of a rounded
    vector is above `kernel_errbound` (src/rounding.jl:630-639)."""
    settings = RoundingSettings() if settings is None else settings
    batch = kernel_vectors_batch if batch is None else batch
    round_batch = kernel_vectors_rational_batch if round_batch is None else round_batch
    if hasattr(sdp_or_block_n, "block_n"):
        block_n = sdp_or_block_n.block_n
    elif hasattr(sdp_or_block_n, "blocks"):
        from .sdp import flatten
        block_n = flatten(sdp_or_block_n).block_n
    else:
        block_n = sdp_or_block_n
    block_n = np.ascontiguousarray(block_n, np.int32).reshape(-1)
    primalsol = dualsol if primalsol is None else primalsol
    if limbs is None:
        planes = max(np.asarray(a).shape[0] if np.asarray(a).ndim == 2 else 1 for a in (dualsol.X, primalsol.Y))
        limbs = 5 if planes == 1 else planes
    limbs = int(limbs)
    if limbs not in LIMBS:
        raise ValueError(f"kernel_vectors: limbs must be one of {LIMBS}, got {limbs}")
    if not settings.kernel_errbound > 0 or not settings.kernel_round_errbound > 0:
        raise ValueError("kernel_vectors: kernel_errbound and kernel_round_errbound must be positive")
    off = np.concatenate([[0], np.cumsum(block_n.astype(np.int64) ** 2)])
    X, Y = _planes(dualsol.X, limbs, int(off[-1]), "X"), _planes(primalsol.Y, limbs, int(off[-1]), "Y")
    tau, dual_max = float(settings.kernel_errbound), 1.0 / float(np.sqrt(settings.kernel_round_errbound))
    if rationalize:
        out = round_batch(block_n, X, Y, limbs, tau, bool(settings.kernel_use_dual), dual_max, float(settings.kernel_round_errbound), device=device)
    else:
        out = batch(block_n, X, Y, limbs, tau, bool(settings.kernel_use_dual), dual_max, device=device)
    for b, k in enumerate(out):
        bad = [v for v in range(k.count) if not k.resid_max[v] < tau]
        if bad:
            raise KernelVectorError(f"{WRONG_VECTOR_MESSAGE}: block {b}, vector {bad[0]} ({k.branch} branch): max |Y v| = {float(k.resid_max[bad[0]]):.3e} "
                                    f"is not below kernel_errbound = {tau:.3e} (max |v| = {float(k.v_max[bad[0]]):.3e})")
    for b, k in enumerate(out if rationalize else ()):
        failed = np.argwhere(np.asarray(k.round_status).T != 0)                  # (vector, entry), the first vector first
        if failed.size:
            v, i = (int(t) for t in failed[0])
            raise KernelVectorError(f"{CLINDEP_MESSAGE}: block {b}, vector {v}, entry {i} (status {int(k.round_status[i, v])})")
        bad = [v for v in range(k.count) if k.round_resid_max[v] > tau]
        if bad:
            raise KernelVectorError(f"{WRONG_VECTOR_MESSAGE}: block {b}, rounded vector {bad[0]} ({k.branch} branch): max |Y vq| = "
                                    f"{float(k.round_resid_max[bad[0]]):.3e} is above kernel_errbound = {tau:.3e}")
    if check_dimensions:
        other = Y.copy()                                     # the matrix the first elimination did not take: Y_b after the dual branch, X_b after the primal
        for b, k in enumerate(out):
            if k.branch == "primal":
                other[:, off[b]:off[b + 1]] = X[:, off[b]:off[b + 1]]
        second = batch(block_n, other, other, limbs, tau, False, dual_max, device=device)
        for b, (k, k2) in enumerate(zip(out, second)):
            if k.rank + k2.rank != int(block_n[b]):
                rx, ry = (k.rank, k2.rank) if k.branch == "dual" else (k2.rank, k.rank)
                raise KernelVectorError(f"{WRONG_VECTOR_MESSAGE}: block {b}: rank {rx} found on X plus rank {ry} found on Y is not n = {int(block_n[b])}")
    return out


def vectors_to_mp(block: BlockKernel):
    """The vectors of a block as lists of mpmath numbers (the exact sums of the limbs), one list per vector."""
    from .mw import from_limbs
    v = np.asarray(block.vectors)
    return [list(from_limbs(v[:, :, c])) for c in range(v.shape[2])]


def vectors_to_fractions(block: BlockKernel):
    """The rounded vectors of a block (after `kernel_vectors(rationalize=True)`) as lists of `fractions.Fraction`, one list per vector."""
    if block.num is None:
        raise ValueError("vectors_to_fractions: the block was not rounded (kernel_vectors(..., rationalize=True))")
    if np.any(np.asarray(block.round_status) != 0):
        raise KernelVectorError(f"{CLINDEP_MESSAGE}: the block has entries without a relation")
    return [[Fraction(int(block.num[i, c]), int(block.den[i, c])) for i in range(block.num.shape[0])] for c in range(block.num.shape[1])]


# ---- pivots of integer systems: RREF mod p (src/rounding.jl:182-211, 288-333; clrs_modp_rref) -------------------------------------------
MODP_PRIME_LIMIT = 1 << 23          # clrs_modp_rref takes primes 2 <= p < 2^23
C_NULL_I32 = _lib.p_i32()


def _is_prime(n: int) -> bool:
    if n < 2:
        return False
    d = 2
    while d * d <= n:
        if n % d == 0:
            return False
        d += 1
    return True


def next_prime(x) -> int:
    """The smallest prime strictly above `x` (Nemo's next_prime, as src/rounding.jl:293 calls it)."""
    n = max(int(x) + 1, 2)
    while not _is_prime(n):
        n += 1
    return n


def _integer_matrix(A, what):
    """anything np.asarray takes -> a 2-d array of a numpy integer type, or of Python integers (dtype object) where those do not fit; an empty input
    becomes 0 x 0"""
    a = np.asarray(A)
    if a.size == 0:
        return np.zeros((a.shape[0], a.shape[1]) if a.ndim == 2 else (0, 0), dtype=np.int64)
    if a.ndim != 2:
        raise ValueError(f"{what}: the matrix must be two-dimensional, got shape {a.shape}")
    if a.dtype.kind in "iu":
        return a
    if a.dtype != object:
        raise ValueError(f"{what}: the entries must be integers, got dtype {a.dtype}")
    for v in a.flat:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: the entries must be integers, got {type(v).__name__}")
    return a


def _max_abs(a) -> int:
    """max |a| as a Python integer"""
    return max(abs(int(a.max())), abs(int(a.min())))


def _residues(a, p):
    """the matrix `a` reduced mod p on the host, int32 in [0, p)"""
    if a.size == 0:
        return np.zeros(a.shape, np.int32)
    if a.dtype != object and a.dtype != np.uint64:
        return np.ascontiguousarray(np.mod(a.astype(np.int64, copy=False), np.int64(p)), dtype=np.int32)
    return np.ascontiguousarray(np.array([int(v) % p for v in a.flat], dtype=np.int64).reshape(a.shape), dtype=np.int32)


def rref_mod_p(A, p: int, device: int = 0, want_rref: bool = False):
    """The reduced row-echelon form of `A` over the integers mod the prime `p` (2 <= p < 2^23) on the device: one call of clrs_modp_rref.  `A`: anything
    `np.asarray` takes, Python integers of any size included; it is reduced mod `p` on the host.  Returns `(pivots, rank)`, `pivots` the 0-based pivot
    columns in ascending order (int32, `rank` of them), or with `want_rref` `(pivots, rank, R)`, `R` (nrows, ncols) int32 with residues in [0, p), the
    pivot rows first and the rows behind them zero."""
    a = _integer_matrix(A, "rref_mod_p")
    p = int(p)
    if p < 2 or p >= MODP_PRIME_LIMIT or not _is_prime(p):
        raise ValueError(f"rref_mod_p: p must be a prime with 2 <= p < 2^23, got {p}")
    nrows, ncols = a.shape
    res = _residues(a, p)
    pivots = np.full(max(min(nrows, ncols), 1), -1, np.int32)
    rank = np.zeros(1, np.int32)
    R = np.zeros((nrows, ncols), np.int32) if want_rref else None
    null = C_NULL_I32
    _lib.check(_lib.load().clrs_modp_rref(int(device), nrows, ncols, p, res.ctypes.data_as(_lib.p_i32) if res.size else null, pivots.ctypes.data_as(_lib.p_i32),
                                          rank.ctypes.data_as(_lib.p_i32), R.ctypes.data_as(_lib.p_i32) if want_rref and R.size else null))
    r = int(rank[0])
    return (pivots[:r].copy(), r, R) if want_rref else (pivots[:r].copy(), r)


class PivotList(list):
    """The 0-based pivot columns `find_pivots_modular` returns: a list of ints with two attributes, `primes` (the primes tried, in order) and `p` (the
    prime whose pivots these are)."""
    primes: List[int]
    p: Optional[int]

    def __init__(self, pivots=(), primes=(), p=None):
        super().__init__(int(c) for c in pivots)
        self.primes = [int(q) for q in primes]
        self.p = None if p is None else int(p)


def find_pivots_modular(A, maxprimes: int = 3, device: int = 0, batch=None) -> PivotList:
    """The reference's `find_pivots_modular(A; maxprimes)` (src/rounding.jl:288-311) with its schedule of primes: p = min(max |A|, 10^4), and per round
    p <- next_prime(p) and the pivot columns of the reduced row-echelon form of A mod p.  The first list with as many pivots as A has rows is returned; after
    `maxprimes` rounds the first of the longest lists seen.  Returns a `PivotList`: the 0-based pivot columns (the reference's are 1-based), with the
    primes tried in `.primes`.  An empty matrix gives `[]` with no prime tried (the reference raises on it); `maxprimes < 1` raises
    `ValueError` (the reference returns `nothing`).  `batch(A, p, device=...)` -> `(pivots, rank)`
    replaces the device call (default `rref_mod_p`)."""
    batch = rref_mod_p if batch is None else batch
    a = _integer_matrix(A, "find_pivots_modular")
    if int(maxprimes) < 1:
        raise ValueError(f"find_pivots_modular: maxprimes must be at least 1, got {maxprimes}")
    if a.size == 0:
        return PivotList()
    nrows = a.shape[0]
    p = min(_max_abs(a), 10 ** 4)
    history, primes = [], []
    for _ in range(int(maxprimes)):
        p = next_prime(p)
        primes.append(p)
        pivots, _ = batch(a, p, device=device)[:2]
        pivots = [int(c) for c in pivots]
        if len(pivots) == nrows:
            return PivotList(pivots, primes, p)
        history.append((pivots, p))
    best = max(len(h[0]) for h in history)
    pivots, p = next(h for h in history if len(h[0]) == best)
    return PivotList(pivots, primes, p)


def _rows_cleared_of_denominators(rows):
    """rows of Fractions -> an object matrix of Python integers, every row multiplied by the least common multiple of its denominators"""
    from math import gcd
    out = np.zeros((len(rows), len(rows[0]) if rows else 0), dtype=object)
    for r, row in enumerate(rows):
        lcm = 1
        for v in row:
            lcm = lcm * v.denominator // gcd(lcm, v.denominator)
        out[r] = [int(v * lcm) for v in row]
    return out


def system_pivots(A, b, maxprimes: int = 3, device: int = 0, batch=None):
    """The pivot part of the reference's `project_to_affine_space` (src/rounding.jl:184-211) for the system A x = b, `A` (nrows, ncols) and `b` (nrows,) or
    (nrows, 1) of `Fraction`s or integers.  Every row of [A b] is cleared of denominators (multiplied by the least common multiple of its denominators, b
    included: preprocess_rows!(include_b = true); the rows of A alone likewise for the second call), `pivots = find_pivots_modular([A b])`; the system is
    inconsistent when the last pivot is the column of b (an empty pivot list counts as consistent); when there are fewer pivots than rows,
    `rows = find_pivots_modular(transpose(A[:, pivots]))`, a set of independent rows, otherwise all rows.  Returns `(pivots, rows, consistent)`, 0-based
    `PivotList`s (`rows` of an inconsistent system is every row)."""
    A = np.asarray(A, dtype=object)
    if A.ndim != 2:
        raise ValueError(f"system_pivots: A must be two-dimensional, got shape {A.shape}")
    nrows, ncols = A.shape
    b = np.asarray(b, dtype=object).reshape(-1)
    if b.size != nrows:
        raise ValueError(f"system_pivots: b must have one entry per row of A, got {b.size} for {nrows} rows")
    rows_of_A = [[Fraction(v) for v in A[r]] for r in range(nrows)]
    Ab = _rows_cleared_of_denominators([rows_of_A[r] + [Fraction(b[r])] for r in range(nrows)]) if nrows else np.zeros((0, ncols + 1), dtype=object)
    pivots = find_pivots_modular(Ab, maxprimes=maxprimes, device=device, batch=batch)
    every_row = PivotList(range(nrows))
    if len(pivots) and pivots[-1] == ncols:
        return pivots, every_row, False
    if len(pivots) == nrows:
        return pivots, every_row, True
    Ai = _rows_cleared_of_denominators(rows_of_A)                  # (the reference's A at that point: rows cleared of the denominators of A alone)
    rows = find_pivots_modular(Ai[:, list(pivots)].T, maxprimes=maxprimes, device=device, batch=batch)
    return pivots, rows, True

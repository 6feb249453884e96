"""Step 1 of the reference's `exact_solution` (src/rounding.jl:1366): "Finding the kernel" (RoundingSettings, src/rounding.jl:4-10;
detecteigenvectors, src/rounding.jl:575-642) at the working precision, on the device (clrs_mw_kernel_vectors).

At an optimum X_b Y_b = 0 for every PSD block: the row space of the dual block X_b is the kernel of the primal block Y_b.  The reference takes the
reduced row-echelon form of a column-pivoted QR of X_b; for a symmetric PSD block that form is [I W] over the pivots of the diagonally pivoted
elimination the preprocessing already uses (`mw.rank_reveal`).  Where the reference takes an SVD of Y_b instead (kernel_use_dual = false, or X_b too
large to be trusted), Y_b itself is eliminated and the relations of its dependent columns are the kernel: the same subspace, in echelon form over
other pivot columns.

With `rationalize=True` the entries of the vectors are also rounded to the field QQ on the device (src/rounding.jl:623-628: roundx -> clindep per entry;
here the first continued-fraction convergent p / q with |q v - p| < kernel_round_errbound, clrs_mw_rationalize) and the rounded
vectors are tested against the primal block again (src/rounding.jl:630-639).  Number fields of degree > 1 and the LLL / HNF reduction of the vectors stay
with the caller; the basis transformations and the exact solve are described below.

The next fixed-width step of the pipeline is the first work of `project_to_affine_space` (src/rounding.jl:182-211): "Finding the pivots of A using RREF mod p"
(`find_pivots_modular`, src/rounding.jl:288-333), a reduced row-echelon form of the integer system [A b] over the integers mod a prime of about 10^4.  It runs
on the device (clrs_modp_rref): `rref_mod_p`, `find_pivots_modular`, `system_pivots`.

The rest of `project_to_affine_space` (src/rounding.jl:213-286, 336-364) is the exact solve of the integer system, the reference's `Nemo._solve_dixon`: Dixon's
p-adic lifting, on the device (clrs_modp_dixon_lift): `dixon_lift`, `solve_dixon`, `solve_system_pseudoinverse`,
`project_to_affine_space`.  The rational reconstruction and the products around the solve are exact host arithmetic in Python integers, unless
`reconstruct=dixon_reconstruct` (section 16) and `matmul=zz_matmul` (the exact integer matrix product clrs_zz_gemm, section 18) move them to the device.

The last numeric step of the chain is `is_valid_solution` (src/rounding.jl:367-415): zero slacks, and every block of the exact solution positive definite
(`checkpd_cholesky`, src/rounding.jl:447-472, Arb's ball-arithmetic Cholesky).  Here the answer is exact: the leading principal minors of the block, cleared of
denominators, mod many primes on the device (clrs_modp_minors), lifted to integers on the host: `leading_minors_mod`, `minor_bounds`,
`crt_tree`, `checkpd`, `is_valid_solution`.  Blocks of at most 128 rows.

Between the kernel vectors and the projection stands `basis_transformations` (src/rounding.jl:750-858): per PSD block `B = [kernel vectors | completing standard
basis vectors]`, `Binv = inv(B)` over QQ, its rows normalised by the lcm of their denominators, and `transform` / `undo_transform` (src/rounding.jl:1191-1253),
which multiply with it.  The inverse is an exact solve with a matrix of right-hand sides: Dixon's lifting with both products of a step as fp64 MFMA GEMMs on
the device (clrs_modp_dixon_lift_multi): `dixon_lift_multi`, `solve_dixon_multi`, `inverse_qq`, `complete_basis`,
`basis_transformations`, `transform`, `undo_transform`.

The reference's reduced branch (`simplify_kernelvectors`, `reduction_step`, `basis_nullspace_remaining`, src/rounding.jl:860-1104: an LLL-reduced Z-basis of the
saturated lattice of the kernel vectors and a unimodular basis change) is an LLL reduction of one embedded lattice per block, a batch on the device
(clrs_zz_lll): `lll_batch`, `lll`, `reduce_kernel_vectors`, and `basis_transformations(..., reduce=reduce_kernel_vectors)`.  It is
taken only when `reduce=` is given: without it the default settings still raise `NotImplementedError`.  Not built: the reference's `kernel_lll` and its
partial-column heuristic above `reduce_kernelvectors_cutoff`.

Over a number field QQ(g) of degree 2 .. 4 the entries of the kernel vectors are rounded by integer relations on the device (src/rounding.jl:481-534: roundx(x, g, deg)
-> clindep -> lindep; clrs_mw_field_round): `NumberField`, `round_to_field`, `field_relations_lll` (the same contract through clrs_zz_lll: the
rescue, degrees 5 .. 8), `kernel_vectors(..., rationalize=True, field=...)`, `vectors_to_field`.  Of the steps after the rounding the positive-definiteness check is built
(`checkpd_field`, exact: the leading minors as elements of Z[g] from their images at the roots of the minimal polynomial mod primes that split it,
clrs_modp_minors_field; `split_primes`, `field_frobenius`, `leading_minors_field_mod`, `field_minor_bounds`, `FieldPDCertificate`,
`is_valid_solution(..., field=...)`), and so is the basis change (`B = [V | E]` and its inverse over QQ(g), src/rounding.jl:834-836, 1017-1050: the determinant and
the adjugate as elements of Z[g] from the inverses of the residue matrices at every (split prime, root) pair, clrs_modp_field_adjugate, DESIGN.md section 25;
`inverse_field`, `FieldInverse`, `field_adjugate_mod`, `field_adjugate_bounds`, `field_matmul`, `complete_basis_field`, `transform_field`, `undo_transform_field`,
`basis_transformations(..., field=...)`).  The system over the field is built too: an `ExactProblem` may carry a `field` and coefficient tuples
(`field_array`; `to_sdp` embeds them at g; `problems.delsarte_exact_problem(..., field=)`), `linear_system(field=)` assembles it with one `assemble` call per
low-rank block on the coefficient planes stacked along the terms, `convert_system` / `xrational_to_field` (src/rounding.jl:1256-1282, 1332-1342) turn it into a
system over QQ and back, `field_least_squares` is the reference's roundx(A, b, x, g, deg) (src/rounding.jl:537-568: regularised normal equations of condition
number about 1e30, their products by clrs_mw_gemm and their solve by clrs_mw_posv, a blocked multi-word Cholesky on the device, `mw.posv`, DESIGN.md section
26), `get_rational_system(field=)` and `exact_solution(field=)` run the chain.  The reduction of the field's kernel vectors is not built: the field branch
needs `RoundingSettings(reduce_kernelvectors=False)`.

The field itself is found from the solution (src/find_field.jl): `select_vals` picks one generic entry per kernel vector, `minimal_polynomials` searches an
integer relation among the powers of each, degree by degree, on the device (clrs_mw_minpoly; `minpoly_relations_lll` is the same contract
through clrs_zz_lll), `find_common_minpoly` joins the generators into one `NumberField`, `find_field` runs the three, and `to_field` writes a number in the field.

The system the projection solves is assembled from an `ExactProblem` (the problem over QQ; `to_sdp` gives the numeric one) by `linear_system`
(`partial_linearsystem`, src/interface.jl:1354-1535): per low-rank block one call of clrs_zz_lowrank_system, a row-wise Gram of long
integers with the digit index in the k-extent of the fp64 MFMA: `lowrank_system`, `system_index`, `select_columns` (src/rounding.jl:95-153),
`get_rational_system` (src/rounding.jl:1284-1296).  `exact_solution` (src/rounding.jl:1366-1409) calls the steps in order.
"""
from __future__ import annotations

import dataclasses
from fractions import Fraction
from typing import List, Optional

import numpy as np

from . import _lib

__all__ = ["RoundingSettings", "KernelVectorError", "BlockKernel", "kernel_vectors", "kernel_vectors_batch", "kernel_vectors_rational_batch", "rationalize",
           "vectors_to_mp", "vectors_to_fractions", "rref_mod_p", "next_prime", "find_pivots_modular", "system_pivots", "PivotList", "to_balanced_digits", "from_balanced_digits",
           "prev_prime", "dixon_steps", "dixon_lift", "rational_reconstruction", "SingularSystemError", "DixonSolution", "solve_dixon",
           "solve_system_pseudoinverse", "project_to_affine_space", "to_digits24", "from_digits24", "dixon_reconstruct", "leading_minors_mod", "minor_bounds", "crt_tree",
           "PDCertificate", "checkpd", "is_valid_solution", "ints_to_planes", "planes_to_ints", "zz_matmul", "dixon_lift_multi", "DixonSolutionMatrix",
           "solve_dixon_multi", "inverse_qq", "complete_basis", "basis_transformations", "transform", "undo_transform", "lowrank_system", "ExactLowRank", "ExactBlock",
           "ExactProblem", "ExactSolution", "system_index", "linear_system", "select_columns", "vectorize_solution", "get_rational_system", "exact_solution",
           "ReductionError", "lll_first_rung", "lll_batch", "lll", "kernel_lattice", "reduce_kernel_vectors", "NumberField", "FieldRounding", "round_to_field",
           "field_relations_lll", "kernel_vectors_field_batch", "vectors_to_field", "split_primes", "field_frobenius", "leading_minors_field_mod", "field_minor_bounds",
           "FieldPDCertificate", "checkpd_field", "convert_system", "xrational_to_field", "field_least_squares", "field_array", "MinPolySearch",
           "minimal_polynomials", "minpoly_relations_lll", "select_vals", "find_common_minpoly", "find_field", "to_field"]

WRONG_VECTOR_MESSAGE = "wrong vector detected"
CLINDEP_MESSAGE = "clindep failed to find a relation"          # src/rounding.jl:508
LIMBS = (4, 5, 6, 8, 10)


@dataclasses.dataclass
class RoundingSettings:
    """The kernel, pseudoinverse and basis-change fields of the reference's RoundingSettings (src/rounding.jl:4-10, 23-25, 57-62) with its defaults."""
    kernel_errbound: float = 1e-10          # pivots / residuals below this are zero
    kernel_round_errbound: float = 1e-15    # the dual block is used while max |X_b| <= 1 / sqrt(this)
    kernel_use_dual: bool = True
    kernel_bits: int = 1000                 # the relation of an entry with the powers of the field's generator is searched up to this many bits (src/rounding.jl:7); not read over QQ
    pseudo: bool = True                     # solve through the pseudoinverse of a few more columns than rows (src/rounding.jl:23, 213)
    pseudo_columnfactor: float = 1.05       # that many columns per row; at least 1 (src/rounding.jl:60-62)
    extracolumns_linindep: bool = False     # take the extra columns linearly independent of each other instead of at random
    reduce_kernelvectors: bool = True       # LLL reduction of the kernel vectors (src/rounding.jl:860-1060): basis_transformations takes it with `reduce=`, and refuses it without
    unimodular_transform: bool = True       # with the reduction: the whole basis change unimodular (src/rounding.jl:960-963); False: only the kernel vectors are replaced
    normalize_transformation: bool = True   # rows of Binv times the lcm of their denominators, columns of B divided by it (src/rounding.jl:844-850)
    regularization: float = 1e-30           # of the least-squares problem of roundx(A, b, x, g, deg) over a number field (src/rounding.jl:537)
    approximation_decimals: int = 40        # the numeric solution is cut to this many decimals before the projection (roundx, src/rounding.jl:515)
    redundancyfactor: int = 10              # select_columns takes about this many columns per constraint; negative: all (src/rounding.jl:95-153)

    def __post_init__(self):
        if self.pseudo_columnfactor < 1:
            self.pseudo_columnfactor = 1


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
    coeffs: Optional[np.ndarray] = None          # with `field=` of degree deg >= 2: (n, count, deg) `Fraction`s, entry = sum_k coeffs[.., k] g^k (num / den stay None)
    round_rung: Optional[np.ndarray] = None      # with `field=`: (n, count), the bits of the rung an entry was accepted at

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
                   check_dimensions: bool = False, batch=None, rationalize: bool = False, round_batch=None, field=None) -> List[BlockKernel]:
    """The kernel vectors of every PSD block of a solution: `dualsol.X` are the dual blocks, `primalsol.Y` the primal blocks (a `SolveResult` of
    `solvesdp_mw`, or anything with those attributes, fp64 or planar limbs; `primalsol=None`: both from `dualsol`).  `sdp_or_block_n`: the problem (a
    `ClusteredLowRankSDP` or `FlatSDP`) or the block sizes in block order.  `limbs`: 4, 5, 6, 8 or 10 (default: the planes of the solution, 5 for fp64).
    Raises `KernelVectorError` ("wrong vector detected") when max |Y_b v| of some vector is not below `settings.kernel_errbound`
    (src/rounding.jl:608, 631-638) and, with `check_dimensions`, when the rank found on X_b plus the rank found on Y_b is not n_b (src/rounding.jl:611-621;
    a second elimination, of the matrix the first did not take).  `batch`: the device call (default `kernel_vectors_batch`).
    `rationalize`: also round every entry to the rationals with `settings.kernel_round_errbound` (the same device call: `round_batch`, default
    `kernel_vectors_rational_batch`) and fill `num`, `den`, `round_status`, `vectors_rounded`, `round_resid_max` of every block.  Raises `KernelVectorError`
    "clindep failed to find a relation" (src/rounding.jl:508) where an entry has no relation, and "wrong vector detected" where max |Y_b vq| of a rounded
    vector is above `kernel_errbound` (src/rounding.jl:630-639).
    `field`: a `NumberField`; of degree >= 2 (with `rationalize`) every entry is rounded to it by an integer relation searched up to `settings.kernel_bits`
    bits (`round_batch`, default `kernel_vectors_field_batch`): `coeffs`, `round_status`, `round_rung`, `vectors_rounded`,
    `round_resid_max` are filled, `num` / `den` stay None, and the same two errors are raised.  None, or degree 1: the path over QQ, untouched."""
    settings = RoundingSettings() if settings is None else settings
    batch = kernel_vectors_batch if batch is None else batch
    over_field = field is not None and field.degree >= 2
    round_batch = (kernel_vectors_field_batch if over_field else kernel_vectors_rational_batch) if round_batch is None else round_batch
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
    if rationalize and over_field:
        out = round_batch(block_n, X, Y, limbs, tau, bool(settings.kernel_use_dual), dual_max, float(settings.kernel_round_errbound), field=field,
                          bits=int(settings.kernel_bits), device=device)
    elif rationalize:
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


def _check_modp_prime(what: str, p: int) -> None:
    if p < 2 or p >= MODP_PRIME_LIMIT or not _is_prime(p):
        raise ValueError(f"{what}: p must be a prime with 2 <= p < 2^23, got {p}")


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
    _check_modp_prime("rref_mod_p", p)
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


# ---- the exact solve: Dixon's p-adic lifting (src/rounding.jl:213-286, 336-364; clrs_modp_dixon_lift) -------------------------------------
DIGIT_BITS = 24                      # integers cross the C boundary in balanced base-2^24 digits, every digit in [-2^23, 2^23)
DIXON_FIRST_PRIME = 8388593          # the largest prime below 2^23: the fewest steps
LIFT_MAX_N = 32767


def _digits24_from_bytes(raw, rows: int, count: int) -> np.ndarray:
    """`rows * count` little-endian digits of three bytes each (bytes, as `int.to_bytes` makes them) -> uint32 (rows, count)"""
    wide = np.zeros((rows, count, 4), np.uint8)
    wide[:, :, :3] = np.frombuffer(raw, dtype=np.uint8).reshape(rows, count, 3)
    return wide.view("<u4").reshape(rows, count)


def _digits24_to_bytes(digits) -> np.ndarray:
    """digits in [0, 2^24), uint32 (rows, count) -> uint8 (rows, 3 count): the three low bytes of every digit, what `int.from_bytes` takes row by row"""
    d = np.ascontiguousarray(digits, dtype="<u4")
    return np.ascontiguousarray(d.view(np.uint8).reshape(d.shape[0], d.shape[1], 4)[:, :, :3]).reshape(d.shape[0], 3 * d.shape[1])


def _balanced_offset(count: int) -> int:
    """H = sum_{l < count} 2^23 2^(24 l): v + H has the digits of v, each raised by 2^23, as its digits in [0, 2^24)"""
    return (1 << (DIGIT_BITS - 1)) * (((1 << (DIGIT_BITS * count)) - 1) // ((1 << DIGIT_BITS) - 1))


def _balanced_need(v: int) -> int:
    """the number of balanced digits the Python integer v needs (at least one): the smallest c with 0 <= v + H_c < 2^(24 c)"""
    c = max(abs(v).bit_length() // DIGIT_BITS, 1)                                 # c digits hold magnitudes below 2^(24 c) only: never too many, at most two too few
    while not 0 <= v + _balanced_offset(c) < 1 << (DIGIT_BITS * c):
        c += 1
    return c


def _ints_to_planes(name: str, values, count: Optional[int]) -> np.ndarray:
    """`to_balanced_digits` and `ints_to_planes` (`name`, for the messages): linear in the digits of every entry.  Values below 2^62 in magnitude are cut by
    numpy on int64; for larger ones, with `H = sum_l 2^23 2^(24 l)`, the bytes of `v + H` (`int.to_bytes`) are cut into 24-bit digits and 2^23 is taken off
    each."""
    a = np.asarray(values)
    if a.dtype != object and a.dtype.kind not in "iu":
        if a.size:
            raise ValueError(f"{name}: the values must be integers, got dtype {a.dtype}")
        a = a.astype(np.int64)
    if count is not None and int(count) < 1:
        raise ValueError(f"{name}: count must be at least 1, got {count}")
    misfit = f"{name}: a value does not fit in {count} balanced digits of {DIGIT_BITS} bits"
    half, base = 1 << (DIGIT_BITS - 1), 1 << DIGIT_BITS
    if a.dtype == object:
        flat = [int(v) for v in a.flat]
        if all(-(1 << 62) < v < 1 << 62 for v in flat):
            a = np.array(flat, dtype=np.int64).reshape(a.shape)
    if a.dtype != object and (a.size == 0 or _max_abs(a) < 1 << 62):
        v, planes = a.astype(np.int64), []
        while True:
            d = ((v + half) & (base - 1)) - half
            planes.append(np.asarray(d, dtype=np.int64).astype(np.int32))
            v = (v - d) >> DIGIT_BITS
            done = not np.any(v != 0)
            if done if count is None else len(planes) == int(count):
                break
        if not done:
            raise ValueError(misfit)
        return np.ascontiguousarray(np.stack(planes))
    flat = [int(v) for v in a.flat]
    if count is None:
        top = max(abs(v).bit_length() for v in flat)
        count = max(_balanced_need(v) for v in flat if abs(v).bit_length() + 2 * DIGIT_BITS >= top)     # (only the longest values can decide the count)
    count = int(count)
    H, nbytes = _balanced_offset(count), 3 * count
    try:
        raw = b"".join((v + H).to_bytes(nbytes, "little") for v in flat)
    except OverflowError:                                           # v + H negative or 2^(24 count) and beyond
        raise ValueError(misfit) from None
    digits = _digits24_from_bytes(raw, len(flat), count).astype(np.int32) - np.int32(half)
    return np.ascontiguousarray(digits.T).reshape((count,) + a.shape)


def to_balanced_digits(values, count: Optional[int] = None) -> np.ndarray:
    """Python integers of any size (anything `np.asarray` takes, any shape) -> balanced base-2^24 digits, little-endian: int32 (count, *shape), every
    digit `d = ((v + 2^23) mod 2^24) - 2^23`, then `v <- (v - d) / 2^24`.  `count=None`: as many digits as the largest value needs (at least one);
    otherwise `ValueError` when a value does not fit.  Linear in the digits of every entry."""
    return _ints_to_planes("to_balanced_digits", values, count)


def ints_to_planes(values, count: Optional[int] = None) -> np.ndarray:
    """`to_balanced_digits` under the name the product functions use (its own name in the messages)."""
    return _ints_to_planes("ints_to_planes", values, count)


def from_balanced_digits(planes) -> np.ndarray:
    """Digit planes (count, *shape) -> the integers `sum_l planes[l] 2^(24 l)` as Python integers (an object array of shape `shape`).  Integer digits in
    [-2^23, 2^23) take the linear way: every digit raised by 2^23, its three low bytes packed, `int.from_bytes`, and `H` taken off.  Planes with other
    digits (2^23 itself, which clrs_zz_gemm accepts as input) go through a Horner loop."""
    planes = np.asarray(planes)
    count, shape = planes.shape[0], planes.shape[1:]
    half = 1 << (DIGIT_BITS - 1)
    if planes.dtype.kind not in "iu" or planes.size == 0 or not shape or int(planes.min()) < -half or int(planes.max()) >= half:
        out = np.zeros(shape, dtype=object)                        # (one integer, `shape` empty, leaves this loop as a Python integer, not an array)
        for l in range(count - 1, -1, -1):
            out = out * (1 << DIGIT_BITS) + planes[l].astype(object)
        return out
    packed = _digits24_to_bytes((planes.reshape(count, -1).astype(np.int64) + half).T)                                   # (entries, 3 count)
    H, step, raw = _balanced_offset(count), 3 * count, packed.tobytes()
    out = np.empty(shape, dtype=object)
    out.flat = [int.from_bytes(raw[i * step:(i + 1) * step], "little") - H for i in range(packed.shape[0])]
    return out


def planes_to_ints(planes) -> np.ndarray:
    """`from_balanced_digits` for the planes a device call returns: at least one plane of an integer dtype, `ValueError` otherwise."""
    planes = np.asarray(planes)
    if planes.ndim < 1 or planes.shape[0] < 1:
        raise ValueError(f"planes_to_ints: at least one plane is needed, got shape {planes.shape}")
    if planes.dtype.kind not in "iu":
        raise ValueError(f"planes_to_ints: the digits must be integers, got dtype {planes.dtype}")
    return np.asarray(from_balanced_digits(planes), dtype=object)


def prev_prime(x) -> int:
    """The largest prime strictly below `x` (`ValueError` for x <= 2)."""
    n = int(x) - 1
    while n >= 2 and not _is_prime(n):
        n -= 1
    if n < 2:
        raise ValueError(f"prev_prime: there is no prime below {x}")
    return n


def _isqrt(v: int) -> int:
    from math import isqrt
    return isqrt(v)


def _object_vector(values) -> np.ndarray:
    """a list -> a one-dimensional object array, whatever the entries are"""
    out = np.empty(len(values), dtype=object)
    out[:] = values
    return out


def _square_system(A, b, what):
    """(A, b) -> an object matrix (n, n) and an object vector (n,) of Python integers"""
    A = _integer_matrix(A, what)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{what}: A must be square, got {A.shape}")
    n = A.shape[0]
    bm = np.asarray(b)
    bv = _integer_matrix(bm.reshape(-1, 1), what).reshape(-1) if bm.size else np.zeros(0, dtype=np.int64)
    if bv.size != n:
        raise ValueError(f"{what}: b must have one entry per row of A, got {bv.size} for {n} rows")
    return (np.array([int(v) for v in A.flat], dtype=object).reshape(n, n) if n else np.zeros((0, 0), dtype=object),
            _object_vector([int(v) for v in bv.flat]))


def dixon_steps(A, b, p: int):
    """The number of lifting steps and the reconstruction bounds for the integer system A x = b at the prime p: `(K, N, D)` with
    `D2 = prod_c max(sum_r A[r, c]^2, 1)` (Hadamard), `N2 = D2 max(sum b^2, 1)` (Cramer), `N = isqrt(N2) + 1`, `D = isqrt(D2) + 1` -- every entry of the
    solution has |numerator| <= N and denominator <= D -- and K the smallest integer with `p^(2K) > 4 N2 D2`."""
    A, b = _square_system(A, b, "dixon_steps")
    p = int(p)
    if p < 2:
        raise ValueError(f"dixon_steps: p must be at least 2, got {p}")
    D2 = 1
    for c in range(A.shape[0]):
        D2 *= max(sum(int(v) * int(v) for v in A[:, c]), 1)
    N2 = D2 * max(sum(int(v) * int(v) for v in b), 1)
    bound = 4 * N2 * D2
    K = max(int((bound.bit_length() - 1) // (2 * p.bit_length())), 0)            # p^(2K) < 2^(2K bits(p)) <= bound: no larger than the answer
    q = p ** (2 * K)
    while q <= bound:
        q *= p * p
        K += 1
    return K, _isqrt(N2) + 1, _isqrt(D2) + 1


def _dixon_lift_digits(Ad, bl, p: int, steps: int, device: int = 0):
    """One call of clrs_modp_dixon_lift on digit planes: `Ad` int32 (nd, n, n), `bl` int32 (nbl, n).  Returns `(X, r_limbs, info)`: X int32 (steps, n),
    r_limbs int32 (nrl, n), info int32 (4,)."""
    Ad, bl = np.ascontiguousarray(Ad, dtype=np.int32), np.ascontiguousarray(bl, dtype=np.int32)
    nd, n, nbl, steps = Ad.shape[0], Ad.shape[1], bl.shape[0], int(steps)
    if Ad.ndim != 3 or Ad.shape[2] != n or bl.shape != (nbl, n):
        raise ValueError(f"dixon_lift: the digits of A must be (nd, n, n) and the limbs of b (nbl, n), got {Ad.shape} and {bl.shape}")
    nrl = max(nbl, nd + 1) + 1
    X = np.zeros((max(steps, 0), n), np.int32)
    r = np.zeros((nrl, n), np.int32)
    info = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.p_i32) if a.size else C_NULL_I32
    _lib.check(_lib.load().clrs_modp_dixon_lift(int(device), n, int(p), nd, ptr(Ad), nbl, ptr(bl), steps, ptr(X), ptr(r), ptr(info)))
    return X, r, info


def dixon_lift(A, b, p: int, steps: int, device: int = 0):
    """`steps` steps of Dixon's p-adic lifting of the integer system A x = b (A n x n, Python integers of any size) on the device: one call of
    clrs_modp_dixon_lift.  `C = A^-1 mod p`, `r_0 = b`, `x_k = C (r_k mod p) mod p`, `r_{k+1} = (r_k - A x_k) / p`.  Returns `(X, r, rank)`: X int32
    (steps, n) with the x_k, residues in [0, p); r (n,) the last residual as Python integers, so that `A sum_k X[k] p^k == b - p^steps r`; rank the rank of
    A mod p.  When rank < n nothing was lifted and X and r are None."""
    A, b = _square_system(A, b, "dixon_lift")
    n, p, steps = A.shape[0], int(p), int(steps)
    _check_modp_prime("dixon_lift", p)
    if n > LIFT_MAX_N or steps < 0:
        raise ValueError(f"dixon_lift: n must be at most {LIFT_MAX_N} and steps at least 0, got n = {n}, steps = {steps}")
    Ad = ints_to_planes(A) if n else np.zeros((1, 0, 0), np.int32)
    bl = ints_to_planes(b) if n else np.zeros((1, 0), np.int32)
    X, r, info = _dixon_lift_digits(Ad, bl, p, steps, device=device)
    rank = int(info[0])
    if rank < n:
        return None, None, rank
    return X, planes_to_ints(r), rank


def rational_reconstruction(a: int, m: int, N: int, D: int):
    """The rational num / den with num = a den (mod m), |num| <= N and 0 < den <= D, by the half-extended Euclidean algorithm on (m, a mod m) stopped at the
    first remainder <= N; `None` when that remainder's cofactor t does not satisfy 0 < |t| <= D or is not coprime to it.  Unique when m > 2 N D."""
    from math import gcd
    m, N, D = int(m), int(N), int(D)
    r0, r1, t0, t1 = m, int(a) % m, 0, 1
    while r1 > N:
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    if t1 == 0 or abs(t1) > D or gcd(r1, abs(t1)) != 1:
        return None
    return Fraction(r1, t1) if t1 > 0 else Fraction(-r1, -t1)


def to_digits24(value: int, count: Optional[int] = None) -> np.ndarray:
    """The Python integer `value >= 0` -> its little-endian digits in [0, 2^24) as int32: as many as it needs (at least one), or `count` (`ValueError`
    when it does not fit).  Linear in the digit count: `int.to_bytes`, then three bytes per digit."""
    value = int(value)
    if value < 0:
        raise ValueError("to_digits24: the value must not be negative")
    need = max((value.bit_length() + DIGIT_BITS - 1) // DIGIT_BITS, 1)
    count = need if count is None else int(count)
    if count < need:
        raise ValueError(f"to_digits24: the value does not fit in {count} digits of {DIGIT_BITS} bits")
    return np.ascontiguousarray(_digits24_from_bytes(value.to_bytes(3 * count, "little"), 1, count)[0].astype(np.int32))


def from_digits24(digits) -> list:
    """Rows of little-endian digits in [0, 2^24) (int32, shape (count,) or (rows, count)) -> the Python integer of every row (an integer for one row given
    as (count,), else a list).  Linear in the digit count: the three low bytes of every digit packed, then `int.from_bytes`."""
    d = np.ascontiguousarray(digits, dtype="<u4")
    if d.size and int(d.max()) >= 1 << DIGIT_BITS:
        raise ValueError("from_digits24: a digit outside [0, 2^24)")
    rows = d.reshape(-1, d.shape[-1]) if d.ndim > 1 else d.reshape(1, -1)
    packed = _digits24_to_bytes(rows)
    out = [int.from_bytes(packed[i].tobytes(), "little") for i in range(rows.shape[0])]
    return out if d.ndim > 1 else out[0]


def _coprime_fraction(num: int, den: int) -> Fraction:
    """`Fraction(num, den)` for coprime num and den > 0 without the gcd of the constructor: `Fraction._from_coprime_ints` where the running Python has it
    (3.12 and later), the constructor's `_normalize=False` before that."""
    make = getattr(Fraction, "_from_coprime_ints", None)
    return make(num, den) if make is not None else Fraction(num, den, _normalize=False)


def dixon_reconstruct(X, p: int, N: int, D: int, device: int = 0, want_x: bool = False):
    """The rational reconstruction of every entry of a lifted solution on the device, one call of clrs_modp_dixon_reconstruct: `X`
    int32 (steps, n) as `dixon_lift` returns it, `x_i = sum_k X[k, i] p^k`, and per entry the half-extended Euclidean algorithm on `(p^steps, x_i)`
    stopped at the first remainder <= N -- what `rational_reconstruction(x_i, p^steps, N, D)` computes, with the same result.  Returns a list of
    `Fraction | None`; with `want_x` also the list of the integers x_i: `(fractions, x)`.  The digits come back as int32 and become Python integers by
    `from_digits24` (linear).  Numerator and denominator arrive coprime (the device has tested it), so each `Fraction` is built without a second gcd:
    by `Fraction._from_coprime_ints` on Python 3.12 and later, by `Fraction(num, den, _normalize=False)` before that.  The counters of the call are kept in
    `dixon_reconstruct.last_info` (`[limbs of p^steps, most quotient steps of an entry, their total, 0]`)."""
    X = np.ascontiguousarray(X, dtype=np.int32)
    if X.ndim != 2:
        raise ValueError(f"dixon_reconstruct: X must be (steps, n), got shape {X.shape}")
    steps, n = X.shape
    p, N, D = int(p), int(N), int(D)
    _check_modp_prime("dixon_reconstruct", p)
    if steps < 1 or n > LIFT_MAX_N or N < 0 or D < 0:
        raise ValueError(f"dixon_reconstruct: steps must be at least 1, n at most {LIFT_MAX_N} and the bounds not negative")
    if n == 0:
        return ([], []) if want_x else []
    Nd, Dd = to_digits24(N), to_digits24(D)
    nl = max(Nd.size, Dd.size)
    nx = (steps * p.bit_length()) // DIGIT_BITS + 1              # p^steps < 2^(steps bits(p)): never fewer limbs than it has
    num, den = np.zeros((n, nl), np.int32), np.zeros((n, nl), np.int32)
    neg, status, info = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(4, np.int32)
    xl = np.zeros((n, nx), np.int32) if want_x else None
    ptr = lambda a: C_NULL_I32 if a is None else a.ctypes.data_as(_lib.p_i32)
    _lib.check(_lib.load().clrs_modp_dixon_reconstruct(int(device), n, p, steps, ptr(X), Nd.size, ptr(Nd), Dd.size, ptr(Dd), nl, ptr(num), ptr(den), ptr(neg),
                                                       ptr(status), nx, ptr(xl), ptr(info)))
    dixon_reconstruct.last_info = [int(v) for v in info]
    nums, dens = from_digits24(num), from_digits24(den)
    out = [None if status[i] else _coprime_fraction(-nums[i] if neg[i] else nums[i], dens[i]) for i in range(n)]
    return (out, from_digits24(xl)) if want_x else out


dixon_reconstruct.last_info = None


class SingularSystemError(ValueError):
    """The matrix of `solve_dixon` was singular mod every prime tried: it is singular, or `maxprimes` was too small (the reference: "The system is
    rank-deficient", src/rounding.jl:250)."""


class DixonSolution(list):
    """The solution `solve_dixon` returns: a list of `Fraction`s with three attributes, `p` (the prime lifted at), `primes` (the primes tried, in order)
    and `steps` (the lifting steps)."""
    p: Optional[int]
    primes: List[int]
    steps: int

    def __init__(self, values=(), p=None, primes=(), steps=0):
        super().__init__(values)
        self.p = None if p is None else int(p)
        self.primes = [int(q) for q in primes]
        self.steps = int(steps)


def _fraction_rows(A, b, what):
    """(A (nrows, ncols), b (nrows,) or (nrows, 1)) of integers or Fractions -> (rows of Fractions, list of Fractions, ncols)"""
    A = np.asarray(A, dtype=object)
    if A.size == 0:
        A = A.reshape((A.shape[0], A.shape[1]) if A.ndim == 2 else (0, 0))
    if A.ndim != 2:
        raise ValueError(f"{what}: A must be two-dimensional, got shape {A.shape}")
    b = np.asarray(b, dtype=object).reshape(-1)
    if b.size != A.shape[0]:
        raise ValueError(f"{what}: b must have one entry per row of A, got {b.size} for {A.shape[0]} rows")
    return [[Fraction(v) for v in A[r]] for r in range(A.shape[0])], [Fraction(v) for v in b], A.shape[1]


def solve_dixon(A, b, maxprimes: int = 3, device: int = 0, lift=None, check: bool = True, reconstruct=None, matmul=None) -> DixonSolution:
    """The exact solution of the square system A x = b (what the reference asks of `Nemo._solve_dixon`, src/rounding.jl:274, 351, 360): `A` (n, n) and `b`
    (n,) or (n, 1) of integers or `Fraction`s.  Every row of [A b] is cleared of denominators; the primes are tried downward from 8388593, the largest
    below 2^23 (the solution does not depend on the prime, and the largest needs the fewest steps), at most `maxprimes` of them, and the first at which A
    has rank n is lifted `K = dixon_steps(A, b, p)[0]` steps; every entry is then reconstructed from `sum_k x_k p^k mod p^K`.  Returns a
    `DixonSolution`.  Raises `SingularSystemError` when A is singular mod every prime tried, `ValueError` for `maxprimes < 1`, and, with `check`,
    `ArithmeticError` unless `A x == b - p^K r_K` holds for the lifted integers and `A solution == b` for the fractions.
    `lift(A, b, p, steps, device=...)` -> `(X, r, rank)` replaces the device call (default `dixon_lift`).
    `reconstruct(X, p, N, D, device=..., want_x=...)` -> the list of `Fraction | None` (with `want_x` also the integers `sum_k X[k] p^k`) replaces the
    Horner loop and the per-entry `rational_reconstruction` on the host; `dixon_reconstruct` does both on the device.  With `check` the identity of the
    lifted integers is then tested on the integers that `reconstruct` returned.
    `matmul(A, B, device=...)` -> the exact product of integer matrices (`zz_matmul` forms it on the device) replaces the host products of the two checks:
    `Ai x` of the lifted integers, and `A solution == b` as ONE integer product `Ai y == L bi` over the common denominator L of the solution (`y = L solution`;
    Ai, bi the rows cleared of denominators).  `None`: the host arithmetic."""
    lift = dixon_lift if lift is None else lift
    if int(maxprimes) < 1:
        raise ValueError(f"solve_dixon: maxprimes must be at least 1, got {maxprimes}")
    rows, bf, ncols = _fraction_rows(A, b, "solve_dixon")
    n = len(rows)
    if ncols != n:
        raise ValueError(f"solve_dixon: A must be square, got {n} x {ncols}")
    if n == 0:
        return DixonSolution()
    Ab = _rows_cleared_of_denominators([rows[r] + [bf[r]] for r in range(n)])
    Ai, bi = Ab[:, :n], Ab[:, n]
    p, primes = DIXON_FIRST_PRIME + 1, []
    for _ in range(int(maxprimes)):
        p = prev_prime(p)
        primes.append(p)
        K, N, D = dixon_steps(Ai, bi, p)
        X, r, rank = lift(Ai, bi, p, K, device=device)
        if rank == n:
            break
    else:
        raise SingularSystemError(f"solve_dixon: the matrix is singular mod every prime tried ({primes})")
    m = p ** K
    if reconstruct is None:
        x = np.zeros(n, dtype=object)
        for k in range(K - 1, -1, -1):                          # Horner: x = sum_k X[k] p^k
            x = x * p + np.asarray(X[k]).astype(object)
    elif check:
        sol, x = reconstruct(X, p, N, D, device=device, want_x=True)
        x = _object_vector([int(v) for v in x])
    else:
        sol, x = reconstruct(X, p, N, D, device=device, want_x=False), None
    if check and any(int(v) != int(w) for v, w in zip(Ai.dot(x) if matmul is None else _matmul_vector(matmul, Ai, x, device), bi - m * np.asarray(r, dtype=object))):
        raise ArithmeticError(f"solve_dixon: A x != b - p^K r after {K} steps at p = {p}")
    if reconstruct is None:
        sol = [rational_reconstruction(int(v), m, N, D) for v in x]
    if any(v is None for v in sol):
        raise ArithmeticError(f"solve_dixon: entry {[v is None for v in sol].index(True)} has no rational reconstruction within the bounds")
    if check and matmul is not None:
        yv, L = _common_denominator(sol)
        if any(v != L * int(w) for v, w in zip(_matmul_vector(matmul, Ai, yv, device), bi)):
            raise ArithmeticError("solve_dixon: A solution != b")
    elif check and any(sum(rows[i][j] * sol[j] for j in range(n)) != bf[i] for i in range(n)):
        raise ArithmeticError("solve_dixon: A solution != b")
    return DixonSolution(sol, p, primes, K)


def _gcd_of(values) -> int:
    from math import gcd
    g = 0
    for v in values:
        g = gcd(g, int(v))
    return g if g else 1                                        # (a zero row or column: the matrix is singular, the solve says so)


def solve_system_pseudoinverse(A, b, maxprimes: int = 3, device: int = 0, lift=None, check: bool = True, reconstruct=None, matmul=None):
    """The reference's `solve_system_pseudoinverse(A, b)` (src/rounding.jl:336-364): for `A` (nrows, ncols) with independent rows and more columns than rows
    the minimum-norm solution `v = A^T (A A^T)^-1 b` of A v = b; otherwise (independent columns) `v = (A^T A)^-1 A^T b`.  A and b are first multiplied by the least
    common multiple of the denominators of A so that the reference's gcds are gcds of integers; the Gram matrix is scaled on the right by `Dr = diag(1 / gcd(column))` and
    then on the left by `Dl = diag(1 / gcd(row))` as there, solved by `solve_dixon` (to which `maxprimes`, `device`, `lift`, `check`, `reconstruct`, `matmul`
    go), and `v = A^T (Dr y)` or `v = Dr y`.  All products are exact host arithmetic, unless `matmul(A, B, device=...)` is given (`zz_matmul`: on the device):
    then the Gram matrix is one integer product, and `A^T b` and the back-substitution `A^T (Dr y)` are one integer product each over the common denominator
    of the vector, divided by it entry by entry -- the same `Fraction`s.  Returns a list of `Fraction`s; `SingularSystemError` when the Gram matrix is
    singular."""
    from math import gcd
    rows, bf, ncols = _fraction_rows(A, b, "solve_system_pseudoinverse")
    nrows = len(rows)
    if nrows == 0 or ncols == 0:
        return [Fraction(0)] * ncols
    lcm = 1                                                     # one multiplier for the whole system: the least-squares solution is that of A, b
    for row in rows:
        for v in row:
            lcm = lcm * v.denominator // gcd(lcm, v.denominator)
    Ai = np.zeros((nrows, ncols), dtype=object)
    for r, row in enumerate(rows):
        Ai[r] = [int(v * lcm) for v in row]
        bf[r] = bf[r] * lcm
    bv = _object_vector(bf)
    wide = ncols > nrows
    if matmul is None:
        G = Ai.dot(Ai.T) if wide else Ai.T.dot(Ai)
        rhs = bv if wide else Ai.T.dot(bv)
    else:
        AiT = np.ascontiguousarray(Ai.T)
        G = np.array(matmul(Ai, AiT, device=device) if wide else matmul(AiT, Ai, device=device), dtype=object).reshape(min(nrows, ncols), min(nrows, ncols))
        rhs = bv
        if not wide:
            bint, Lb = _common_denominator(bf)
            rhs = _object_vector([Fraction(v, Lb) for v in _matmul_vector(matmul, AiT, bint, device)])
    k = G.shape[0]
    dr = [_gcd_of(G[:, c]) for c in range(k)]
    for c in range(k):
        G[:, c] = [int(v) // dr[c] for v in G[:, c]]
    dl = [_gcd_of(G[r]) for r in range(k)]
    for r in range(k):
        G[r] = [int(v) // dl[r] for v in G[r]]
    y = solve_dixon(G, [Fraction(rhs[r]) / dl[r] for r in range(k)], maxprimes=maxprimes, device=device, lift=lift, check=check,
                    reconstruct=reconstruct, matmul=matmul)
    y = [y[c] / dr[c] for c in range(k)]
    if not wide:
        return y
    if matmul is not None:
        yint, Ly = _common_denominator(y)
        return [Fraction(v, Ly) for v in _matmul_vector(matmul, AiT, yint, device)]
    return [sum((int(Ai[r, c]) * y[r] for r in range(nrows)), Fraction(0)) for c in range(ncols)]


def project_to_affine_space(A, b, settings: Optional[RoundingSettings] = None, rng=None, device: int = 0, batch=None, lift=None, reconstruct=None, matmul=None):
    """The reference's `project_to_affine_space(A, b; settings)` (src/rounding.jl:182-286): a solution of A x = b, `A` (nrows, ncols) and `b` (nrows,) or
    (nrows, 1) of `Fraction`s or integers.  Returns `(x, correct_slacks, finished)`, x a list of ncols `Fraction`s.

    `system_pivots` gives the pivot columns and independent rows; an inconsistent system returns the zero vector, False, False.  With `settings.pseudo`:
    the columns that are no pivots, shuffled by `rng` (a `numpy.random.Generator`, default `default_rng(0)`; the reference calls `shuffle`), are put behind
    the pivots -- or, with `extracolumns_linindep`, rounds of `find_pivots_modular` on the shuffled remaining columns until there are
    `pseudo_columnfactor * nrows` of them -- the list is cut at `round(pseudo_columnfactor * nrows)` columns, and those columns of the independent rows
    are solved by `solve_system_pseudoinverse`; `correct_slacks = (A x == b)`.  When that solve meets a singular matrix (`SingularSystemError`; the
    reference prints "The system is rank-deficient") or without `pseudo`: the pivot columns alone, by `solve_dixon` when they form a square system
    (`correct_slacks = True`), through the normal equations otherwise (`correct_slacks = (A_piv^T A_piv x == A_piv^T b)`).  Indices are 0-based.
    `batch` / `lift` replace the device calls of `find_pivots_modular` / `solve_dixon`; `reconstruct` goes to `solve_dixon` as it is.
    `matmul(A, B, device=...)` (`zz_matmul`: on the device) goes to `solve_system_pseudoinverse` and `solve_dixon` and replaces the `Fraction` loops here by
    integer products: `A x == b` over the common denominator of x on the rows of [A b] cleared of denominators; the normal equations as `M^T M` and `M^T c`
    for `[M c] = D [A_piv b]`, D the least common multiple of all denominators, divided by D^2; and their test as one more product.  The same results."""
    settings = RoundingSettings() if settings is None else settings
    rng = np.random.default_rng(0) if rng is None else rng
    rows_f, bf, ncols = _fraction_rows(A, b, "project_to_affine_space")
    nrows = len(rows_f)
    zero = [Fraction(0)] * ncols
    if nrows == 0 or ncols == 0:
        return zero, all(v == 0 for v in bf), True
    pivots, rows, consistent = system_pivots(rows_f, bf, device=device, batch=batch)
    if not consistent:
        return zero, False, False
    pivots, rows = [int(c) for c in pivots], [int(r) for r in rows]
    residual_free = lambda x: all(sum((rows_f[r][c] * x[c] for c in range(ncols) if x[c] != 0), Fraction(0)) == bf[r] for r in range(nrows))
    if matmul is not None:
        def residual_free(x):
            Ab = _rows_cleared_of_denominators([rows_f[r] + [bf[r]] for r in range(nrows)])
            yv, L = _common_denominator(x)
            return all(v == L * int(w) for v, w in zip(_matmul_vector(matmul, Ab[:, :ncols], yv, device), Ab[:, ncols]))
    if settings.pseudo:
        try:
            if settings.extracolumns_linindep:
                Ai = _rows_cleared_of_denominators(rows_f)
                extracolumns = []
                while sum(len(e) for e in extracolumns) + len(pivots) < settings.pseudo_columnfactor * nrows:
                    taken = set(pivots).union(*extracolumns)
                    nonpivots = [c for c in range(ncols) if c not in taken]
                    if not nonpivots:
                        break
                    nonpivots = [int(c) for c in rng.permutation(nonpivots)]
                    extra = find_pivots_modular(Ai[rows][:, nonpivots], device=device, batch=batch)
                    if not len(extra):
                        break                                   # (only zero columns are left; the reference would not end)
                    extracolumns.append([nonpivots[t] for t in extra])
            else:
                in_pivots = set(pivots)
                extracolumns = [[int(c) for c in rng.permutation([c for c in range(ncols) if c not in in_pivots])]]
            subset = list(dict.fromkeys(pivots + [c for e in extracolumns for c in e]))
            subset = subset[:min(len(subset), int(round(settings.pseudo_columnfactor * nrows)))]
            newx = solve_system_pseudoinverse([[rows_f[r][c] for c in subset] for r in rows], [bf[r] for r in rows], device=device,
                                              lift=lift, reconstruct=reconstruct, matmul=matmul)
            x = list(zero)
            for c, v in zip(subset, newx):
                x[c] = v
            return x, residual_free(x), True
        except SingularSystemError:
            pass                                                # the reference: "The system is rank-deficient"; the pivot system follows
    Apiv = [[rows_f[r][c] for c in pivots] for r in range(nrows)]
    nA, nb = Apiv, list(bf)
    square = nrows == len(pivots)
    Mi = None
    if not square and matmul is not None and pivots:            # the normal equations as integer products of [M c] = D [A_piv b]
        k = len(pivots)
        scaled, D = _common_denominator([v for r in range(nrows) for v in Apiv[r] + [bf[r]]])
        scaled = scaled.reshape(nrows, k + 1)
        Mi, ci = scaled[:, :k], scaled[:, k]
        MiT = np.ascontiguousarray(Mi.T)
        nAi = np.array(matmul(MiT, Mi, device=device), dtype=object).reshape(k, k)
        nbi = _matmul_vector(matmul, MiT, ci, device)
        nA = [[Fraction(int(nAi[i, j]), D * D) for j in range(k)] for i in range(k)]
        nb = [Fraction(v, D * D) for v in nbi]
    elif not square:                                            # the normal equations
        k = len(pivots)
        nb = [sum((Apiv[r][i] * bf[r] for r in range(nrows)), Fraction(0)) for i in range(k)]
        nA = [[sum((Apiv[r][i] * Apiv[r][j] for r in range(nrows)), Fraction(0)) for j in range(k)] for i in range(k)]
    newx = solve_dixon(nA, nb, device=device, lift=lift, reconstruct=reconstruct, matmul=matmul) if pivots else []
    if Mi is not None:
        yv, L = _common_denominator(newx)
        correct = all(v == L * w for v, w in zip(_matmul_vector(matmul, nAi, yv, device), nbi))
    else:
        correct = True if square else all(sum((nA[i][j] * newx[j] for j in range(len(pivots))), Fraction(0)) == nb[i] for i in range(len(pivots)))
    x = list(zero)
    for j, c in enumerate(pivots):
        x[c] = newx[j]
    return x, correct, True


# ---- the exact positive-definiteness check: leading minors mod many primes (src/rounding.jl:367-415, 447-472; clrs_modp_minors) ------------
MINORS_MAX_N = 128                   # clrs_modp_minors keeps the matrix of a prime in the LDS of one workgroup
MINORS_MAX_PRIMES = 65535            # primes of one call of clrs_modp_minors


def _primes_descending():
    """every prime below 2^23, descending (what repeated `prev_prime` from 2^23 gives), sieved once"""
    if _primes_descending.cache is None:
        sieve = np.ones(MODP_PRIME_LIMIT, dtype=bool)
        sieve[:2] = False
        for d in range(2, _isqrt(MODP_PRIME_LIMIT) + 1):
            if sieve[d]:
                sieve[d * d::d] = False
        _primes_descending.cache = np.flatnonzero(sieve)[::-1].astype(np.int64)
    return _primes_descending.cache


_primes_descending.cache = None


def _symmetric_integer_matrix(M, what):
    """-> an object matrix (n, n) of Python integers; `ValueError` unless square and symmetric"""
    a = _integer_matrix(M, what)
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"{what}: the matrix must be square, got {a.shape}")
    n = a.shape[0]
    out = np.array([int(v) for v in a.flat], dtype=object).reshape(n, n) if n else np.zeros((0, 0), dtype=object)
    if any(out[i, j] != out[j, i] for i in range(n) for j in range(i)):
        raise ValueError(f"{what}: the matrix must be symmetric")
    return out


def leading_minors_mod(M, primes, device: int = 0):
    """The leading principal minors of the symmetric integer matrix `M` (n <= 128, Python integers of any size) mod every prime of `primes` (distinct, in
    [2, 2^23), at most 65535) on the device: one call of clrs_modp_minors.  Returns `(minors, breakdown)`: minors int32 (len(primes), n), row q holding
    minor_1 .. minor_n mod primes[q]; breakdown int32 (len(primes),), 0 or the order k of the first minor that is 0 mod primes[q] -- row q then holds 0 at
    position k and -1 behind it (the elimination takes no exchanges, so nothing behind a zero pivot is defined).  The counters of the call are kept in
    `leading_minors_mod.last_info` (`[LDS bytes per workgroup, workgroups, primes that broke down, 0]`)."""
    a = _symmetric_integer_matrix(M, "leading_minors_mod")
    n = a.shape[0]
    pr = np.ascontiguousarray([int(p) for p in primes], dtype=np.int64)
    if n < 1 or n > MINORS_MAX_N:
        raise ValueError(f"leading_minors_mod: n must lie in [1, {MINORS_MAX_N}], got {n}")
    if pr.size < 1 or pr.size > MINORS_MAX_PRIMES or pr.min() < 2 or pr.max() >= MODP_PRIME_LIMIT:
        raise ValueError(f"leading_minors_mod: between 1 and {MINORS_MAX_PRIMES} primes in [2, 2^23) are needed")
    pr = pr.astype(np.int32)
    digits = to_balanced_digits(a)
    minors, breakdown, info = np.full((pr.size, n), -2, np.int32), np.full(pr.size, -2, np.int32), np.zeros(4, np.int32)
    ptr = lambda v: v.ctypes.data_as(_lib.p_i32)
    _lib.check(_lib.load().clrs_modp_minors(int(device), n, digits.shape[0], ptr(digits), pr.size, ptr(pr), ptr(minors), ptr(breakdown), ptr(info)))
    leading_minors_mod.last_info = [int(v) for v in info]
    return minors, breakdown


leading_minors_mod.last_info = None


def minor_bounds(M) -> list:
    """Python integers `H_k >= |minor_k|`, k = 1 .. n, for the symmetric integer matrix `M`: Hadamard's bound on the leading k x k part, the product of
    the Euclidean norms of its rows, every square root an integer square root rounded up."""
    a = _symmetric_integer_matrix(M, "minor_bounds")
    n = a.shape[0]
    sums, out = [0] * n, []
    for k in range(1, n + 1):
        for i in range(k - 1):
            sums[i] += a[i, k - 1] * a[i, k - 1]
        sums[k - 1] = sum(a[k - 1, j] * a[k - 1, j] for j in range(k))
        h = 1
        for i in range(k):
            r = _isqrt(sums[i])
            h *= r if r * r == sums[i] else r + 1
        out.append(h)
    return out


def crt_tree(residues, primes):
    """Balanced Chinese remaindering of many residue vectors over ONE product tree: `primes` m distinct primes, `residues` (m, count) (or (m,)): row q
    holds the residues mod primes[q].  Returns `(values, modulus)`: `modulus` the product P of the primes, `values` a list of `count` Python integers
    (one integer for (m,)), the representatives in (-P / 2, P / 2].

    The tree of products is built once.  The cofactors (P / p_q)^-1 mod p_q come from one remainder tree of P modulo the squares of the nodes
    ((P mod p^2) / p = (P / p) mod p); a vector is then combined upwards, `v_left P_right + v_right P_left` per node.  Every level costs a few
    multiplications of the total size, so the whole is quasi-linear in the bits of P (a Horner-style incremental CRT is quadratic)."""
    pr = [int(p) for p in primes]
    m = len(pr)
    res = np.asarray(residues)
    single = res.ndim == 1
    res = res.reshape(m, -1) if m else res.reshape(0, 0)
    if m < 1 or len(set(pr)) != m or min(pr) < 2:
        raise ValueError("crt_tree: at least one modulus, all distinct and at least 2")
    count = res.shape[1]
    levels = [pr]
    while len(levels[-1]) > 1:
        prev = levels[-1]
        levels.append([prev[i] * prev[i + 1] if i + 1 < len(prev) else prev[i] for i in range(0, len(prev), 2)])
    P = levels[-1][0]
    rem = [P]
    for lev in reversed(levels[:-1]):
        rem = [rem[i // 2] % (v * v) for i, v in enumerate(lev)]
    inv = [pow((rem[i] // pr[i]) % pr[i], -1, pr[i]) for i in range(m)]
    if max(pr) < MODP_PRIME_LIMIT:                                  # the leaves in int64: a residue times a cofactor is below 2^46
        leaves = np.mod(np.mod(res.astype(np.int64), np.array(pr, np.int64)[:, None]) * np.array(inv, np.int64)[:, None], np.array(pr, np.int64)[:, None]).astype(object)
    else:
        leaves = np.array([[(int(res[i, c]) % pr[i]) * inv[i] % pr[i] for c in range(count)] for i in range(m)], dtype=object).reshape(m, count)
    half = P // 2
    values = []
    for c in range(count):
        vals = [int(v) for v in leaves[:, c]]
        for lev in levels[:-1]:
            vals = [vals[i] * lev[i + 1] + vals[i + 1] * lev[i] if i + 1 < len(vals) else vals[i] for i in range(0, len(vals), 2)]
        x = vals[0] % P
        values.append(x - P if x > half else x)
    return (values[0] if single else values), P


@dataclasses.dataclass
class PDCertificate:
    """What `checkpd` proves about a symmetric rational matrix A.  `pd`: A is positive definite.  `scale`: the positive least common multiple D of the
    denominators; the minors are those of the integer matrix D A.  `minors`: the exact leading principal minors of D A as Python integers, from order 1 up
    to the order at which the walk stopped (all n of them when `pd`).  `failed_order`: None, or the order k of the first minor that is <= 0 (`minors[-1]`).
    When a diagonal entry <= 0 decided the question on the host, no minor was computed: `minors` is empty and `failed_order` is the 1-based index of that
    entry.  `primes`: every prime the device was given, in order; `discarded`: `(prime, order)` for the primes that broke down (a zero pivot at that
    order: the prime divides that minor) and were left out of every minor behind it."""
    pd: bool
    minors: list
    failed_order: Optional[int]
    scale: int
    primes: list
    discarded: list

    def __bool__(self):
        return self.pd


def _product(values) -> int:
    values = list(values)
    while len(values) > 1:
        values = [values[i] * values[i + 1] if i + 1 < len(values) else values[i] for i in range(0, len(values), 2)]
    return values[0] if values else 1


def checkpd(A, device: int = 0, minors=None) -> PDCertificate:
    """Is the symmetric matrix `A` (n <= 128, `Fraction`s or integers) positive definite?  An exact answer with its proof, where the reference asks Arb for a
    ball-arithmetic Cholesky (checkpd_cholesky, src/rounding.jl:447-472).  `ValueError` unless A is square and symmetric.

    M = D A with D the positive least common multiple of the denominators; A is positive definite iff every leading principal minor of M is positive.  An
    empty matrix is positive definite; a diagonal entry <= 0 answers from the host.  Otherwise the minors are computed mod primes taken downward from
    8388593 (`minors(M, primes, device=...)` -> `(residues, breakdown)`, default `leading_minors_mod`; at most 65535 primes per call) and lifted by
    `crt_tree`: for minor k the primes with `breakdown == 0` or `breakdown >= k` are usable, and their product must exceed `2 minor_bounds(M)[k - 1]`.
    The orders are walked upwards; where breakdowns leave too few primes for the next order, more primes are drawn in a further call; the walk stops at the
    first minor <= 0.  A prime at which minor k is not 0 cannot break down at order k or below, so for a non-zero minor only the finitely many primes that
    divide it or an earlier minor are lost; when minor k is 0 every prime breaks down at k at the latest, all are usable for k, and the zero is proven by
    the same bound."""
    from math import gcd
    minors_fn = leading_minors_mod if minors is None else minors
    a = np.asarray(A, dtype=object)
    if a.size == 0 and a.ndim <= 2 and (a.ndim < 2 or a.shape[0] == a.shape[1]):
        return PDCertificate(True, [], None, 1, [], [])
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"checkpd: the matrix must be square, got shape {a.shape}")
    n = a.shape[0]
    rows = [[Fraction(v) for v in a[i]] for i in range(n)]
    if any(rows[i][j] != rows[j][i] for i in range(n) for j in range(i)):
        raise ValueError("checkpd: the matrix must be symmetric")
    scale = 1
    for row in rows:
        for v in row:
            scale = scale * v.denominator // gcd(scale, v.denominator)
    for i in range(n):
        if rows[i][i] <= 0:
            return PDCertificate(False, [], i + 1, scale, [], [])
    if n > MINORS_MAX_N:
        raise ValueError(f"checkpd: blocks of more than {MINORS_MAX_N} rows are not supported, got {n}")
    M = np.zeros((n, n), dtype=object)
    for i in range(n):
        M[i] = [int(v * scale) for v in rows[i]]
    H = minor_bounds(M)
    schedule = _primes_descending()
    primes, breaks, columns = [], [], []                            # per prime: its breakdown and its row of residues
    exact, done, drawn = [], 0, 0                                   # the minors lifted so far (orders 1 .. done)
    while done < n:
        # draw: enough primes that, were none to break down, the product exceeds twice the largest bound still ahead
        need, have = 2 * max(max(H[done:]), 1), _product(p for p, k in zip(primes, breaks) if k == 0)
        batch = []
        while (have <= need or not batch) and len(batch) < MINORS_MAX_PRIMES:
            if drawn >= schedule.size:
                raise ArithmeticError("checkpd: the primes below 2^23 are exhausted")
            batch.append(int(schedule[drawn]))
            have *= batch[-1]
            drawn += 1
        res, brk = minors_fn(M, batch, device=device)
        primes += batch
        breaks += [int(k) for k in brk]
        columns += [np.asarray(r) for r in np.asarray(res)]
        # lift every order whose usable primes suffice, in groups that share their set of usable primes (one tree per group)
        groups, products, order = {}, {}, done + 1
        while order <= n:
            usable = tuple(q for q, k in enumerate(breaks) if k == 0 or k >= order)
            if usable not in products:
                products[usable] = _product(primes[q] for q in usable)
            if not usable or products[usable] <= 2 * H[order - 1]:
                break
            groups.setdefault(usable, []).append(order)
            order += 1
        stop = False
        for usable, orders in groups.items():                      # (insertion order: ascending orders)
            values, _ = crt_tree(np.array([[int(columns[q][k - 1]) for k in orders] for q in usable], dtype=np.int64), [primes[q] for q in usable])
            for k, v in zip(orders, values):
                exact.append(v)
                done = k
                if v <= 0:
                    stop = True
                    break
            if stop:
                break
        if stop:
            break
    discarded = [(p, k) for p, k in zip(primes, breaks) if k != 0]
    failed = done if exact and exact[-1] <= 0 else None
    return PDCertificate(failed is None, exact, failed, scale, primes, discarded)


def is_valid_solution(blocks, A=None, b=None, x=None, check_slacks: bool = True, device: int = 0, minors=None, matmul=None, field=None, primes=None):
    """The numeric part of the reference's `is_valid_solution` (src/rounding.jl:367-415): are the slacks zero, and is every block of the exact solution
    positive definite?  `blocks`: the symmetric blocks (`Fraction`s or integers), each through `checkpd` (`device`, `minors` go there).  With
    `check_slacks` the slacks `A x - b` (`A` (nrows, ncols), `b` (nrows,), `x` (ncols,)) are formed in `Fraction` arithmetic on the host, or, with
    `matmul(A, B, device=...)` (`zz_matmul`: on the device), as ONE integer product of the rows of [A b] cleared of denominators with `L x`, L the common
    denominator of x, divided by L and the row's multiplier entry by entry: the same `Fraction`s.  Returns
    `(success, failures)`: `failures` lists `("constraint", i, slack)` for every constraint i with a non-zero slack and `("block", j, failed_order)` for
    every block j that is not positive definite.

    With `field` (a `NumberField`) the blocks are matrices of coefficient tuples over QQ(g) and go through `checkpd_field` (`minors`, `primes` go there); the
    slack check over a field is not built, so `check_slacks` must be False then."""
    failures = []
    if field is not None and check_slacks:
        raise ValueError("is_valid_solution: the slack check over a number field is not built; pass check_slacks=False")
    if check_slacks:
        if A is None or b is None or x is None:
            raise ValueError("is_valid_solution: A, b and x are needed to check the slacks")
        rows, bf, ncols = _fraction_rows(A, b, "is_valid_solution")
        xf = [Fraction(v) for v in np.asarray(x, dtype=object).reshape(-1)]
        if len(xf) != ncols:
            raise ValueError(f"is_valid_solution: x must have one entry per column of A, got {len(xf)} for {ncols} columns")
        if matmul is not None and rows and ncols:
            cleared = [_common_denominator(rows[i] + [bf[i]]) for i in range(len(rows))]       # row i of [A b] times its multiplier cleared[i][1]
            Ab = np.array([list(c[0]) for c in cleared], dtype=object).reshape(len(rows), ncols + 1)
            yv, L = _common_denominator(xf)
            for i, v in enumerate(_matmul_vector(matmul, Ab[:, :ncols], yv, device)):
                num = v - L * int(Ab[i, ncols])
                if num != 0:
                    failures.append(("constraint", i, Fraction(num, L * cleared[i][1])))
            rows = []
        for i, row in enumerate(rows):
            slack = sum((row[c] * xf[c] for c in range(ncols) if xf[c] != 0), Fraction(0)) - bf[i]
            if slack != 0:
                failures.append(("constraint", i, slack))
    for j, blk in enumerate(blocks):
        cert = checkpd(blk, device=device, minors=minors) if field is None else checkpd_field(blk, field, device=device, minors=minors, primes=primes)
        if not cert.pd:
            failures.append(("block", j, cert.failed_order))
    return not failures, failures


# ---- exact integer matrix products on the device (clrs_zz_gemm): what `matmul=zz_matmul` routes the products of the functions above through ----
ZZ_MAX_DIGITS = 32767                # digit planes of an operand or of the result of clrs_zz_gemm


def _zz_gemm_planes(Ad, Bd, ndc: int, device: int = 0):
    """One call of clrs_zz_gemm on digit planes: `Ad` int32 (nda, m, k), `Bd` int32 (ndb, k, n) -> `(C, info)`, C int32 (ndc, m, n), info int32 (4,).  The
    counters are written before the call raises, so `info` can be read from `zz_matmul.last_info` after a refusal for `ndc` too small."""
    Ad, Bd = np.ascontiguousarray(Ad, dtype=np.int32), np.ascontiguousarray(Bd, dtype=np.int32)
    if Ad.ndim != 3 or Bd.ndim != 3 or Ad.shape[2] != Bd.shape[1]:
        raise ValueError(f"zz_matmul: the digits must be (nda, m, k) and (ndb, k, n), got {Ad.shape} and {Bd.shape}")
    (nda, m, k), (ndb, _, n) = Ad.shape, Bd.shape
    Cd, info = np.zeros((int(ndc), m, n), np.int32), np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.p_i32) if a.size else C_NULL_I32
    try:
        _lib.check(_lib.load().clrs_zz_gemm(int(device), m, k, n, nda, ptr(Ad), ndb, ptr(Bd), int(ndc), ptr(Cd), info.ctypes.data_as(_lib.p_i32)))
    finally:
        zz_matmul.last_info = [int(v) for v in info]
    return Cd, info


def _integer_operand(M, what):
    """-> (a two-dimensional array of integers, whether the input was a vector): a vector is a one-column matrix"""
    a = np.asarray(M)
    vector = a.ndim == 1
    if vector:
        a = a.reshape(-1, 1)
    if a.size == 0:
        if a.ndim != 2:
            raise ValueError(f"{what}: the operands must be matrices or vectors, got shape {a.shape}")
        return np.zeros(a.shape, dtype=np.int64), vector
    return _integer_matrix(a, what), vector


def zz_matmul(A, B, device: int = 0) -> np.ndarray:
    """The exact product `A B` of integer matrices on the device, one call of clrs_zz_gemm: `A` (m, k) and `B` (k, n) of integers
    of any size (anything `np.asarray` takes; object arrays of Python integers); a vector is a one-column matrix, and the product with a vector `B` is a
    vector, as with `numpy.dot`.  Returns an object array of Python integers.  The operands cross in balanced base-2^24 digits (`ints_to_planes`); the
    result takes `ndc` digits computed from `k max|A| max|B|`.  The counters of the call are kept in `zz_matmul.last_info` (`[entries that did not fit,
    ranges of digits, GEMM workgroups, 0]`).  This is the `matmul=` of `solve_dixon`, `solve_system_pseudoinverse`, `project_to_affine_space` and
    `is_valid_solution`."""
    a, _ = _integer_operand(A, "zz_matmul")
    b, vector = _integer_operand(B, "zz_matmul")
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"zz_matmul: the shapes {a.shape} and {b.shape} do not match")
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    out = np.zeros((m, n), dtype=object)
    if m and n and k:
        Ad, Bd = ints_to_planes(a), ints_to_planes(b)
        bound = k * max(abs(int(a.max())), abs(int(a.min()))) * max(abs(int(b.max())), abs(int(b.min())))
        ndc = max((bound.bit_length() + DIGIT_BITS + 1) // DIGIT_BITS, 1)         # 24 ndc >= bits + 2: twice the bound is below 2^(24 ndc - 1), which ndc digits hold
        if max(Ad.shape[0], Bd.shape[0], ndc) > ZZ_MAX_DIGITS:
            raise ValueError(f"zz_matmul: an operand or the result needs more than {ZZ_MAX_DIGITS} digits")
        Cd, _ = _zz_gemm_planes(Ad, Bd, ndc, device=device)
        out = planes_to_ints(Cd)
    else:
        zz_matmul.last_info = [0, 0, 0, 0]
    return out.reshape(m) if vector else out


zz_matmul.last_info = None


def _common_denominator(values):
    """Fractions (or integers) -> `(y, L)`: L the least common multiple of the denominators, y the object vector of the integers `value L`"""
    from math import gcd
    fr = [Fraction(v) for v in values]
    L = 1
    for v in fr:
        L = L * v.denominator // gcd(L, v.denominator)
    return _object_vector([v.numerator * (L // v.denominator) for v in fr]), L


def _matmul_vector(matmul, M, y, device):
    """`matmul(M, y)` for an integer matrix M and an integer vector y, as a list of Python integers"""
    out = np.asarray(matmul(M, y, device=device), dtype=object).reshape(-1)
    if out.size != np.asarray(M).shape[0]:
        raise ArithmeticError(f"matmul returned {out.size} entries for {np.asarray(M).shape[0]} rows")
    return [int(v) for v in out]


# ---- the exact solve with a matrix of right-hand sides, the inverse over QQ and the basis change (src/rounding.jl:750-858, 1191-1253; clrs_modp_dixon_lift_multi) ----
def _object_matrix(M, what, cast=int) -> np.ndarray:
    """anything two-dimensional -> an object array of `cast(entry)`; an empty input keeps its shape when it has two dimensions and becomes 0 x 0 otherwise"""
    a = np.asarray(M, dtype=object)
    if a.size == 0:
        return np.zeros((a.shape[0], a.shape[1]) if a.ndim == 2 else (0, 0), dtype=object)
    if a.ndim != 2:
        raise ValueError(f"{what}: a matrix must be two-dimensional, got shape {a.shape}")
    out = np.empty(a.shape, dtype=object)
    out.flat = [cast(v) for v in a.flat]
    return out


def _dixon_lift_multi_digits(Ad, Bl, p: int, steps: int, device: int = 0):
    """One call of clrs_modp_dixon_lift_multi on digit planes: `Ad` int32 (nd, n, n), `Bl` int32 (nbl, n, m).  Returns `(X, R_limbs, info)`: X int32
    (steps, n, m), R_limbs int32 (nrl, n, m), info int32 (6,)."""
    Ad, Bl = np.ascontiguousarray(Ad, dtype=np.int32), np.ascontiguousarray(Bl, dtype=np.int32)
    if Ad.ndim != 3 or Bl.ndim != 3 or Ad.shape[2] != Ad.shape[1] or Bl.shape[1] != Ad.shape[1]:
        raise ValueError(f"dixon_lift_multi: the digits of A must be (nd, n, n) and the limbs of B (nbl, n, m), got {Ad.shape} and {Bl.shape}")
    nd, n, nbl, m, steps = Ad.shape[0], Ad.shape[1], Bl.shape[0], Bl.shape[2], int(steps)
    nrl = max(nbl, nd + 1) + 1
    X = np.zeros((max(steps, 0), n, m), np.int32)
    R = np.zeros((nrl, n, m), np.int32)
    info = np.zeros(6, np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.p_i32) if a.size else C_NULL_I32
    _lib.check(_lib.load().clrs_modp_dixon_lift_multi(int(device), n, m, int(p), nd, ptr(Ad), nbl, ptr(Bl), steps, ptr(X), ptr(R), ptr(info)))
    dixon_lift_multi.last_info = [int(v) for v in info]
    return X, R, info


def dixon_lift_multi(A, B, p: int, steps: int, device: int = 0):
    """`steps` steps of Dixon's p-adic lifting of the integer system A X = B (A n x n, B n x m, Python integers of any size) on the device: one call of
    clrs_modp_dixon_lift_multi, which lifts all columns side by side (both products of a step are matrix products).  Per column the result is that of
    `dixon_lift`.  Returns `(X, R, rank)`: X int32 (steps, n, m), residues in [0, p); R an object array (n, m), the last residual as Python integers, so that
    `A sum_k X[k] p^k == B - p^steps R`; rank the rank of A mod p.  When rank < n nothing was lifted: `(None, None, rank)`.  With m = 0 (and n > 0) there is
    nothing to lift and the rank is not examined: it is reported as n.  The counters of the call are kept in `dixon_lift_multi.last_info` (`[rank, steps,
    remainders, overflows, chunks of columns, impossible GEMM pairs]`)."""
    A, B = _object_matrix(_integer_matrix(A, "dixon_lift_multi"), "dixon_lift_multi"), np.asarray(B)
    n = A.shape[0]
    if A.shape[1] != n:
        raise ValueError(f"dixon_lift_multi: A must be square, got {A.shape}")
    if B.ndim != 2 or B.shape[0] != n:
        raise ValueError(f"dixon_lift_multi: B must be (n, m) with one row per row of A, got shape {B.shape} for n = {n}")
    m = B.shape[1]
    B = _object_matrix(_integer_matrix(B, "dixon_lift_multi"), "dixon_lift_multi") if B.size else np.zeros((n, m), dtype=object)
    p, steps = int(p), int(steps)
    _check_modp_prime("dixon_lift_multi", p)
    if n > LIFT_MAX_N or steps < 0:
        raise ValueError(f"dixon_lift_multi: n must be at most {LIFT_MAX_N} and steps at least 0, got n = {n}, steps = {steps}")
    if n == 0 or m == 0:
        dixon_lift_multi.last_info = [0, steps, 0, 0, 0, 0]
        return np.zeros((steps, n, m), np.int32), np.zeros((n, m), dtype=object), n
    X, R, info = _dixon_lift_multi_digits(ints_to_planes(A), ints_to_planes(B), p, steps, device=device)
    rank = int(info[0])
    if rank < n:
        return None, None, rank
    return X, planes_to_ints(R), rank


dixon_lift_multi.last_info = None


class DixonSolutionMatrix(np.ndarray):
    """The solution `solve_dixon_multi` returns: an object array (n, m) of `Fraction`s with three attributes, `p` (the prime lifted at; None when nothing
    was lifted), `primes` (the primes tried, in order) and `steps` (the lifting steps)."""

    def __new__(cls, values, p=None, primes=(), steps=0):
        obj = np.asarray(values, dtype=object).view(cls)
        obj.p = None if p is None else int(p)
        obj.primes = [int(q) for q in primes]
        obj.steps = int(steps)
        return obj

    def __array_finalize__(self, obj):
        self.p = getattr(obj, "p", None)
        self.primes = list(getattr(obj, "primes", []))
        self.steps = getattr(obj, "steps", 0)


def _column_denominators(S):
    """an object matrix of Fractions -> `(Y, L)`: L[j] the least common multiple of the denominators of column j, Y[:, j] = S[:, j] L[j] as Python integers"""
    from math import gcd
    Y, L = np.zeros(S.shape, dtype=object), []
    for j in range(S.shape[1]):
        l = 1
        for v in S[:, j]:
            l = l * v.denominator // gcd(l, v.denominator)
        L.append(l)
        Y[:, j] = [v.numerator * (l // v.denominator) for v in S[:, j]]
    return Y, L


def _matmul_matrix(matmul, A, B, device):
    """the product of two integer matrices as an object matrix of Python integers: ONE call of `matmul`, or the host product when it is None"""
    if matmul is None:
        return _object_matrix(A.dot(B), "matmul")
    out = _object_matrix(np.asarray(matmul(A, B, device=device), dtype=object).reshape(A.shape[0], B.shape[1]), "matmul")
    return out


def solve_dixon_multi(A, B, maxprimes: int = 3, device: int = 0, lift=None, check: bool = True, reconstruct=None, matmul=None) -> DixonSolutionMatrix:
    """The exact solution of the square system A X = B with a matrix of right-hand sides: `A` (n, n) and `B` (n, m) of integers or `Fraction`s;
    `solve_dixon` column by column, as ONE lifting.  Every row of [A B] is cleared of denominators; the schedule of primes is that of `solve_dixon`
    (downward from 8388593, at most `maxprimes`); there is one `K = dixon_steps(A, b, p)[0]` for all columns, b the column of B of largest norm (its Cramer
    bound holds for every column); every entry is reconstructed from `sum_k X[k] p^k mod p^K`.  Returns a `DixonSolutionMatrix` (n, m).  Raises
    `SingularSystemError` when A is singular mod every prime tried, `ValueError` for `maxprimes < 1` or shapes that do not match, and, with `check`,
    `ArithmeticError` unless `A X == B - p^K R_K` holds for the lifted integers and `A solution == B` for the fractions; the second is tested as
    `Ai Y == Bi diag(L)` over one common denominator L[j] per column (Y[:, j] = L[j] solution[:, j]; Ai, Bi the rows cleared of denominators).
    `lift(A, B, p, steps, device=...)` -> `(X, R, rank)` replaces the device call (default `dixon_lift_multi`).
    `reconstruct(X, p, N, D, device=..., want_x=...)` as in `solve_dixon`; it is fed `X.reshape(steps, n m)` in pieces of at most 32767 entries
    (`dixon_reconstruct` takes no more).  `matmul(A, B, device=...)` (`zz_matmul`) takes the two products of the checks, as one matrix product each."""
    lift = dixon_lift_multi if lift is None else lift
    if int(maxprimes) < 1:
        raise ValueError(f"solve_dixon_multi: maxprimes must be at least 1, got {maxprimes}")
    Af, Bf = _object_matrix(A, "solve_dixon_multi", Fraction), np.asarray(B, dtype=object)
    n = Af.shape[0]
    if Af.shape[1] != n:
        raise ValueError(f"solve_dixon_multi: A must be square, got {Af.shape[0]} x {Af.shape[1]}")
    if Bf.ndim != 2 or Bf.shape[0] != n:
        raise ValueError(f"solve_dixon_multi: B must be (n, m) with one row per row of A, got shape {Bf.shape} for n = {n}")
    m = Bf.shape[1]
    if n == 0 or m == 0:
        return DixonSolutionMatrix(np.zeros((n, m), dtype=object))
    Bf = _object_matrix(Bf, "solve_dixon_multi", Fraction)
    AB = _rows_cleared_of_denominators([list(Af[r]) + list(Bf[r]) for r in range(n)])
    Ai, Bi = AB[:, :n], AB[:, n:]
    norms = [sum(int(v) * int(v) for v in Bi[:, j]) for j in range(m)]
    bmax = Bi[:, norms.index(max(norms))]
    p, primes = DIXON_FIRST_PRIME + 1, []
    for _ in range(int(maxprimes)):
        p = prev_prime(p)
        primes.append(p)
        K, N, D = dixon_steps(Ai, bmax, p)
        X, R, rank = lift(Ai, Bi, p, K, device=device)
        if rank == n:
            break
    else:
        raise SingularSystemError(f"solve_dixon_multi: the matrix is singular mod every prime tried ({primes})")
    q = p ** K
    X = np.asarray(X)
    sol, x = None, None
    if reconstruct is None:
        x = np.zeros((n, m), dtype=object)
        for k in range(K - 1, -1, -1):                          # Horner: x = sum_k X[k] p^k
            x = x * p + X[k].astype(object)
        flat = None
    else:
        Xf = np.ascontiguousarray(X.reshape(K, n * m))
        flat, xs = [], []
        for a in range(0, n * m, LIFT_MAX_N):
            piece = reconstruct(np.ascontiguousarray(Xf[:, a:a + LIFT_MAX_N]), p, N, D, device=device, want_x=bool(check))
            if check:
                flat.extend(piece[0]); xs.extend(int(v) for v in piece[1])
            else:
                flat.extend(piece)
        if check:
            x = _object_vector(xs).reshape(n, m)
    if check:
        lhs, rhs = _matmul_matrix(matmul, Ai, x, device), Bi - q * _object_matrix(R, "solve_dixon_multi")
        if any(int(v) != int(w) for v, w in zip(lhs.flat, rhs.flat)):
            raise ArithmeticError(f"solve_dixon_multi: A X != B - p^K R after {K} steps at p = {p}")
    if flat is None:
        flat = [rational_reconstruction(int(v), q, N, D) for v in x.flat]
    if any(v is None for v in flat):
        e = [v is None for v in flat].index(True)
        raise ArithmeticError(f"solve_dixon_multi: entry {divmod(e, m)} has no rational reconstruction within the bounds")
    sol = _object_vector(flat).reshape(n, m)
    if check:
        Y, L = _column_denominators(sol)
        lhs = _matmul_matrix(matmul, Ai, Y, device)
        if any(int(lhs[i, j]) != L[j] * int(Bi[i, j]) for i in range(n) for j in range(m)):
            raise ArithmeticError("solve_dixon_multi: A solution != B")
    return DixonSolutionMatrix(sol, p, primes, K)


def inverse_qq(B, maxprimes: int = 3, device: int = 0, lift=None, check: bool = True, reconstruct=None, matmul=None) -> DixonSolutionMatrix:
    """The inverse over QQ of a square matrix of integers or `Fraction`s (the reference's `inv(B)`, src/rounding.jl:836): `solve_dixon_multi(B, I)`, to which
    every keyword goes.  Raises `SingularSystemError` on a singular matrix."""
    Bf = _object_matrix(B, "inverse_qq", Fraction)
    n = Bf.shape[0]
    if Bf.shape[1] != n:
        raise ValueError(f"inverse_qq: the matrix must be square, got {Bf.shape[0]} x {Bf.shape[1]}")
    eye = np.zeros((n, n), dtype=object)
    for i in range(n):
        eye[i, i] = 1
    return solve_dixon_multi(Bf, eye, maxprimes=maxprimes, device=device, lift=lift, check=check, reconstruct=reconstruct, matmul=matmul)


def complete_basis(V, maxprimes: int = 3, device: int = 0, batch=None, below: Optional[int] = None) -> PivotList:
    """The standard basis vectors that complete the independent columns of `V` ((N, s), integers or `Fraction`s) to a basis of QQ^N: the indices i of the pivot
    columns s + i of the reduced row-echelon form mod a prime p of `[V with its rows cleared of denominators | I_N]` (scaling a row by a non-zero factor does
    not change which e_i depend on the columns before them).  This is the greedy choice of the reference's Gram-Schmidt loop (src/rounding.jl:1032-1049) --
    e_i in ascending order, kept when it is independent of the columns of V and the e_j kept so far -- but decided by exact arithmetic mod p and not at
    a threshold of 1e-40 on 512-bit floating-point numbers.  The primes are taken downward from 8388593 (or from below `below`), at most `maxprimes` of
    them; a prime is accepted only when the first s pivots are the columns 0 ... s - 1, i.e. when the columns of V stay independent mod p, otherwise the
    next prime is taken; `ValueError` when no prime of the schedule is accepted (V has dependent columns, or `maxprimes` was too small).  Whatever the prime,
    [V | e_i chosen] is invertible mod p and hence over QQ; the choice is the greedy one over QQ unless p divides one of the minors that decide it, which
    `basis_transformations` rules out afterwards from the inverse.  Returns a `PivotList` of N - s indices with `.p` and `.primes`.
    `batch(A, p, device=...)` -> `(pivots, rank)` replaces the device call (default `rref_mod_p`)."""
    batch = rref_mod_p if batch is None else batch
    if int(maxprimes) < 1:
        raise ValueError(f"complete_basis: maxprimes must be at least 1, got {maxprimes}")
    Vf = np.asarray(V, dtype=object)
    if Vf.ndim != 2:
        raise ValueError(f"complete_basis: V must be (N, s), got shape {Vf.shape}")
    N, s = Vf.shape
    if s > N:
        raise ValueError(f"complete_basis: {s} vectors of {N} entries cannot be independent")
    if s == 0:
        return PivotList(range(N))
    Vi = _rows_cleared_of_denominators([[Fraction(v) for v in Vf[r]] for r in range(N)])
    M = np.zeros((N, s + N), dtype=object)
    M[:, :s] = Vi
    for i in range(N):
        M[i, s + i] = 1
    p, primes = (DIXON_FIRST_PRIME + 1 if below is None else int(below)), []
    for _ in range(int(maxprimes)):
        p = prev_prime(p)
        primes.append(p)
        pivots = [int(c) for c in batch(M, p, device=device)[0]]
        if pivots[:s] == list(range(s)):
            if len(pivots) != N:
                raise ArithmeticError(f"complete_basis: {len(pivots)} pivots for {N} rows at p = {p}")
            return PivotList([c - s for c in pivots[s:]], primes, p)
    raise ValueError(f"complete_basis: the columns of V are dependent mod every prime tried ({primes})")


def _rational_matmul(P, Q, matmul, device):
    """the product of two object matrices of Fractions: in Fractions, or with `matmul` as ONE integer product over a common denominator per operand"""
    if matmul is None or P.size == 0 or Q.size == 0:
        return _object_matrix(P.dot(Q), "transform", Fraction) if P.shape[1] else _object_matrix(np.zeros((P.shape[0], Q.shape[1]), dtype=object), "transform", Fraction)
    (pn, pl), (qn, ql) = _common_denominator(P.flat), _common_denominator(Q.flat)
    prod = _matmul_matrix(matmul, pn.reshape(P.shape), qn.reshape(Q.shape), device)
    return _object_matrix(prod, "transform", lambda v: Fraction(int(v), pl * ql))


def transform(M, Binv, s: int, matmul=None, device: int = 0) -> np.ndarray:
    """The reference's `transform(p, Binv, s)` (src/rounding.jl:1191-1196) for an exact rational matrix: `Binv[s:, :] M Binv^T[:, s:]`, an object array
    (N - s, N - s) of `Fraction`s.  The two products are taken in `Fraction`s, or, with `matmul(A, B, device=...)` (`zz_matmul`), as integer products over
    common denominators."""
    Mf, Bf, s = _object_matrix(M, "transform", Fraction), _object_matrix(Binv, "transform", Fraction), int(s)
    N = Bf.shape[0]
    if Bf.shape[1] != N or Mf.shape != (N, N) or not 0 <= s <= N:
        raise ValueError(f"transform: M and Binv must be (N, N) and 0 <= s <= N, got {Mf.shape}, {Bf.shape} and s = {s}")
    P = Bf[s:, :]
    return _rational_matmul(_rational_matmul(P, Mf, matmul, device), P.T, matmul, device)


def undo_transform(Mt, Binv, s: int, matmul=None, device: int = 0) -> np.ndarray:
    """The reference's `undo_transform` of one block (src/rounding.jl:1239-1253): `Mt` ((N - s, N - s), exact rationals) is padded with s zero rows and
    columns in front and multiplied by `Binv^T` from the left and `Binv` from the right: `transform(padded, Binv^T, 0)`.  `matmul` as in `transform`."""
    Bf, s = _object_matrix(Binv, "undo_transform", Fraction), int(s)
    N = Bf.shape[0]
    Mf = _object_matrix(Mt, "undo_transform", Fraction)
    if Bf.shape[1] != N or not 0 <= s <= N or Mf.shape != (N - s, N - s):
        raise ValueError(f"undo_transform: Binv must be (N, N) and Mt (N - s, N - s), got {Bf.shape}, {Mf.shape} and s = {s}")
    padded = _object_matrix(np.zeros((N, N), dtype=object), "undo_transform", Fraction)
    padded[s:, s:] = Mf
    return transform(padded, Bf.T, 0, matmul=matmul, device=device)


# ---- LLL reduction of a batch of lattices; the reduced, unimodular basis change (src/rounding.jl:860-1104; clrs_zz_lll) ------------------
LLL_LIMBS = (2, 4, 6)                # the rungs of the ladder: the fp64 words of the Gram-Schmidt data clrs_zz_lll is instantiated for
LLL_MAX_ROWS, LLL_MAX_COLS, LLL_MAX_DIGITS = 128, 256, 20


class ReductionError(ArithmeticError):
    """`lll_batch` could not reduce a lattice: status 1 or 2 on the last rung of the ladder, or entries beyond the digits clrs_zz_lll takes; or
    `reduce_kernel_vectors` could not verify a block on the last rung."""


def lll_first_rung(bits: int, d: int) -> int:
    """The rung (fp64 words of the Gram-Schmidt data) a lattice of `d` rows with entries of at most `bits` bits starts on: the least of 2, 4, 6 words with
    53 words >= 2 bits + ceil(1.6 d) + 10 (2 bits for the cancellation in r_kk = G_kk - sum mu_kj r_kj of a size-reduced row,
    1.6 d for the growth of errors along the Cholesky row at (delta, eta) = (0.99, 0.51), 10 to spare), else 6."""
    need = 2 * int(bits) + -(-8 * int(d) // 5) + 10
    return next((K for K in LLL_LIMBS if 53 * K >= need), LLL_LIMBS[-1])


def _lll_call_device(rows, cols, cols_gram, nd, digits, delta, eta, limbs, max_swaps, device=0):
    """one call of clrs_zz_lll: `digits` the packed planes (int32, flat); returns (out (flat, zeros where nothing was written), info (nb, 8))"""
    rows, cols, cols_gram = (np.ascontiguousarray(a, np.int32) for a in (rows, cols, cols_gram))
    digits = np.ascontiguousarray(digits, np.int32).reshape(-1)
    out, info = np.zeros(max(digits.size, 1), np.int32), np.zeros((max(rows.size, 1), 8), np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.p_i32)
    _lib.check(_lib.load().clrs_zz_lll(int(device), int(rows.size), ptr(rows), ptr(cols), ptr(cols_gram), int(nd), ptr(digits) if digits.size else ptr(out), ptr(out),
                                       float(delta), float(eta), int(limbs), int(max_swaps), ptr(info)))
    return out[:digits.size], info[:rows.size]


def lll_batch(lattices, delta: float = 0.99, eta: float = 0.51, transform: bool = False, limbs: Optional[int] = None, device: int = 0, cols_gram=None,
              max_swaps: Optional[int] = None, call=None):
    """LLL-reduce a batch of integer lattices on the device (clrs_zz_lll, one workgroup per lattice).  `lattices`: matrices of Python integers (anything
    `np.asarray` takes), each with at most 128 independent rows and 256 columns.  Returns the reduced bases as object arrays, in order; with `transform`
    pairs `(out, U)` with `U` unimodular and `U A == out` (an identity is appended to the rows and kept out of the dot products).  `cols_gram`: per lattice
    the number of leading columns the dot products run over (default: all).  Every row operation is exact, so `out` spans the lattice of the input
    whatever the floating point does; `(delta, eta)` are what the floating-point Gram-Schmidt data aim at.
    Per lattice: the digits `nd` come from the bit length of its entries plus 40 bits of headroom, and on status 3 (an entry left its digits) the lattice is
    repeated with two more; the first rung is `lll_first_rung(bits, d)` (or `limbs`), and on status 1 or 2 the lattice alone is repeated on the next rung
    from its original input; past the last rung, or past 20 digits, `ReductionError`.  `max_swaps` defaults to twice the potential bound
    d (d - 1) log2(max row norm) / log2(1 / delta), clipped to int32.  Lattices that share (rung, digits) go in one device call, which takes ONE cap: the
    largest of its members'.  A lattice in a batch may so be given more exchanges than it would get alone, never fewer: a lattice that ends with status 0
    gives the digits and counters of its single call, and only where a cap is reached (status 1) can the batch differ from the single calls.  The counters are kept in
    `lll_batch.last_info`: per lattice a dict with `status`, `swaps`, `passes`, `launches`, `limbs`, `nd` and `rungs`, the list of every
    (limbs, nd, status) tried.  `call` replaces the device call (the tests' host build)."""
    from math import log2
    call = _lll_call_device if call is None else call
    if limbs is not None and int(limbs) not in LLL_LIMBS:
        raise ValueError(f"lll_batch: limbs must be one of {LLL_LIMBS}, got {limbs}")
    mats, grams, jobs = [], [], []
    for idx, A in enumerate(lattices):
        a = _integer_matrix(A, "lll_batch")
        a = np.array([int(v) for v in a.flat], dtype=object).reshape(a.shape)
        d, c = a.shape
        g = c if cols_gram is None else int(cols_gram[idx])
        if d > LLL_MAX_ROWS or c + (d if transform else 0) > LLL_MAX_COLS or not 0 <= g <= c or (d and g < 1):
            raise ValueError(f"lll_batch: lattice {idx}: at most {LLL_MAX_ROWS} rows and {LLL_MAX_COLS} columns (the identity of `transform` included) and "
                             f"1 <= cols_gram <= cols, got {d} x {c} and cols_gram = {g}")
        if transform:
            wide = np.zeros((d, c + d), dtype=object)
            wide[:, :c] = a
            for i in range(d):
                wide[i, c + i] = 1
            a = wide
        mats.append(a)
        grams.append(g)
        bits = max((abs(int(v)).bit_length() for v in a.flat), default=0)
        norm2 = max((sum(int(v) * int(v) for v in a[i, :g]) for i in range(d)), default=1)
        bound = 2.0 * d * (d - 1) * max(0.5 * log2(max(norm2, 2)), 1.0) / log2(1.0 / delta) if delta < 1 else float(2 ** 31 - 1)
        jobs.append({"rung": LLL_LIMBS.index(int(limbs) if limbs is not None else lll_first_rung(bits, d)), "nd": (bits + 40) // DIGIT_BITS + 1,
                     "max_swaps": int(min(max(bound, 16.0), 2 ** 31 - 1)) if max_swaps is None else int(max_swaps), "rungs": [], "out": None, "info": None})
    pending = list(range(len(mats)))
    while pending:
        groups = {}
        for idx in pending:
            if jobs[idx]["nd"] > LLL_MAX_DIGITS:
                lll_batch.last_info = [dict(j["info"] or {}, rungs=j["rungs"]) for j in jobs]
                raise ReductionError(f"lll_batch: lattice {idx} needs {jobs[idx]['nd']} digits of {DIGIT_BITS} bits, clrs_zz_lll takes {LLL_MAX_DIGITS}")
            groups.setdefault((jobs[idx]["rung"], jobs[idx]["nd"]), []).append(idx)
        pending = []
        for (rung, nd), members in sorted(groups.items()):
            K = LLL_LIMBS[rung]
            planes = [ints_to_planes(mats[i], nd) if mats[i].size else np.zeros((nd,) + mats[i].shape, np.int32) for i in members]
            digits = np.concatenate([p.reshape(-1) for p in planes]) if planes else np.zeros(0, np.int32)
            out, info = call([mats[i].shape[0] for i in members], [mats[i].shape[1] for i in members], [grams[i] for i in members], nd, digits, delta, eta, K,
                             max(jobs[i]["max_swaps"] for i in members), device=device)
            off = 0
            for pos, i in enumerate(members):
                count, job = planes[pos].size, jobs[i]
                status = int(info[pos][0])
                job["rungs"].append((K, nd, status))
                job["info"] = {"status": status, "swaps": int(info[pos][1]), "passes": int(info[pos][2]), "launches": int(info[pos][3]), "limbs": K, "nd": nd}
                if status == 0:
                    job["out"] = planes_to_ints(np.asarray(out[off:off + count]).reshape(planes[pos].shape)) if count else mats[i].copy()
                elif status == 3:
                    job["nd"] += 2
                    pending.append(i)
                elif status in (1, 2) and rung + 1 < len(LLL_LIMBS):
                    job["rung"] += 1
                    pending.append(i)
                else:
                    lll_batch.last_info = [dict(j["info"] or {}, rungs=j["rungs"]) for j in jobs]
                    raise ReductionError(f"lll_batch: lattice {i}: status {status} on the last rung ({K} words, {nd} digits); tried {job['rungs']}")
                off += count
    lll_batch.last_info = [dict(j["info"] or {}, rungs=j["rungs"]) for j in jobs]
    if not transform:
        return [j["out"] for j in jobs]
    return [(j["out"][:, :j["out"].shape[1] - j["out"].shape[0]], j["out"][:, j["out"].shape[1] - j["out"].shape[0]:]) for j in jobs]


lll_batch.last_info = None


def lll(A, delta: float = 0.99, eta: float = 0.51, transform: bool = False, limbs: Optional[int] = None, device: int = 0, **kw):
    """`lll_batch` for one lattice: the reduced basis of the rows of `A`, or `(out, U)` with `transform`."""
    return lll_batch([A], delta=delta, eta=eta, transform=transform, limbs=limbs, device=device, **kw)[0]


def kernel_lattice(N: int, s: int, M, R: int, q_extra: int = 0):
    """The lattice whose reduction gives the unimodular basis change of a block: the N rows of `[lambda M^T | I_N]`, an object
    matrix N x (N - s + N), with `M` ((N - s) x N, integers of rank N - s whose integer kernel is the lattice L wanted) and lambda = 2^(24 q), q the least
    with 24 q >= ceil((N - 1) / 2) + ceil(log2 R) + 2 (`R` an integer: L holds s independent vectors of norm <= R), plus `q_extra`.  Returns (rows, q)."""
    N, s, R = int(N), int(s), max(int(R), 1)
    M = _integer_matrix(M, "kernel_lattice")
    if M.shape != (N - s, N):
        raise ValueError(f"kernel_lattice: M must be ({N - s}, {N}), got {M.shape}")
    need = -(-(N - 1) // 2) + (R - 1).bit_length() + 2
    q = -(-need // DIGIT_BITS) + int(q_extra)
    rows = np.zeros((N, N - s + N), dtype=object)
    for i in range(N):
        for r in range(N - s):
            rows[i, r] = int(M[r, i]) << (DIGIT_BITS * q)
        rows[i, N - s + i] = 1
    return rows, q


def reduce_kernel_vectors(blocks, settings: Optional[RoundingSettings] = None, device: int = 0, matmul=None, lll=None):
    """The reduction of the kernel vectors of every block in ONE `lll_batch` call (the reference's `reduction_step`, src/rounding.jl:1062-1104, without an
    HNF).  `blocks`: a list of `(N, s, M, R)` as `kernel_lattice` takes them, 0 < s < N.  Returns per block the integer matrix `U` (N x N, an object array):
    unimodular by construction, its first s rows an LLL-reduced Z-basis of `L = {u in Z^N : M u = 0}`.  What the rest of the chain relies on is verified
    exactly: the left part `lambda M u` of the first s reduced rows is zero and that of the others is not, and `M U^T[:, :s] == 0` as one product
    (`matmul(A, B, device=...)`, default Python integers).  A block that fails is repeated with lambda 2^24 times as large, then on the next rung of the
    ladder, and is a `ReductionError` past the last.  `lll` replaces `lll_batch` (same keywords).  `settings` is the second argument every `reduce=` hook is
    called with; this one reads nothing from it (delta and eta are `lll_batch`'s defaults, FLINT's)."""
    reduce_batch = lll_batch if lll is None else lll
    blocks = [(int(N), int(s), _integer_matrix(M, "reduce_kernel_vectors"), int(R)) for N, s, M, R in blocks]
    for N, s, M, R in blocks:
        if not 0 < s < N or N > LLL_MAX_ROWS:
            raise ValueError(f"reduce_kernel_vectors: 0 < s < N <= {LLL_MAX_ROWS} is needed, got N = {N}, s = {s}")
    out = [None] * len(blocks)
    attempts = [(0, None)] + [(1, None)] + [(1, K) for K in LLL_LIMBS[1:]]            # (more of lambda, rung): each block walks this list on its own
    step = [0] * len(blocks)
    todo = list(range(len(blocks)))
    infos = [None] * len(blocks)
    while todo:
        ready = {}
        for b in todo:
            ready.setdefault(attempts[step[b]][1], []).append(b)
        todo = []
        for K, members in ready.items():
            lattices = [kernel_lattice(*blocks[b], q_extra=attempts[step[b]][0])[0] for b in members]
            reduced = reduce_batch(lattices, limbs=K, device=device)
            last = getattr(reduce_batch, "last_info", None)
            for pos, (b, red) in enumerate(zip(members, reduced)):
                N, s, M, _ = blocks[b]
                infos[b] = last[pos] if last else None
                left, U = red[:, :N - s], red[:, N - s:]
                ok = all(int(v) == 0 for v in left[:s].flat) and all(any(int(v) != 0 for v in left[i]) for i in range(s, N))
                if ok:
                    prod = _matmul_matrix(matmul, np.array([int(v) for v in M.flat], dtype=object).reshape(M.shape), np.ascontiguousarray(U[:s].T), device)
                    ok = all(int(v) == 0 for v in np.asarray(prod, dtype=object).flat)
                if ok:
                    out[b] = U
                    continue
                step[b] += 1
                while step[b] < len(attempts) and attempts[step[b]][1] is not None and infos[b] and attempts[step[b]][1] <= infos[b].get("limbs", 0):
                    step[b] += 1                                                        # (a rung the ladder of lll_batch has already passed)
                if step[b] >= len(attempts):
                    raise ReductionError(f"reduce_kernel_vectors: block {b} (N = {N}, s = {s}) failed its exact verification on every rung")
                todo.append(b)
    reduce_kernel_vectors.last_info = infos
    return out


reduce_kernel_vectors.last_info = None


def _unreduced_basis(key, N, vectors, settings, device, maxprimes, batch, lift, check, reconstruct, matmul):
    """B = [V | E] with the greedy completion E and Binv = inverse_qq(B), not normalised (the loop over primes of `basis_transformations`)"""
    s = len(vectors)
    B = _object_matrix(np.zeros((N, N), dtype=object), "basis_transformations", Fraction)
    for c, v in enumerate(vectors):
        if len(v) != N:
            raise ValueError(f"basis_transformations: block {key!r}: vector {c} has {len(v)} entries for a block of size {N}")
        B[:, c] = [Fraction(x) for x in v]
    below = None
    for _ in range(int(maxprimes)):
        extra = complete_basis(B[:, :s], maxprimes=maxprimes, device=device, batch=batch, below=below)
        B[:, s:] = Fraction(0)
        for c, i in enumerate(extra):
            B[i, s + c] = Fraction(1)
        Binv = np.asarray(inverse_qq(B, maxprimes=maxprimes, device=device, lift=lift, check=check, reconstruct=reconstruct, matmul=matmul))
        taken = set(extra)
        if all(Binv[s + c, i] == 0 for i in range(N) if i not in taken for c, j in enumerate(extra) if j > i):
            return B, Binv
        below = extra.p
    raise ArithmeticError(f"basis_transformations: block {key!r}: no prime gave the greedy completion of the kernel vectors")


def _normalized(B, Binv):
    """row i of Binv times the least common multiple of its denominators, column i of B divided by it (src/rounding.jl:844-850), in place"""
    from math import gcd
    for i in range(B.shape[0]):
        l = 1
        for v in Binv[i]:
            l = l * v.denominator // gcd(l, v.denominator)
        Binv[i] = [v * l for v in Binv[i]]
        B[:, i] = [v / l for v in B[:, i]]


def _kernel_block(N, vectors, Binv0):
    """(N, s, M, R) of a block for `reduce_kernel_vectors`: M = the rows s .. N - 1 of inv([V | E]), which annihilate V, each cleared of denominators and of
    its content; R = an integer bound on the norms of the vectors times the lcm of their denominators"""
    from math import gcd, isqrt
    s = len(vectors)
    M = _rows_cleared_of_denominators([[Fraction(v) for v in Binv0[r]] for r in range(s, N)])
    for r in range(M.shape[0]):
        g = 0
        for v in M[r]:
            g = gcd(g, int(v))
        if g > 1:
            M[r] = [int(v) // g for v in M[r]]
    R2 = 1
    for v in vectors:
        cleared = _rows_cleared_of_denominators([[Fraction(x) for x in v]])[0]
        R2 = max(R2, sum(int(x) * int(x) for x in cleared))
    return N, s, M, isqrt(R2) + 1


def basis_transformations(kernels, settings: Optional[RoundingSettings] = None, device: int = 0, maxprimes: int = 3, batch=None, lift=None, check: bool = True,
                          reconstruct=None, matmul=None, reduce=None, verbose: bool = False, field=None, adjugate=None, primes=None) -> dict:
    """The reference's `basis_transformations` over QQ (src/rounding.jl:750-858).  `kernels` maps a block key to `(N, vectors)`: the size of the block and
    its s rational kernel vectors, each of N entries (what `vectors_to_fractions(BlockKernel)` returns).  Returns `{key: (B^T, Binv, s)}`, object arrays
    (N, N) of `Fraction`s, like the reference, in the order of `kernels`.

    The unreduced branch (`settings.reduce_kernelvectors` false; src/rounding.jl:967-971, 1017-1050): the vectors become the first s columns of B,
    `B = [V | E]` with the standard basis vectors E of `complete_basis`, `Binv = inverse_qq(B)`, and, with `settings.normalize_transformation`, row i of
    Binv multiplied by the least common multiple of its denominators and column i of B divided by it (src/rounding.jl:844-850).  A block without kernel
    vectors gives identities and s = 0.  The completion is tested against the inverse: an e_i that was not taken must lie in the span of V and the e_j taken
    before it, i.e. column i of Binv is zero in the rows of the e_j taken with j > i; otherwise the prime of `complete_basis` divided a deciding minor and
    the next prime is taken (at most `maxprimes` times, then `ArithmeticError`).

    The reduced branch (`settings.reduce_kernelvectors` true, the default as in the reference, AND `reduce=` given, e.g. `reduce=reduce_kernel_vectors`;
    src/rounding.jl:860-1104): blocks with s = 0 or s = N give identities; for the others the unreduced `[V | E]` and its inverse
    give the integer matrix M whose kernel is the saturated lattice of the vectors, ONE call `reduce(blocks, settings, device=..., matmul=...)` for all
    blocks returns the matrices U, and with `settings.unimodular_transform` `B = U^T`, `Binv = inverse_qq(B)`, an integer matrix (`ArithmeticError` if
    not); without it the first s rows of U replace the vectors and the unreduced branch runs on them.  `verbose`: prints the largest entry of B after the
    reduction, as the reference does.  With `settings.reduce_kernelvectors` true and `reduce=None` this raises `NotImplementedError`: pass `reduce=`, or
    `RoundingSettings(reduce_kernelvectors=False)`.
    `batch` goes to `complete_basis`; `lift`, `check`, `reconstruct`, `matmul` go to `inverse_qq`.

    Over a number field: when the vectors hold coefficient tuples (`vectors_to_field`) and `field` is a `NumberField` of degree
    at least 2, the unreduced branch runs over QQ(g): `B = [V | E]` with E from `complete_basis_field` (`batch`, `primes`), `Binv =
    inverse_field(B, field, adjugate=adjugate, primes=primes, matmul=matmul, check=check).inverse`, the completion tested against the inverse in the same
    way (the next (prime, root) pair on failure), and no normalisation (the reference normalises at degree 1 only, src/rounding.jl:844).  The matrices
    returned are object arrays of coefficient tuples.  The reduction of kernel vectors over number fields is not built: with
    `settings.reduce_kernelvectors` true this raises `NotImplementedError`.  Without `field` tuples are refused as before."""
    settings = RoundingSettings() if settings is None else settings
    if any(isinstance(x, tuple) for _, vectors in kernels.values() for v in vectors for x in v):
        if field is not None and getattr(field, "degree", 1) >= 2:
            if settings.reduce_kernelvectors:
                raise NotImplementedError("basis_transformations: the reduction of kernel vectors over number fields is not built; pass "
                                          "RoundingSettings(reduce_kernelvectors=False)")
            return _basis_transformations_field(kernels, field, device, maxprimes, batch, check, matmul, adjugate, primes)
        raise NotImplementedError("basis_transformations: the kernel vectors hold coefficient tuples over a number field (vectors_to_field); the basis change "
                                  "over a field of degree above 1 -- the inverse of [V | E] over QQ(g) -- is not built yet, only the rounding of the vectors is")
    if settings.reduce_kernelvectors and reduce is None:
        raise NotImplementedError("basis_transformations: settings.reduce_kernelvectors is true, but the HNF / LLL reduction of the kernel vectors is not on "
                                  "the device yet (nor are number fields of degree above 1); pass RoundingSettings(reduce_kernelvectors=False)")
    hooks = (settings, device, maxprimes, batch, lift, check, reconstruct, matmul)
    kernels = {key: (int(N), [list(v) for v in vectors]) for key, (N, vectors) in kernels.items()}
    reduced = {}
    if settings.reduce_kernelvectors:
        keys = [key for key, (N, vectors) in kernels.items() if 0 < len(vectors) < N]
        blocks = [_kernel_block(kernels[key][0], kernels[key][1], _unreduced_basis(key, *kernels[key], *hooks)[1]) for key in keys]
        reduced = dict(zip(keys, reduce(blocks, settings, device=device, matmul=matmul))) if keys else {}
    out = {}
    for key, (N, vectors) in kernels.items():
        s = len(vectors)
        if s == 0 or (settings.reduce_kernelvectors and s == N):
            B = _object_matrix(np.zeros((N, N), dtype=object), "basis_transformations", Fraction)
            for i in range(N):
                B[i, i] = Fraction(1)
            out[key] = (B.T.copy(), B.copy(), s)
            continue
        if key in reduced and settings.unimodular_transform:
            U = np.asarray(reduced[key], dtype=object)
            B = _object_matrix(U.T, "basis_transformations", Fraction)
            Binv = np.asarray(inverse_qq(B, maxprimes=maxprimes, device=device, lift=lift, check=check, reconstruct=reconstruct, matmul=matmul))
            if any(v.denominator != 1 for v in Binv.flat):
                raise ArithmeticError(f"basis_transformations: block {key!r}: the inverse of the reduced basis change is not an integer matrix")
        else:
            if key in reduced:
                vectors = [[Fraction(int(x)) for x in row] for row in np.asarray(reduced[key], dtype=object)[:s]]
            B, Binv = _unreduced_basis(key, N, vectors, *hooks)
            if settings.normalize_transformation:
                _normalized(B, Binv)
        if verbose and key in reduced:
            print(f"    After reduction, the maximum number of the basis transformation matrix is {max(abs(v) for v in B.flat)}")          # (maximum(abs.(B)), :972)
        out[key] = (B.T.copy(), Binv.copy(), s)
    return out


# ---- the rational linear system and the driver (src/interface.jl:1354-1535, src/rounding.jl:95-179, 1284-1296, 1366-1409; clrs_zz_lowrank_system) ----
LRSYS_MAX_K = 1 << 14                # clrs_zz_lowrank_system: (most terms of a row) min(ndu, ndw) stays below this


def _lowrank_system_planes(Ud, Wd, rowptr, col_a, col_b, ndc: int, device: int = 0):
    """One call of clrs_zz_lowrank_system on digit planes: `Ud` int32 (ndu, n, T), `Wd` int32 (ndw, n, T), `rowptr` (R + 1,), the pairs `col_a`, `col_b`
    (nc,) -> `(C, info)`, C int32 (ndc, R, nc), info int32 (4,).  The counters are written before the call raises: `lowrank_system.last_info`."""
    Ud, Wd = np.ascontiguousarray(Ud, dtype=np.int32), np.ascontiguousarray(Wd, dtype=np.int32)
    rowptr, col_a, col_b = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (rowptr, col_a, col_b))
    if Ud.ndim != 3 or Wd.ndim != 3 or Ud.shape[1:] != Wd.shape[1:] or rowptr.size < 1 or col_a.size != col_b.size:
        raise ValueError(f"lowrank_system: the digits must be (ndu, n, T) and (ndw, n, T), got {Ud.shape} and {Wd.shape}")
    (ndu, n, T), ndw, R, nc = Ud.shape, Wd.shape[0], rowptr.size - 1, col_a.size
    Cd, info = np.zeros((int(ndc), R, nc), np.int32), np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.p_i32) if a.size else C_NULL_I32
    try:
        _lib.check(_lib.load().clrs_zz_lowrank_system(int(device), n, T, R, ptr(rowptr), ndu, ptr(Ud), ndw, ptr(Wd), nc, ptr(col_a), ptr(col_b), int(ndc), ptr(Cd),
                                                      info.ctypes.data_as(_lib.p_i32)))
    finally:
        lowrank_system.last_info = [int(v) for v in info]
    return Cd, info


def _pairs_of(pairs, n: int, what: str):
    """pairs (a, b) with 0 <= a <= b < n -> two int32 vectors"""
    p = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    if p.size and (p.min() < 0 or p.max() >= n or np.any(p[:, 0] > p[:, 1])):
        raise ValueError(f"{what}: every pair (a, b) needs 0 <= a <= b < {n}")
    return np.ascontiguousarray(p[:, 0], dtype=np.int32), np.ascontiguousarray(p[:, 1], dtype=np.int32)


def _row_pointer(rowptr, T: int, what: str) -> np.ndarray:
    rp = np.asarray(rowptr, dtype=np.int64).reshape(-1)
    if rp.size < 1 or rp[0] != 0 or rp[-1] != T or np.any(np.diff(rp) < 0):
        raise ValueError(f"{what}: rowptr must be non-decreasing from 0 to the number of terms {T}")
    return rp


def lowrank_system(U, W, rowptr, pairs, device: int = 0) -> np.ndarray:
    """The rows of a linear system from low-rank terms on the device, one call of clrs_zz_lowrank_system: `U`, `W` (n, T) integer
    matrices of any size (one column per term), `rowptr` (R + 1,) the terms of every row, `pairs` the (a, b), 0 <= a <= b < n, of the nc columns.  Returns the
    object array (R, nc) of the Python integers `2^(a != b) sum_{t in row i} U[a, t] W[b, t]`.  The operands cross in balanced base-2^24 digits
    (`ints_to_planes`); the result takes `ndc` digits computed from `2 (most terms of a row) max|U| max|W|`.  The counters of the call are kept in
    `lowrank_system.last_info` (`[entries that did not fit, chunks of rows, tile workgroups, 0]`).  This is the default `assemble=` of `linear_system`."""
    u, _ = _integer_operand(U, "lowrank_system")
    w, _ = _integer_operand(W, "lowrank_system")
    if u.shape != w.shape:
        raise ValueError(f"lowrank_system: U and W must have the same shape (n, T), got {u.shape} and {w.shape}")
    n, T = u.shape
    rp = _row_pointer(rowptr, T, "lowrank_system")
    col_a, col_b = _pairs_of(pairs, n, "lowrank_system")
    R, nc = rp.size - 1, col_a.size
    out = np.zeros((R, nc), dtype=object)
    if R and nc and T:
        Ud, Wd = ints_to_planes(u), ints_to_planes(w)
        rmax = int(np.diff(rp).max())
        if rmax * min(Ud.shape[0], Wd.shape[0]) >= LRSYS_MAX_K:
            raise ValueError(f"lowrank_system: (terms of a row) * (digits of the shorter operand) = {rmax * min(Ud.shape[0], Wd.shape[0])} must be below {LRSYS_MAX_K}")
        bound = 2 * rmax * max(abs(int(u.max())), abs(int(u.min()))) * max(abs(int(w.max())), abs(int(w.min())))
        ndc = max((bound.bit_length() + DIGIT_BITS + 1) // DIGIT_BITS, 1)          # 24 ndc >= bits + 2, as in zz_matmul
        if max(Ud.shape[0], Wd.shape[0], ndc) > ZZ_MAX_DIGITS:
            raise ValueError(f"lowrank_system: an operand or the result needs more than {ZZ_MAX_DIGITS} digits")
        Cd, _ = _lowrank_system_planes(Ud, Wd, rp, col_a, col_b, ndc, device=device)
        out = planes_to_ints(Cd)
    else:
        lowrank_system.last_info = [0, 0, 0, 0]
    return out


lowrank_system.last_info = None


def _fraction_array(a, shape=None) -> np.ndarray:
    """anything -> an object array of `Fraction`s (of the given shape)"""
    src = np.asarray(a, dtype=object)
    out = np.empty(src.shape, dtype=object)
    for idx in np.ndindex(*src.shape):                                                                         # (tuples: elements of a number field, kept)
        v = src[idx]
        out[idx] = tuple(Fraction(x) for x in v) if isinstance(v, tuple) else Fraction(v)
    return out if shape is None else out.reshape(shape)


@dataclasses.dataclass
class ExactLowRank:
    """`sdp.LowRankMat` over QQ: sum_k lam[k] vs[k] ws[k]^T with `lam` (rank,), `vs`, `ws` (rank, delta) object arrays of `Fraction`s."""
    lam: np.ndarray
    vs: np.ndarray
    ws: np.ndarray

    def __post_init__(self):
        self.lam, self.vs, self.ws = _fraction_array(self.lam).reshape(-1), _fraction_array(self.vs), _fraction_array(self.ws)
        if self.vs.ndim != 2 or self.vs.shape != self.ws.shape or self.lam.shape[0] != self.vs.shape[0]:
            raise ValueError("ExactLowRank should have the same number of values as vectors")

    @property
    def rank(self) -> int:
        return self.lam.shape[0]

    @property
    def delta(self) -> int:
        return self.vs.shape[1]


@dataclasses.dataclass
class ExactBlock:
    """`sdp.Block` over QQ: `entries[(r, s)][p]` is an `ExactLowRank` or a dense (n, n) object array of `Fraction`s (then m == 1)."""
    m: int
    delta: int
    entries: dict
    name: object = None

    @property
    def n(self) -> int:
        return self.m * self.delta

    @property
    def high_rank(self) -> bool:
        return any(not isinstance(e, ExactLowRank) for d in self.entries.values() for e in d.values())


@dataclasses.dataclass
class ExactProblem:
    """`sdp.ClusteredLowRankSDP` over QQ, the problem `exact_solution` rounds to: `blocks[j][l]` are `ExactBlock`s, `B[j]` (P_j, N), `c[j]` (P_j,), `C[j][l]`
    (n, n) and `b` (N,) object arrays of `Fraction`s, `constant` a `Fraction`.  Constraint p of cluster j reads
    `sum_l <A_l^p, Y_l> + (B[j] y)[p] = c[j][p]`, the objective `constant + sum <C[j][l], Y_l> + b . y`."""
    maximize: bool
    constant: Fraction
    blocks: list
    B: list
    c: list
    C: list
    b: np.ndarray
    names: dict = dataclasses.field(default_factory=dict)
    field: object = None          # a `NumberField`: every number may then be a tuple of `degree` `Fraction`s, the coefficients in g (object arrays whose ELEMENTS are tuples: `field_array`)

    def __post_init__(self):
        self.constant = _fraction_array([self.constant] if not isinstance(self.constant, tuple) else field_array([self.constant]))[0]
        self.b = _fraction_array(self.b).reshape(-1)
        self.c = [_fraction_array(x).reshape(-1) for x in self.c]
        self.B = [_fraction_array(x, (len(cj), self.b.size)) for x, cj in zip(self.B, self.c)]
        self.C = [[_fraction_array(x) for x in cl] for cl in self.C]

    def flat_blocks(self):
        """[(cluster j, block)] in flat block order"""
        return [(j, bl) for j, cl in enumerate(self.blocks) for bl in cl]

    @property
    def block_n(self) -> np.ndarray:
        return np.array([bl.n for _, bl in self.flat_blocks()], dtype=np.int32)

    def to_sdp(self, prec: int = 256):
        """The numeric problem: every `Fraction` as the quotient of two mpmath integers at `prec` bits, in a `ClusteredLowRankSDP` of the same structure."""
        import mpmath as mp
        from .sdp import Block, ClusteredLowRankSDP, HiLo, LowRankMat

        def num(a):
            src = np.asarray(a, dtype=object)
            if src.size == 0:
                return np.zeros(src.shape)
            out = np.empty(src.shape, dtype=object)
            q = lambda v: mp.mpf(v.numerator) / mp.mpf(v.denominator)
            gp = self.field.power_values(prec=int(prec)) if self.field is not None else None
            for idx in np.ndindex(*src.shape):                       # a field element is embedded at field.g
                v = src[idx]
                out[idx] = mp.fsum(q(c) * g for c, g in zip(v, gp) if c) if isinstance(v, tuple) else q(v)
            return out

        with mp.workprec(int(prec)):
            ent = lambda e: LowRankMat(num(e.lam), num(e.vs), num(e.ws)) if isinstance(e, ExactLowRank) else HiLo.of(num(e))
            blocks = [[Block(bl.m, bl.delta, {rs: {p: ent(e) for p, e in d.items()} for rs, d in bl.entries.items()}, bl.name) for bl in cl] for cl in self.blocks]
            return ClusteredLowRankSDP(bool(self.maximize), float(num([self.constant])[0]), blocks, [num(x) for x in self.B], [num(x) for x in self.c],
                                       [[num(x) for x in cl] for cl in self.C], num(self.b), self.names)


@dataclasses.dataclass
class ExactSolution:
    """What `exact_solution` returns: `Y` the blocks (object arrays of `Fraction`s; untransformed unless `transformed`), `y` the free variables, `objective`,
    `correct_slacks` of the projection, `certificates` (one `PDCertificate` per block that kept a dimension), `Bs` of `basis_transformations`, and
    `success = correct_slacks and every certificate positive`."""
    success: bool
    Y: list
    y: list
    objective: Fraction
    correct_slacks: bool
    certificates: list
    Bs: dict


def _kept_rows(problem, Bs, d=None):
    """per block in flat order: (P, n') with P = Binv[s:, :] ((n', N) `Fraction`s, or coefficient tuples of `d` of them; None: the identity)"""
    out = []
    for bi, (_, bl) in enumerate(problem.flat_blocks()):
        if Bs is not None and bi in Bs:
            _, Binv, s = Bs[bi]
            P = (_object_matrix(Binv, "linear_system", Fraction) if d is None else _field_matrix(Binv, d, "linear_system"))[int(s):, :]
            if P.shape[1] != bl.n:
                raise ValueError(f"linear_system: the transformation of block {bi} has {P.shape[1]} columns for a block of size {bl.n}")
            out.append((P, P.shape[0]))
        else:
            out.append((None, bl.n))
    return out


def system_index(problem, Bs=None, field=None) -> list:
    """The columns of `linear_system`: `(block, a, b)`, a <= b row-major, block by block in flat order (blocks whose transformation keeps no dimension give
    none), then `("free", k)`."""
    d = None if field is None else len(_minpoly_of(field)) - 1
    index = [(bi, a, b) for bi, (_, nk) in enumerate(_kept_rows(problem, Bs, d)) for a in range(nk) for b in range(a, nk)]
    return index + [("free", k) for k in range(problem.b.size)]


def _lcm_of(values) -> int:
    from math import gcd
    l = 1
    for v in values:
        l = l * v.denominator // gcd(l, v.denominator)
    return l


def linear_system(problem, Bs=None, columns=None, assemble=None, matmul=None, device: int = 0, field=None):
    """The reference's `linearsystem` / `partial_linearsystem` (src/interface.jl:1354-1535) over QQ for an `ExactProblem`: `(A, b, index)` with
    `A x = b` the constraints in the variables x = (entries (a <= b) of the blocks, free variables).  Rows: cluster by cluster, constraint by constraint;
    columns: `system_index(problem, Bs)`, or its entries `columns` (indices into it) in the given order; `b` the concatenated `c[j]`.  `A` is an object array
    of `Fraction`s, `b` a list of `Fraction`s: what `project_to_affine_space(A, b)` takes as it is.  With `Bs` from `basis_transformations` (keys: flat block
    indices) block l is transformed, `A_l -> P_l A_l P_l^T` with `P_l = Binv_l[s_l:, :]` (src/rounding.jl:1182-1196).

    A low-rank block takes ONE call `assemble(U, W, rowptr, pairs, device=...)` (default `lowrank_system`, on the device): a term of sub-block (r, s) places
    `lam v` at rows r delta ... and `w` at rows s delta ... of a column of length n; the columns of the terms of a constraint are multiplied by the least
    common multiple of their denominators, P_l by that of its own, `U = P_l [lam v]`, `W = P_l [w]` as integer products (`matmul(A, B, device=...)`, e.g.
    `zz_matmul`; default: Python integers), and entry (i, (a, b)) is `assemble`'s integer over the product of the four multipliers.  Clearing denominators is
    host work of the size of the vectors; the quotient per entry is the only host work of the size of A.  The transposed partners `ClusteredLowRankSDP.check`
    demands make the sum over the terms symmetric, which the factor 2 off the diagonal relies on.  Dense entries go through `transform`.

    With `field` (a `NumberField` or its minimal polynomial; `Bs` then from `basis_transformations(field=...)`) the numbers of the problem may be coefficient
    tuples and `A`, `b` hold tuples (`_linear_system_field`): still one `assemble` call per low-rank block, on the coefficient planes stacked along the terms."""
    assemble = lowrank_system if assemble is None else assemble
    if field is not None:
        return _linear_system_field(problem, Bs, columns, assemble, matmul, device, field)
    kept = _kept_rows(problem, Bs)
    index = system_index(problem, Bs)
    take = list(range(len(index))) if columns is None else [int(c) for c in columns]
    if any(not 0 <= c < len(index) for c in take):
        raise ValueError(f"linear_system: a column outside [0, {len(index)})")
    where = {}
    for pos, c in enumerate(take):
        where.setdefault(c, []).append(pos)
    sizes = [len(cj) for cj in problem.c]
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    A = np.empty((int(row0[-1]), len(take)), dtype=object)
    A.fill(Fraction(0))
    first = {}                                               # block -> its first column in `index`
    for ci, e in enumerate(index):
        first.setdefault(e[0], ci)
    for bi, (j, bl) in enumerate(problem.flat_blocks()):
        P, nk = kept[bi]
        cols = [(a, b) for a in range(nk) for b in range(a, nk)]
        sel = [(t, ab) for t, ab in enumerate(cols) if first.get(bi, 0) + t in where] if nk else []
        if not sel:
            continue
        Pj, n, delta = sizes[j], bl.n, bl.delta
        if bl.high_rank:
            for p, M in bl.entries.get((0, 0), {}).items():
                Mt = _object_matrix(M, "linear_system", Fraction) if P is None else transform(M, Bs[bi][1], Bs[bi][2], matmul=matmul, device=device)
                for t, (a, b) in sel:
                    v = Mt[a, b] if a == b else Mt[a, b] + Mt[b, a]
                    for pos in where[first[bi] + t]:
                        A[row0[j] + p, pos] = v
            continue
        terms = [[] for _ in range(Pj)]                         # per constraint: (r, s, lam, v, w) in the order of `flatten`
        for (r, s), d in bl.entries.items():
            for p, e in d.items():
                for k in range(e.rank):
                    terms[p].append((r, s, k, e))
        rowptr, Vc, Wc, mult = [0], [], [], []
        for p in range(Pj):
            terms[p].sort(key=lambda t: t[:3])
            vcols, wcols = [], []
            for r, s, k, e in terms[p]:
                v, w = [Fraction(0)] * n, [Fraction(0)] * n
                v[r * delta:(r + 1) * delta] = [e.lam[k] * x for x in e.vs[k]]
                w[s * delta:(s + 1) * delta] = list(e.ws[k])
                vcols.append(v); wcols.append(w)
            lv, lw = _lcm_of(x for col in vcols for x in col), _lcm_of(x for col in wcols for x in col)
            Vc += [[int(x * lv) for x in col] for col in vcols]
            Wc += [[int(x * lw) for x in col] for col in wcols]
            mult.append(lv * lw)
            rowptr.append(len(Vc))
        T = len(Vc)
        Vi = np.array(Vc, dtype=object).reshape(T, n).T         # (n, T) integers
        Wi = np.array(Wc, dtype=object).reshape(T, n).T
        lp = 1
        if P is not None and T:
            Pn, lp = _common_denominator(P.flat)
            Pn = Pn.reshape(P.shape)
            Vi = _matmul_matrix(matmul, Pn, Vi, device) if matmul is not None else Pn.dot(Vi)
            Wi = _matmul_matrix(matmul, Pn, Wi, device) if matmul is not None else Pn.dot(Wi)
        G = np.asarray(assemble(Vi, Wi, rowptr, [ab for _, ab in sel], device=device), dtype=object)
        if G.shape != (Pj, len(sel)):
            raise ArithmeticError(f"linear_system: assemble returned shape {G.shape} for {Pj} rows and {len(sel)} columns")
        for p in range(Pj):
            den = lp * lp * mult[p]
            for q, (t, _) in enumerate(sel):
                g = int(G[p, q])
                if g:
                    v = Fraction(g, den)
                    for pos in where[first[bi] + t]:
                        A[row0[j] + p, pos] = v
    nY = len(index) - problem.b.size
    for k in range(problem.b.size):
        for pos in where.get(nY + k, ()):
            for j in range(len(sizes)):
                A[row0[j]:row0[j + 1], pos] = problem.B[j][:, k]
    b = [Fraction(v) for cj in problem.c for v in cj]
    return A, b, [index[c] for c in take]


def _objective_marks(problem, Bs, matmul, device):
    """per column of `system_index(problem, Bs)`: does the (transformed) objective touch it?"""
    marks = []
    for bi, ((j, bl), (P, nk)) in enumerate(zip(problem.flat_blocks(), _kept_rows(problem, Bs))):
        if not nk:
            continue
        l = bi - sum(len(cl) for cl in problem.blocks[:j])
        Ct = problem.C[j][l] if P is None else transform(problem.C[j][l], Bs[bi][1], Bs[bi][2], matmul=matmul, device=device)
        marks += [Ct[a, b] != 0 or Ct[b, a] != 0 for a in range(nk) for b in range(a, nk)]
    return marks + [v != 0 for v in problem.b]


def select_columns(problem_or_index, redundancyfactor: int = 10, rng=None, nconstraints: Optional[int] = None, objective=None, Bs=None) -> list:
    """The reference's `select_columns` (src/rounding.jl:95-153): the columns of the system the projection works with.  `problem_or_index`: an `ExactProblem`
    (its index with `Bs`, its number of constraints and its objective are used) or the index of `linear_system` with `nconstraints` and, optionally,
    `objective` (per column: is it in the objective?).  Entries on the diagonal and next to it get the mark 1, columns of the objective +2.  A negative
    factor takes all columns.  Otherwise, with K = redundancyfactor * nconstraints: the columns marked >= 2 and then those marked 1 -- or, when they are more
    than K, a random K of them (`rng.permutation`, where the reference shuffles), those of the objective first -- followed by
    `max((redundancyfactor - 2) * nconstraints, K - taken)` unmarked columns at random.  `rng`: a `numpy.random.Generator` (default `default_rng(0)`).
    0-based indices."""
    rng = np.random.default_rng(0) if rng is None else rng
    if isinstance(problem_or_index, ExactProblem):
        index = system_index(problem_or_index, Bs)
        nconstraints = sum(len(cj) for cj in problem_or_index.c) if nconstraints is None else nconstraints
        objective = _objective_marks(problem_or_index, Bs, None, 0) if objective is None else objective
    else:
        index = list(problem_or_index)
        if nconstraints is None:
            raise ValueError("select_columns: an index needs nconstraints")
    redundancyfactor, nconstraints = int(redundancyfactor), int(nconstraints)
    if redundancyfactor < 0:
        return list(range(len(index)))
    objective = [False] * len(index) if objective is None else [bool(v) for v in objective]
    if len(objective) != len(index):
        raise ValueError(f"select_columns: objective has {len(objective)} entries for {len(index)} columns")
    marks = [(1 if e[0] != "free" and e[2] - e[1] <= 1 else 0) + (2 if o else 0) for e, o in zip(index, objective)]
    obj_cols = [i for i, v in enumerate(marks) if v >= 2]
    chosen = [i for i, v in enumerate(marks) if v == 1]
    K = redundancyfactor * nconstraints
    if len(obj_cols) + len(chosen) > K:
        both = obj_cols + chosen
        cut = [both[t] for t in rng.permutation(len(both))][:K]
        in_obj = set(obj_cols)
        pivot_cols = list(dict.fromkeys([i for i in cut if i in in_obj] + cut))
    else:
        pivot_cols = obj_cols + chosen
    needed = max((redundancyfactor - 2) * nconstraints, K - len(pivot_cols), 0)
    rest = [i for i, v in enumerate(marks) if v == 0]
    rest = [rest[t] for t in rng.permutation(len(rest))]
    return pivot_cols + rest[:min(needed, len(rest))]


def vectorize_solution(Yt, y, index) -> list:
    """the vector x of `linear_system` for the blocks `Yt` (a list in flat block order, or a dict by block) and the free variables `y`"""
    return [Fraction(y[e[1]]) if e[0] == "free" else Fraction(Yt[e[0]][e[1], e[2]]) for e in index]


def get_rational_system(problem, Yt, y, Bs=None, columns=None, settings: Optional[RoundingSettings] = None, assemble=None, matmul=None, device: int = 0,
                        field=None, limbs: Optional[int] = None, form: str = "auto", gemm=None, solve=None):
    """The reference's `get_rational_system` over QQ (src/rounding.jl:1284-1296): `(A_cols, rhs, x_rounded, columns)`.  x = the entries (a <= b) of the
    transformed blocks `Yt` and the free variables `y` (exact rationals) in the order of `system_index(problem, Bs)`;
    `x_rounded = floor(x 10^dec) / 10^dec` entry by entry with `dec = settings.approximation_decimals` (`roundx`, src/rounding.jl:515-517);
    `rhs = b - A x_rounded` over ALL columns of the transformed system (with `matmul`: one integer product of the rows cleared of denominators), and
    `A_cols` its columns `columns` (default: all).  The full triangle is assembled once (`linear_system`).

    With `field` (src/rounding.jl:1299-1330; `Yt`, `y` numeric: mpmath numbers): the full system over the field, `convert_system`, `field_least_squares` at
    `limbs` limbs (`form`, `gemm`, `solve` as there) for `x_rounded` (m d numbers), `rhs = btot - Atot x_rounded`, and the columns `[c + m k]`, k < d, of
    every column c."""
    settings = RoundingSettings() if settings is None else settings
    if field is not None:
        A, b, index = linear_system(problem, Bs=Bs, assemble=assemble, matmul=matmul, device=device, field=field)
        Atot, btot = convert_system(A, b, field)
        d, m = field.degree, len(index)
        x = [y[e[1]] if e[0] == "free" else Yt[e[0]][e[1], e[2]] for e in index]
        x_rounded = field_least_squares(Atot, btot, x, field, limbs, settings.regularization, settings.approximation_decimals, form=form, gemm=gemm, solve=solve,
                                        device=device)
        nrows, ncols = Atot.shape
        if matmul is not None and nrows and ncols:
            cleared = [_common_denominator(list(Atot[i])) for i in range(nrows)]
            Ai = np.array([list(cl[0]) for cl in cleared], dtype=object).reshape(nrows, ncols)
            xv, L = _common_denominator(x_rounded)
            rhs = [btot[i] - Fraction(v, L * cleared[i][1]) for i, v in enumerate(_matmul_vector(matmul, Ai, xv, device))]
        else:
            rhs = [btot[i] - sum((Atot[i, c] * x_rounded[c] for c in range(ncols) if Atot[i, c] != 0), Fraction(0)) for i in range(nrows)]
        columns = list(range(m)) if columns is None else [int(c) for c in columns]
        columns = [c + m * k for c in columns for k in range(d)]
        return Atot[:, columns], rhs, x_rounded, columns
    A, b, index = linear_system(problem, Bs=Bs, assemble=assemble, matmul=matmul, device=device)
    scale = 10 ** int(settings.approximation_decimals)
    x_rounded = [Fraction((v * scale).__floor__(), scale) for v in vectorize_solution(Yt, y, index)]
    nrows, ncols = A.shape
    if matmul is not None and nrows and ncols:
        cleared = [_common_denominator(list(A[i])) for i in range(nrows)]
        Ai = np.array([list(cl[0]) for cl in cleared], dtype=object).reshape(nrows, ncols)
        xv, L = _common_denominator(x_rounded)
        rhs = [b[i] - Fraction(v, L * cleared[i][1]) for i, v in enumerate(_matmul_vector(matmul, Ai, xv, device))]
    else:
        rhs = [b[i] - sum((A[i, c] * x_rounded[c] for c in range(ncols) if A[i, c] != 0), Fraction(0)) for i in range(nrows)]
    columns = list(range(ncols)) if columns is None else [int(c) for c in columns]
    return A[:, columns], rhs, x_rounded, columns


def _exact_blocks(result_Y, block_n, limbs=None):
    """the blocks of a solution (fp64 (len,) or planar limbs (planes, len), column-major per block) as symmetric matrices of exact dyadic `Fraction`s"""
    a = np.asarray(result_Y, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if limbs is not None:
        a = a[:int(limbs)]
    off = np.concatenate([[0], np.cumsum(np.asarray(block_n, dtype=np.int64) ** 2)])
    if a.shape[1] != off[-1]:
        raise ValueError(f"exact_solution: the solution holds {a.shape[1]} numbers per plane for blocks of {int(off[-1])} entries")
    out = []
    for bi, n in enumerate(int(v) for v in block_n):
        vals = [sum((Fraction(float(a[l, o])) for l in range(a.shape[0]) if a[l, o] != 0.0), Fraction(0)) for o in range(off[bi], off[bi + 1])]
        M = np.array(vals, dtype=object).reshape(n, n).T if n else np.zeros((0, 0), dtype=object)
        out.append(_object_matrix((M + M.T) / 2 if n else M, "exact_solution", Fraction))
    return out


def _lift_by_columns(lift):
    """the `lift` hook of `solve_dixon` (one right-hand side) as the `lift` hook of `solve_dixon_multi`: column by column"""
    def multi(A, B, p, steps, device=0):
        B = np.asarray(B, dtype=object)
        cols = [lift(A, B[:, j], p, steps, device=device) for j in range(B.shape[1])]
        if cols[0][0] is None:
            return None, None, cols[0][2]
        R = np.zeros(B.shape, dtype=object)
        for j, c in enumerate(cols):
            R[:, j] = [int(v) for v in c[1]]
        return np.ascontiguousarray(np.stack([np.asarray(c[0]) for c in cols], axis=2)), R, cols[0][2]
    return multi


def exact_solution(problem, result, settings: Optional[RoundingSettings] = None, limbs: Optional[int] = None, transformed: bool = False, rng=None,
                   device: int = 0, batch=None, lift=None, reconstruct=None, matmul=None, minors=None, round_batch=None, assemble=None, reduce=None, verbose: bool = False,
                   field=None, gemm=None, solve=None, adjugate=None, primes=None) -> ExactSolution:
    """The reference's `exact_solution` over QQ (src/rounding.jl:1366-1409, 155-179) for an `ExactProblem` and a numeric solution `result` of
    `problem.to_sdp(...)` (a `SolveResult` of `solvesdp_mw`, or anything with `X`, `Y` (fp64 or planar limbs) and `y`):

      1. `kernel_vectors(..., rationalize=True)`;  2. `basis_transformations`;  3. the blocks Y as the exact dyadic rationals their limbs sum to,
      `Yt = B^T[s:, :] Y B[:, s:]`;  4. the loop of the reference's `project_to_affine_space(problem, sol)`: `select_columns` with
      `settings.redundancyfactor + extra`, `get_rational_system`, `project_to_affine_space(A, b)`; an inconsistent system takes `extra += 2`, and is an
      `ArithmeticError` when all columns were already taken;  5. the positive-definiteness part of `is_valid_solution(..., check_slacks=False)`: `checkpd`
      of every transformed block, the certificates kept;  6. `undo_transform`, unless `transformed`.

    With the default `settings.reduce_kernelvectors` and `reduce=None` `basis_transformations` raises its `NotImplementedError`, which passes through;
    `reduce=reduce_kernel_vectors` (or a stand-in) takes the reference's reduced, unimodular basis change (`verbose` goes there too).  The hooks replace the
    device calls of the steps: `round_batch` (`kernel_vectors`), `batch` (`rref_mod_p`), `lift` (the one-column hook of `solve_dixon`; the inverse of
    `basis_transformations` then takes it column by column), `reconstruct`, `matmul`, `minors` (`checkpd`), `assemble` (`linear_system`).  `rng`: the generator of `select_columns` and `project_to_affine_space`."""
    settings = RoundingSettings() if settings is None else settings
    rng = np.random.default_rng(0) if rng is None else rng
    if field is not None:
        return _exact_solution_field(problem, result, settings, limbs, transformed, rng, device, batch, lift, reconstruct, matmul, minors, round_batch, assemble,
                                     field, gemm, solve, adjugate, primes)
    block_n = problem.block_n
    kernels = kernel_vectors(block_n, result, result, limbs=limbs, settings=settings, device=device, rationalize=True, round_batch=round_batch)
    Bs = basis_transformations({bi: (int(n), vectors_to_fractions(k)) for bi, (n, k) in enumerate(zip(block_n, kernels))}, settings, device=device, batch=batch,
                               lift=None if lift is None else _lift_by_columns(lift), reconstruct=reconstruct, matmul=matmul, reduce=reduce, verbose=verbose)
    Y = _exact_blocks(result.Y, block_n, limbs)
    y = [sum((Fraction(float(v)) for v in np.atleast_2d(np.asarray(getattr(result, "y", np.zeros(0)), dtype=np.float64))[:, k]), Fraction(0))
         for k in range(problem.b.size)]
    Yt = {bi: transform(Y[bi], Bs[bi][0], Bs[bi][2], matmul=matmul, device=device) for bi in Bs}
    index = system_index(problem, Bs)
    nconstraints = sum(len(cj) for cj in problem.c)
    objective = _objective_marks(problem, Bs, matmul, device)
    extra = 0
    while True:
        columns = select_columns(index, settings.redundancyfactor + extra, rng, nconstraints=nconstraints, objective=objective)
        A, rhs, x, columns = get_rational_system(problem, Yt, y, Bs, columns, settings, assemble=assemble, matmul=matmul, device=device)
        x_extra, correct_slacks, finished = project_to_affine_space(A, rhs, settings=settings, rng=rng, device=device, batch=batch, lift=lift,
                                                                    reconstruct=reconstruct, matmul=matmul)
        if finished:
            break
        if len(columns) >= len(index):
            raise ArithmeticError("exact_solution: the system is inconsistent but all columns were taken")
        extra += 2
    for pos, c in enumerate(columns):
        x[c] += x_extra[pos]
    sol_t, free = {}, [Fraction(0)] * problem.b.size
    for bi, (_, _, s) in Bs.items():
        nk = int(block_n[bi]) - int(s)
        sol_t[bi] = _object_matrix(np.zeros((nk, nk), dtype=object), "exact_solution", Fraction)
    for e, v in zip(index, x):
        if e[0] == "free":
            free[e[1]] = v
        else:
            sol_t[e[0]][e[1], e[2]] = sol_t[e[0]][e[2], e[1]] = v
    certificates = [checkpd(sol_t[bi], device=device, minors=minors) for bi in sol_t if sol_t[bi].shape[0]]
    success = bool(correct_slacks) and all(cert.pd for cert in certificates)
    full = [undo_transform(sol_t[bi], Bs[bi][1], Bs[bi][2], matmul=matmul, device=device) for bi in sorted(sol_t)]
    objective_value = problem.constant + sum((v * free[k] for k, v in enumerate(problem.b)), Fraction(0))
    for (j, l), M in zip(((j, l) for j, cl in enumerate(problem.blocks) for l in range(len(cl))), full):
        objective_value += sum((problem.C[j][l][a, b] * M[a, b] for a in range(M.shape[0]) for b in range(M.shape[0]) if M[a, b] != 0), Fraction(0))
    return ExactSolution(success, [sol_t[bi] for bi in sorted(sol_t)] if transformed else full, free, objective_value, bool(correct_slacks), certificates, Bs)


# ---- rounding to a number field of degree above 1: integer relations (src/rounding.jl:481-534, 623-628; clrs_mw_field_round) ----------------
FIELD_KERNEL_DEGREES = (2, 3, 4)     # what k_mw_field_round is instantiated for
FIELD_LLL_MAX_DEGREE = 8             # `field_relations_lll` goes further, through clrs_zz_lll
FIELD_FOUND, FIELD_EXHAUSTED, FIELD_NOT_FINITE, FIELD_STEER, FIELD_OVERFLOW, FIELD_NO_FIELD = range(6)


def field_top_bits(bits: int, limbs: int) -> int:
    """the top rung of the ladder 1, 6, 11, ..: min(bits, 53 limbs - 16) rounded down onto it"""
    return 1 + 5 * ((min(int(bits), 53 * int(limbs) - 16) - 1) // 5)


class NumberField:
    """QQ(g): `minpoly` the integer coefficients of a polynomial with root g, low to high; `g` an mpmath number (taken at `prec` bits, default the current
    mpmath precision) or its limbs (a 1-d fp64 array, `prec` = 53 per limb).  Refuses a `g` with |minpoly(g)| above 2^(8 - prec) sum_k |c_k| |g|^k."""

    def __init__(self, minpoly, g, prec: Optional[int] = None):
        import mpmath as mp
        self.minpoly = [int(c) for c in minpoly]
        if len(self.minpoly) < 2 or self.minpoly[-1] == 0 or any(int(c) != c for c in minpoly):
            raise ValueError("NumberField: minpoly must hold the integer coefficients of a polynomial of degree >= 1, low to high")
        if isinstance(g, (np.ndarray, list, tuple)):
            limbs = np.asarray(g, dtype=np.float64).reshape(-1)
            self.prec = 53 * limbs.size if prec is None else int(prec)
            with mp.workprec(64 * limbs.size + 1200):
                self.g = mp.fsum(mp.mpf(float(x)) for x in limbs)
        else:
            self.prec = int(mp.mp.prec if prec is None else prec)
            self.g = mp.mpf(g)
        if self.residual() > mp.ldexp(1, 8 - self.prec):
            raise ValueError(f"NumberField: |minpoly(g)| is {mp.nstr(self.residual(), 3)} of its terms, not below 2^{8 - self.prec}: g is no root at {self.prec} bits")

    @property
    def degree(self) -> int:
        return len(self.minpoly) - 1

    def residual(self):
        """|minpoly(g)| / sum_k |c_k| |g|^k"""
        import mpmath as mp
        with mp.workprec(self.prec + 64):
            terms = [c * self.g ** k for k, c in enumerate(self.minpoly)]
            return abs(mp.fsum(terms)) / mp.fsum(abs(t) for t in terms)

    def power_values(self, count: Optional[int] = None, prec: Optional[int] = None):
        import mpmath as mp
        with mp.workprec((self.prec if prec is None else prec) + 64):
            return [self.g ** k for k in range(self.degree if count is None else count)]

    def powers(self, limbs: int) -> np.ndarray:
        """g^0 .. g^(degree - 1) as planar limbs (limbs, degree), what clrs_mw_field_round takes; refuses a g not known to the 53 limbs - 16 bits of the ladder"""
        import mpmath as mp
        from .mw import to_limbs
        need = 53 * int(limbs) - 16
        if self.prec < need or self.residual() > mp.ldexp(1, 8 - need):
            raise ValueError(f"NumberField.powers: g is a root to {self.prec} bits, {limbs} limbs need {need}")
        return np.ascontiguousarray(to_limbs(self.power_values(prec=64 * int(limbs) + 64), int(limbs)))


@dataclasses.dataclass
class FieldRounding:
    """What `round_to_field` returns.  `coeffs` (count, deg) object: x_k = -a_{k+1} / a_0 as `Fraction`s where `status` is 0, else None; `rel` (count, deg + 1)
    Python integers, the relation a (zeros unless status is 0 or 5); `status` (count,): 0 found, 1 ladder exhausted, 2 not finite, 3 steering failed or a cap
    was hit, 4 an entry left its digits, 5 a_0 = 0; `rung`: the bits of the rung a number ended at; `err`: |sum a_i u_i| there; `vq` planar (limbs, count): the
    element in limbs; `exchanges`, `rungs` (count,): the counters of the kernel; `path` (count,): 0 the kernel, 1 `field_relations_lll`."""
    coeffs: np.ndarray
    rel: np.ndarray
    status: np.ndarray
    rung: np.ndarray
    err: np.ndarray
    vq: np.ndarray
    exchanges: np.ndarray
    rungs: np.ndarray
    path: np.ndarray


def _field_round_call_device(limbs, deg, gpow, count, v, plane, bits, errbound, nd, device=0):
    """one call of clrs_mw_field_round: returns (rel (nd, deg + 1, plane) int32, status, rung, err, vq (limbs, plane), info (2, plane))"""
    D = deg + 1
    rel, status, rung = np.zeros((nd, D, max(plane, 1)), np.int32), np.zeros(max(plane, 1), np.int32), np.zeros(max(plane, 1), np.int32)
    err, vq, info = np.zeros(max(plane, 1)), np.zeros((limbs, max(plane, 1))), np.zeros((2, max(plane, 1)), np.int32)
    pi, pd = (lambda a: a.ctypes.data_as(_lib.p_i32)), (lambda a: a.ctypes.data_as(_lib.p_d))
    _lib.check(_lib.load().clrs_mw_field_round(int(device), int(limbs), int(deg), pd(gpow), int(count), pd(v), int(plane), int(bits), float(errbound), int(nd),
                                               pi(rel), pi(status), pi(rung), pd(err), pd(vq), pi(info)))
    return rel, status, rung, err, vq, info


def _field_values(values, limbs, what):
    a = np.asarray(values, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] > limbs:
        raise ValueError(f"{what}: values must be fp64 (count,) or planar (planes <= {limbs}, count), got {a.shape}")
    v = np.zeros((limbs, max(a.shape[1], 1)))
    v[:a.shape[0], :a.shape[1]] = a
    return v, a.shape[1]


def _field_coeffs(rel, status):
    coeffs = np.empty((rel.shape[0], rel.shape[1] - 1), dtype=object)
    for i in range(rel.shape[0]):
        for k in range(rel.shape[1] - 1):
            coeffs[i, k] = Fraction(-int(rel[i, k + 1]), int(rel[i, 0])) if status[i] == FIELD_FOUND else None
    return coeffs


def field_default_digits(bits: int, limbs: int) -> int:
    """the digits per entry `round_to_field` gives the kernel: a reduced basis at p bits with one short relation has entries near p / 2 bits at worst (deg 2)"""
    return min(LLL_MAX_DIGITS, field_top_bits(bits, limbs) // (2 * DIGIT_BITS) + 3)


def _relation_ladder(us, D: int, P: int, errbound: float, lll, device):
    """The rung loop of `field_relations_lll` and `minpoly_relations_lll`: `us[i]` the D mpmath numbers of number i (None: not finite, status 2).  Per rung
    p = 1, 6, 11, .. <= P one batched `lll` call over the numbers still open, each on [I | floor(2^p u)] from scratch; the first row a is accepted when
    |sum a_k u_k| < errbound in the caller's mpmath precision.  Returns (rel (count, D) object, status, rung, err): status 0 wherever a row was accepted,
    whatever its entries; 1 ladder exhausted; 3 / 4 where `lll` raised `ReductionError`."""
    import mpmath as mp
    count = len(us)
    rel, status = np.zeros((count, D), dtype=object), np.full(count, -1, np.int32)
    rung, err = np.zeros(count, np.int32), np.zeros(count)
    for i, u in enumerate(us):
        if u is None:
            status[i] = FIELD_NOT_FINITE
    p = 1
    while p <= P and np.any(status == -1):
        opened = [i for i in range(count) if status[i] == -1]
        lattices = []
        for i in opened:
            A = np.zeros((D, D + 1), dtype=object)
            for r in range(D):
                A[r, r], A[r, D] = 1, int(mp.floor(mp.ldexp(us[i][r], p)))
            lattices.append(A)
        try:
            outs = lll(lattices, device=device)
        except ReductionError:
            outs = []
            for A in lattices:                                             # (one lattice failed: find out which)
                try:
                    outs.append(lll([A], device=device)[0])
                except ReductionError as e:
                    outs.append(FIELD_OVERFLOW if "digits" in str(e) else FIELD_STEER)
        for i, out in zip(opened, outs):
            rung[i] = p
            if isinstance(out, int):
                status[i] = out
                continue
            a = [int(x) for x in out[0, :D]]
            e = abs(mp.fsum(x * u for x, u in zip(a, us[i])))
            err[i] = float(e)
            if e < errbound:
                rel[i] = a
                status[i] = FIELD_FOUND
        p += 5
    status[status == -1] = FIELD_EXHAUSTED
    return rel, status, rung, err


def field_relations_lll(values, field: NumberField, limbs: int, errbound: float = 1e-15, bits: int = 1000, device: int = 0, lll=None) -> FieldRounding:
    """The contract of `round_to_field` through `lll_batch` (clrs_zz_lll): per rung p = 1, 6, 11, .. one batched call over the numbers still open, each on
    the lattice [I | floor(2^p u)] from scratch; the first row is accepted on the host, in mpmath, when |sum a_i u_i| < errbound.  Degrees 2 .. 8; limited
    by the 20 digits of `lll_batch` (status 4 where a lattice leaves them, 3 where it could not be reduced).  The rescue of `round_to_field` for statuses 3
    and 4, its path for degrees 5 .. 8, and an independent device-side cross-check of k_mw_field_round.  `lll` replaces `lll_batch` (the tests' host build)."""
    import mpmath as mp
    from .mw import from_limbs, to_limbs
    limbs, deg = int(limbs), field.degree
    if limbs not in LIMBS:
        raise ValueError(f"field_relations_lll: limbs must be one of {LIMBS}, got {limbs}")
    if not 2 <= deg <= FIELD_LLL_MAX_DEGREE:
        raise ValueError(f"field_relations_lll: the degree must lie in [2, {FIELD_LLL_MAX_DEGREE}], got {deg}")
    if not errbound > 0 or bits < 1:
        raise ValueError("field_relations_lll: errbound must be positive and bits at least 1")
    lll = lll_batch if lll is None else lll
    v, count = _field_values(values, limbs, "field_relations_lll")
    D, P = deg + 1, field_top_bits(bits, limbs)
    field.powers(limbs)                                                         # (refuses a g not known to the ladder's bits)
    vqs = [mp.mpf(0)] * count
    with mp.workprec(64 * limbs + 128):
        gp = [mp.mpf(x) for x in from_limbs(field.powers(limbs))]
        finite = np.all(np.isfinite(v[:, :count]), axis=0)
        us = [[x] + gp if finite[i] else None for i, x in enumerate(from_limbs(v[:, :count]))]
        rel, status, rung, err = _relation_ladder(us, D, P, errbound, lll, device)
        for i in np.flatnonzero(status == FIELD_FOUND):
            a = rel[i]
            if a[0] == 0:
                status[i] = FIELD_NO_FIELD
            else:
                vqs[i] = -mp.fsum(x * u for x, u in zip(a[1:], gp)) / a[0]
        vq = to_limbs(vqs, limbs) if count else np.zeros((limbs, 0))
    zeros = np.zeros(count, np.int32)
    return FieldRounding(_field_coeffs(rel, status), rel, status, rung, err, vq, zeros, zeros.copy(), np.ones(count, np.int32))


def round_to_field(values, field: NumberField, limbs: int, errbound: float = 1e-15, bits: int = 1000, device: int = 0, relations=None, nd: Optional[int] = None,
                   call=None) -> FieldRounding:
    """Round numbers to QQ(g) on the device (clrs_mw_field_round, one lane per number): `values` planar (planes <= limbs, count) or fp64 (count,).  Per
    number v the first rung p = 1, 6, 11, .. <= min(bits, 53 limbs - 16) at which the first row a of the LLL-reduced basis of [I | floor(2^p (v, 1, g, ..))]
    has |a_0 v + a_1 + a_2 g + ..| < errbound, evaluated in `limbs` limbs from the numbers as given; then v ~ sum_k x_k g^k with x_k = -a_{k+1} / a_0.
    Degrees 2 .. 4 run in the kernel; numbers it ends with status 3 or 4, and every number of a field of degree 5 .. 8, go to `relations` (default
    `field_relations_lll`; False: nowhere).  `nd`: the base-2^24 digits per lattice entry (default `field_default_digits`); `call` replaces the device
    call (the tests' host build)."""
    limbs, deg = int(limbs), field.degree
    if limbs not in LIMBS:
        raise ValueError(f"round_to_field: limbs must be one of {LIMBS}, got {limbs}")
    if deg < 2:
        raise ValueError("round_to_field: a field of degree 1 is QQ: use rationalize")
    relations = field_relations_lll if relations is None else relations
    if deg not in FIELD_KERNEL_DEGREES:
        if relations is False:
            raise ValueError(f"round_to_field: the kernel takes degrees {FIELD_KERNEL_DEGREES}, got {deg}")
        return relations(values, field, limbs, errbound=errbound, bits=bits, device=device)
    v, count = _field_values(values, limbs, "round_to_field")
    nd = field_default_digits(bits, limbs) if nd is None else int(nd)
    gpow = field.powers(limbs)
    call = _field_round_call_device if call is None else call
    reld, status, rung, err, vq, info = call(limbs, deg, gpow, count, v, v.shape[1], int(bits), float(errbound), nd, device=device)
    status, rung, err, vq = status[:count].copy(), rung[:count].copy(), err[:count].copy(), vq[:, :count].copy()
    rel = planes_to_ints(reld[:, :, :count]).T.copy() if count else np.zeros((0, deg + 1), dtype=object)
    out = FieldRounding(_field_coeffs(rel, status), rel, status, rung, err, vq, info[0, :count].copy(), info[1, :count].copy(), np.zeros(count, np.int32))
    again = np.flatnonzero((status == FIELD_STEER) | (status == FIELD_OVERFLOW))
    if again.size and relations is not False:
        r = relations(v[:, again], field, limbs, errbound=errbound, bits=bits, device=device)
        out.coeffs[again], out.rel[again], out.status[again], out.rung[again], out.err[again], out.path[again] = r.coeffs, r.rel, r.status, r.rung, r.err, 1
        out.vq[:, again] = r.vq
    return out


def kernel_vectors_field_batch(block_n, X, Y, limbs: int, tau: float, use_dual: bool, dual_max: float, round_errbound: float, field: NumberField = None,
                               bits: int = 1000, device: int = 0, batch=None, round=None, gemm=None):
    """`kernel_vectors_batch`, then on the device the rounding of every entry of every vector to `field` (`round_to_field`) and the reference's second
    check Y_b Vq_b of the rounded vectors (src/rounding.jl:630-639) by the kernel of clrs_mw_gemm.  Fills `coeffs` (n, count, deg), `round_status`,
    `round_rung`, `vectors_rounded` and `round_resid_max` of every block; `num` / `den` stay None.  Without hooks this is ONE call,
    clrs_mw_kernel_vectors_field; `batch`, `round`, `gemm` replace the three device calls it is made of (and make it three calls), which is also what runs
    when an entry ends with status 3 or 4: `round_to_field` then sends it to `field_relations_lll`."""
    from .mw import gemm_batch
    if batch is None and round is None and gemm is None and field.degree in FIELD_KERNEL_DEGREES:
        out = _kernel_vectors_field_call(block_n, X, Y, int(limbs), tau, use_dual, dual_max, float(round_errbound), field, int(bits), device)
        if not any(np.any((k.round_status == FIELD_STEER) | (k.round_status == FIELD_OVERFLOW)) for k in out):
            return out                                    # (else: the composed path below, whose `round_to_field` sends such entries to `field_relations_lll`)
    batch = kernel_vectors_batch if batch is None else batch
    round = round_to_field if round is None else round
    gemm = gemm_batch if gemm is None else gemm
    out = batch(block_n, X, Y, limbs, tau, use_dual, dual_max, device=device)
    n = np.ascontiguousarray(block_n, np.int32).reshape(-1)
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)])
    sizes = [int(n[b]) * k.count for b, k in enumerate(out)]
    pool = np.concatenate([np.asarray(k.vectors).reshape(limbs, -1) for k in out], axis=1) if out else np.zeros((limbs, 0))
    r = round(pool, field, limbs, errbound=float(round_errbound), bits=int(bits), device=device)
    pos, jobs = 0, []
    for b, (k, size) in enumerate(zip(out, sizes)):
        nn, shape = int(n[b]), (int(n[b]), k.count)
        k.coeffs = r.coeffs[pos:pos + size].reshape(shape + (field.degree,))
        k.round_status, k.round_rung = r.status[pos:pos + size].reshape(shape), r.rung[pos:pos + size].reshape(shape)
        k.vectors_rounded = np.ascontiguousarray(r.vq[:, pos:pos + size].reshape((limbs,) + shape))
        k.round_resid_max = np.zeros(k.count)
        if size:
            jobs.append((b, (np.asarray(Y)[:, off[b]:off[b + 1]].reshape(limbs, nn, nn), k.vectors_rounded, None, False, False, 1, 0)))
        pos += size
    for (b, _), prod in zip(jobs, gemm([j for _, j in jobs], limbs, device=device)):
        out[b].round_resid_max = np.max(np.abs(prod[0]), axis=0)
    return out


def _kernel_vectors_field_call(block_n, X, Y, limbs, tau, use_dual, dual_max, round_errbound, field, bits, device=0, nd=None):
    """one call of clrs_mw_kernel_vectors_field: the elimination, the rounding of every entry to `field` and the second check, on the device"""
    n = np.ascontiguousarray(block_n, np.int32).reshape(-1)
    nb, deg = n.size, field.degree
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)])
    xoff = np.concatenate([[0], np.cumsum(n.astype(np.int64))])
    plane, xlen = int(off[-1]), int(xoff[-1])
    nd = field_default_digits(bits, limbs) if nd is None else int(nd)
    X, Y = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (X, Y))
    if X.shape != (limbs, plane) or Y.shape != (limbs, plane):
        raise ValueError(f"kernel_vectors_field_batch: X and Y must be planar ({limbs}, {plane}), got {X.shape} and {Y.shape}")
    p1 = max(plane, 1)
    pool = lambda: np.zeros((limbs, p1))
    Xp, Yp, V, Vq = pool(), pool(), pool(), pool()
    Xp[:, :plane], Yp[:, :plane] = X, Y
    branch, rank, count = (np.zeros(max(nb, 1), np.int32) for _ in range(3))
    perm = np.zeros(max(xlen, 1), np.int32)
    rmax, vmax, rmax2, piv = np.zeros(max(xlen, 1)), np.zeros(max(xlen, 1)), np.zeros(max(xlen, 1)), np.zeros((limbs, max(xlen, 1)))
    rel, status, rung = np.zeros((nd, deg + 1, p1), np.int32), np.zeros(p1, np.int32), np.zeros(p1, np.int32)
    err, info, gpow = np.zeros(p1), np.zeros((2, p1), np.int32), field.powers(limbs)
    pi, pd = (lambda a: a.ctypes.data_as(_lib.p_i32)), (lambda a: a.ctypes.data_as(_lib.p_d))
    _lib.check(_lib.load().clrs_mw_kernel_vectors_field(int(device), limbs, nb, pi(n), pd(Xp), pd(Yp), plane if plane else 0, float(tau), int(bool(use_dual)),
                                                        float(dual_max), float(round_errbound), deg, pd(gpow), int(bits), nd, pi(branch), pi(perm), pi(rank),
                                                        pi(count), pd(V), pd(rmax), pd(vmax), pd(piv), pi(rel), pi(status), pi(rung), pd(err), pd(Vq), pi(info),
                                                        pd(rmax2)))
    out = []
    for b in range(nb):
        nn, r, c = int(n[b]), int(rank[b]), int(count[b])
        seg = slice(int(off[b]), int(off[b]) + nn * c)
        cols = lambda a: np.ascontiguousarray(np.moveaxis(a[..., seg].reshape(a.shape[:-1] + (c, nn)), -1, -2))
        k = BlockKernel("dual" if branch[b] else "primal", r, c, perm[xoff[b]:xoff[b + 1]].copy(), cols(V), rmax[xoff[b]:xoff[b] + c].copy(),
                        vmax[xoff[b]:xoff[b] + c].copy(), piv[:, xoff[b]:xoff[b] + nn - r].copy())
        k.round_status, k.round_rung, k.vectors_rounded = cols(status), cols(rung), cols(Vq)
        ints = planes_to_ints(rel[:, :, seg]).T if nn * c else np.zeros((0, deg + 1), dtype=object)           # (entry, deg + 1), entries vector by vector
        k.coeffs = np.ascontiguousarray(np.transpose(_field_coeffs(ints, status[seg]).reshape(c, nn, deg), (1, 0, 2)))
        k.round_resid_max = rmax2[xoff[b]:xoff[b] + c].copy()
        out.append(k)
    return out


def vectors_to_field(block: BlockKernel):
    """The rounded vectors of a block (after `kernel_vectors(rationalize=True, field=...)`): per vector a list of coefficient tuples (x_0, .., x_{deg-1}) of
    `Fraction`s, entry = sum_k x_k g^k."""
    if block.coeffs is None:
        raise ValueError("vectors_to_field: the block was not rounded to a field (kernel_vectors(..., rationalize=True, field=...))")
    if np.any(np.asarray(block.round_status) != 0):
        raise KernelVectorError(f"{CLINDEP_MESSAGE}: the block has entries without a relation")
    c = block.coeffs
    return [[tuple(c[i, v]) for i in range(c.shape[0])] for v in range(c.shape[1])]


# ---- the exact positive-definiteness check over a number field: leading minors in Z[g] from split primes (src/rounding.jl:417-472; clrs_modp_minors_field) ----
FIELD_MINORS_DEGREES = (2, 3, 4)     # what k_minors_residues_field and k_field_frobenius are instantiated for
FIELD_FROBENIUS_MAX_PRIMES = 1 << 20


def _pmod_divmod(a, f, p):
    """(quotient, remainder) of the polynomial a by f over F_p (coefficient lists low to high, trimmed; f != 0)"""
    a = [int(v) % p for v in a]
    df, inv = len(f) - 1, pow(f[-1], -1, p)
    q = [0] * max(len(a) - df, 0)
    while len(a) - 1 >= df:
        c = a[-1] * inv % p
        if c:
            off = len(a) - 1 - df
            q[off] = c
            for j in range(df):
                a[off + j] = (a[off + j] - c * f[j]) % p
        a.pop()
    while a and a[-1] == 0:
        a.pop()
    return q, a


def _pmod_mul(a, b, f, p):
    """a b mod (f, p)"""
    if not a or not b:
        return []
    t = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    return _pmod_divmod(t, f, p)[1]


def _pmod_pow(base, e: int, f, p):
    """base^e mod (f, p) by square and multiply"""
    r, b = _pmod_divmod([1], f, p)[1], _pmod_divmod(base, f, p)[1]
    while e:
        if e & 1:
            r = _pmod_mul(r, b, f, p)
        b = _pmod_mul(b, b, f, p)
        e >>= 1
    return r


def _pmod_gcd(a, b, p):
    """the monic greatest common divisor over F_p"""
    a, b = [int(v) % p for v in a], [int(v) % p for v in b]
    while a and a[-1] == 0:
        a.pop()
    while b and b[-1] == 0:
        b.pop()
    while b:
        a, b = b, _pmod_divmod(a, b, p)[1]
    inv = pow(a[-1], -1, p) if a else 0
    return [v * inv % p for v in a]


def _frobenius_host(minpoly, p: int) -> list:
    """the coefficients of x^p mod (minpoly, p), `degree` of them, or -1 throughout where p divides the leading coefficient: what k_field_frobenius computes"""
    d = len(minpoly) - 1
    if minpoly[-1] % p == 0:
        return [-1] * d
    r = _pmod_pow([0, 1], p, [int(c) % p for c in minpoly], p)
    return r + [0] * (d - len(r))


def _split_roots(f, p: int) -> list:
    """the roots, ascending, of a polynomial f over F_p that is a product of distinct linear factors: Cantor-Zassenhaus, gcd(f, (x + a)^((p - 1) / 2) - 1)
    for a = 1, 2, .. (deterministic); by trial below 64"""
    f = _pmod_gcd(f, [], p)                                          # monic
    if len(f) <= 1:
        return []
    if len(f) == 2:
        return [(-f[0]) % p]
    if p < 64:
        return [r for r in range(p) if sum(c * pow(r, j, p) for j, c in enumerate(f)) % p == 0]
    for a in range(1, p):
        h = _pmod_pow([a, 1], (p - 1) // 2, f, p)
        h = [(h[0] - 1) % p] + h[1:] if h else [p - 1]
        g = _pmod_gcd(f, h, p)
        if 1 < len(g) < len(f):
            return sorted(_split_roots(g, p) + _split_roots(_pmod_divmod(f, g, p)[0], p))
    raise ArithmeticError(f"_split_roots: no splitting element mod {p}")


def field_frobenius(minpoly, primes, device: int = 0) -> np.ndarray:
    """x^p mod (f, p) for every prime of `primes` (in [2, 2^23), at most 2^20) on the device, one lane per prime (clrs_modp_field_frobenius): int32
    (len(primes), degree), row q the coefficients low to high, -1 throughout where the prime divides the leading coefficient.  `minpoly`: the integer
    coefficients of f, low to high, degree 2 .. 4, below 2^63 in size.  The `frobenius=` of `split_primes`."""
    f = [int(c) for c in minpoly]
    d = len(f) - 1
    if d not in FIELD_MINORS_DEGREES or f[-1] == 0 or any(abs(c) >= 1 << 63 for c in f):
        raise ValueError(f"field_frobenius: a polynomial of degree in {FIELD_MINORS_DEGREES} with coefficients below 2^63 is needed")
    pr = np.ascontiguousarray([int(p) for p in primes], dtype=np.int64)
    if pr.size < 1 or pr.size > FIELD_FROBENIUS_MAX_PRIMES or pr.min() < 2 or pr.max() >= MODP_PRIME_LIMIT:
        raise ValueError(f"field_frobenius: between 1 and {FIELD_FROBENIUS_MAX_PRIMES} primes in [2, 2^23) are needed")
    pr, fc, out = pr.astype(np.int32), np.array(f, dtype=np.int64), np.full((pr.size, d), -2, np.int32)
    _lib.check(_lib.load().clrs_modp_field_frobenius(int(device), d, fc.ctypes.data_as(_lib.p_i64), pr.size, pr.ctypes.data_as(_lib.p_i32), out.ctypes.data_as(_lib.p_i32)))
    return out


def split_primes(field, count: int, start: Optional[int] = None, frobenius=None):
    """The first `count` primes below `start` (default 2^23), descending, at which the minimal polynomial f of `field` (a `NumberField`, or the coefficient
    list itself) splits into distinct linear factors, with their roots: `(primes, roots)`, roots[q] the `degree` roots of f mod primes[q], ascending.

    p splits f completely iff p divides neither lc(f) nor disc(f) and x^p = x mod (f, p).  `frobenius(minpoly, primes)` -> rows of coefficients of x^p
    decides that for a batch: None is the host's square and multiply on Python integers, prime by prime; `field_frobenius` is the device, 4096 primes
    per call.  The roots of the primes that passed are found on the host (Cantor-Zassenhaus).  `ArithmeticError` when the primes run out."""
    f = [int(c) for c in (field.minpoly if hasattr(field, "minpoly") else field)]
    d = len(f) - 1
    if d < 2 or f[-1] == 0:
        raise ValueError("split_primes: a minimal polynomial of degree at least 2 is needed")
    fprime = [j * c for j, c in enumerate(f)][1:]
    want = [0, 1] + [0] * (d - 2)
    sched = _primes_descending()
    at = 0 if start is None else int(np.count_nonzero(sched >= int(start)))
    step = 1 if frobenius is None else 4096
    primes, roots = [], []
    while len(primes) < int(count):
        cand = [int(p) for p in sched[at:at + step]]
        if not cand:
            raise ArithmeticError("split_primes: the primes below 2^23 are exhausted")
        at += len(cand)
        rows = [_frobenius_host(f, p) for p in cand] if frobenius is None else np.asarray(frobenius(f, cand))
        for p, row in zip(cand, rows):
            if [int(v) for v in row] != want or f[-1] % p == 0 or len(_pmod_gcd(f, fprime, p)) != 1:
                continue
            primes.append(p)
            roots.append(_split_roots(f, p))
            if len(roots[-1]) != d:
                raise ArithmeticError(f"split_primes: {p} passed the test and has {len(roots[-1])} roots")
            if len(primes) == int(count):
                break
    return primes, roots


def _field_coeff_matrices(coeff_matrices, what):
    """-> object array (d, n, n) of Python integers, every matrix symmetric"""
    mats = [_symmetric_integer_matrix(M, what) for M in coeff_matrices]
    if len(mats) < 2 or any(m.shape != mats[0].shape for m in mats):
        raise ValueError(f"{what}: at least two coefficient matrices of one shape are needed")
    out = np.empty((len(mats),) + mats[0].shape, dtype=object)
    for j, m in enumerate(mats):
        out[j] = m
    return out


def leading_minors_field_mod(coeff_matrices, primes, roots, device: int = 0):
    """The leading principal minors of M = sum_j M_j g^j evaluated at g = roots[q][i] mod primes[q], for every pair, on the device: one call of
    clrs_modp_minors_field.  `coeff_matrices`: the d (2 .. 4) symmetric integer matrices M_0 .. M_(d-1) (n <= 128, Python integers of any size); `primes`
    distinct, in [2, 2^23), at most 65535; `roots` (len(primes), d): distinct numbers in [0, p) per prime (for the minors of M in Z[g]: the roots of the
    monic minimal polynomial of g mod p).  Returns `(minors, breakdown)`: int32 (len(primes), d, n) and (len(primes), d), per pair what
    `leading_minors_mod` returns per prime.  The counters are kept in `leading_minors_field_mod.last_info`."""
    a = _field_coeff_matrices(coeff_matrices, "leading_minors_field_mod")
    d, n = a.shape[0], a.shape[1]
    pr = np.ascontiguousarray([int(p) for p in primes], dtype=np.int64)
    if d not in FIELD_MINORS_DEGREES:
        raise ValueError(f"leading_minors_field_mod: the degree must be one of {FIELD_MINORS_DEGREES}, got {d}")
    if n < 1 or n > MINORS_MAX_N:
        raise ValueError(f"leading_minors_field_mod: n must lie in [1, {MINORS_MAX_N}], got {n}")
    if pr.size < 1 or pr.size > MINORS_MAX_PRIMES or pr.min() < 2 or pr.max() >= MODP_PRIME_LIMIT:
        raise ValueError(f"leading_minors_field_mod: between 1 and {MINORS_MAX_PRIMES} primes in [2, 2^23) are needed")
    rt = np.ascontiguousarray(np.asarray([[int(r) for r in row] for row in roots], dtype=np.int64).reshape(pr.size, -1))
    if rt.shape != (pr.size, d) or rt.min() < 0 or np.any(rt >= pr[:, None]):
        raise ValueError(f"leading_minors_field_mod: roots must be ({pr.size}, {d}) with every root in [0, p)")
    pr, rt = pr.astype(np.int32), rt.astype(np.int32)
    digits = np.ascontiguousarray(np.swapaxes(to_balanced_digits(a), 0, 1))                 # (d, nd, n, n)
    minors, breakdown, info = np.full((pr.size, d, n), -2, np.int32), np.full((pr.size, d), -2, np.int32), np.zeros(4, np.int32)
    ptr = lambda v: v.ctypes.data_as(_lib.p_i32)
    _lib.check(_lib.load().clrs_modp_minors_field(int(device), n, d, digits.shape[1], ptr(digits), pr.size, ptr(pr), ptr(rt), ptr(minors), ptr(breakdown), ptr(info)))
    leading_minors_field_mod.last_info = [int(v) for v in info]
    return minors, breakdown


leading_minors_field_mod.last_info = None


def _field_monic(field):
    """(h, a): a = |lc(f)| and h the monic integer minimal polynomial of a g (h(y) = a^(d-1) f(y / a) up to sign), low to high"""
    f = [int(c) for c in field.minpoly]
    if f[-1] < 0:
        f = [-c for c in f]
    a, d = f[-1], len(f) - 1
    return [c * a ** (d - 1 - j) for j, c in enumerate(f[:-1])] + [1], a


def _root_bound(h) -> int:
    """an integer rho >= |z| for every complex root z of the monic integer polynomial h: the smaller of Cauchy's 1 + max |h_j| and max(1, sum |h_j|), j < deg"""
    low = [abs(c) for c in h[:-1]]
    return min(1 + max(low), max(1, sum(low)))


def _trace_matrix_inverse(h):
    """T^-1 as `Fraction`s, T[a][b] = Tr(g^(a + b)) for a root g of the monic h: the power sums s_0 .. s_(2d-2) by Newton's identities"""
    d = len(h) - 1
    e = [1] + [(-1) ** k * h[d - k] for k in range(1, d + 1)]        # elementary symmetric polynomials of the roots
    s = [d]
    for k in range(1, 2 * d - 1):
        s.append(sum((-1) ** (i - 1) * e[i] * s[k - i] for i in range(1, min(k, d + 1))) + ((-1) ** (k - 1) * k * e[k] if k <= d else 0))
    T = [[Fraction(s[a + b]) for b in range(d)] + [Fraction(int(a == b)) for b in range(d)] for a in range(d)]
    for c in range(d):
        piv = next((r for r in range(c, d) if T[r][c] != 0), None)
        if piv is None:
            raise ArithmeticError("the minimal polynomial has a repeated root: its trace form is singular")
        T[c], T[piv] = T[piv], T[c]
        T[c] = [v / T[c][c] for v in T[c]]
        for r in range(d):
            if r != c and T[r][c] != 0:
                T[r] = [v - T[r][c] * w for v, w in zip(T[r], T[c])]
    return [row[d:] for row in T]


def field_minor_bounds(coeff_matrices, field) -> list:
    """Python integers `C_k`, k = 1 .. n, with |c_(k,j)| <= C_k for every coefficient of the k-th leading principal minor sum_j c_(k,j) h^j of
    M = sum_j M_j h^j, h the generator `checkpd_field` normalises to (lc(f) g: g itself where the minimal polynomial of `field` is monic), M_j the symmetric
    integer matrices `coeff_matrices`.  With rho >= every |conjugate of h| (`_root_bound`), E = sum_j |M_j| rho^j entry by entry and H_k =
    minor_bounds(E)[k - 1] (Hadamard), every conjugate of the minor is at most H_k in size; t_b = Tr(minor h^b) is then at most d H_k rho^b, and the
    coefficients are T^-1 t, T[a][b] = Tr(h^(a + b)): C_k = max_j ceil(H_k d sum_b |T^-1[j][b]| rho^b).  DESIGN.md section 24."""
    a = _field_coeff_matrices(coeff_matrices, "field_minor_bounds")
    h, _ = _field_monic(field)
    d = len(h) - 1
    if a.shape[0] != d:
        raise ValueError(f"field_minor_bounds: {d} coefficient matrices are needed for a field of degree {d}, got {a.shape[0]}")
    rho, n = _root_bound(h), a.shape[1]
    E = np.array([sum(abs(int(a[j, r, c])) * rho ** j for j in range(d)) for r in range(n) for c in range(n)], dtype=object).reshape(n, n)
    Tinv = _trace_matrix_inverse(h)
    factor = max(sum((abs(Tinv[j][b]) * d * rho ** b for b in range(d)), Fraction(0)) for j in range(d))
    return [-((-H * factor.numerator) // factor.denominator) for H in minor_bounds(E)]


def _poly_at(coeffs, x):
    acc = Fraction(0)
    for c in reversed(coeffs):
        acc = acc * x + c
    return acc


def _poly_range(coeffs, lo, hi):
    """an interval that holds sum_j coeffs[j] x^j for every x in [lo, hi]: Horner in interval arithmetic on exact rationals"""
    a = b = Fraction(0)
    for c in reversed(coeffs):
        prods = (a * lo, a * hi, b * lo, b * hi)
        a, b = min(prods) + c, max(prods) + c
    return a, b


class _RealRoot:
    """The real root of the monic integer polynomial h next to the rational `near`, held in an isolating interval [lo, hi] with dyadic endpoints: h changes
    sign on it and h' has no zero on it (interval evaluation), so it holds exactly one root.  `refine(bits)` shrinks it below 2^-bits by quadratic interval
    refinement (the interval is cut into N parts, the part the secant points at is kept when h changes sign on it and N is squared, else the interval is
    bisected and N goes back to its root): every step is decided by exact signs of h."""

    def __init__(self, h, near: Fraction, prec: int):
        self.h = [int(c) for c in h]
        dh = [j * c for j, c in enumerate(self.h)][1:]
        scale = max(1, abs(near.numerator) // near.denominator + 1)
        for k in sorted({max(prec - 16, 8), max(prec // 2, 8), 32, 16, 8}, reverse=True):
            w = Fraction(scale, 1 << k)
            lo, hi = near - w, near + w
            flo, fhi = _poly_at(self.h, lo), _poly_at(self.h, hi)
            if flo == 0 or fhi == 0:
                raise ArithmeticError("the minimal polynomial has a rational root: it is reducible")
            d0, d1 = _poly_range(dh, lo, hi)
            if (flo < 0) != (fhi < 0) and (d0 > 0 or d1 < 0):
                self.lo, self.hi, self.flo, self.fhi, self.N = lo, hi, flo, fhi, 4
                return
        raise ArithmeticError("the generator could not be isolated as a simple real root of the minimal polynomial")

    def refine(self, bits: int) -> None:
        tol = Fraction(1, 1 << bits)
        while self.hi - self.lo > tol:
            N, width = self.N, self.hi - self.lo
            t = self.flo / (self.flo - self.fhi)                     # the secant's zero, as a share of the width, in (0, 1)
            k = min(N - 1, (t.numerator * N) // t.denominator)
            a = self.lo + width * k / N
            b = a + width / N
            fa, fb = _poly_at(self.h, a), _poly_at(self.h, b)
            if fa == 0 or fb == 0:
                raise ArithmeticError("the minimal polynomial has a rational root: it is reducible")
            if (fa < 0) != (fb < 0):
                self.lo, self.hi, self.flo, self.fhi, self.N = a, b, fa, fb, N * N
                continue
            m = (self.lo + self.hi) / 2
            fm = _poly_at(self.h, m)
            if fm == 0:
                raise ArithmeticError("the minimal polynomial has a rational root: it is reducible")
            if (fm < 0) != (self.flo < 0):
                self.hi, self.fhi = m, fm
            else:
                self.lo, self.flo = m, fm
            self.N = max(4, _isqrt(N))

    def sign(self, coeffs, what: str) -> int:
        """the sign of sum_j coeffs[j] eta^j at the root eta, rigorously: 0 only for the zero element.  A non-zero element x of Z[eta] has a norm of size at
        least 1, and each of its d conjugates is at most B = sum_j |c_j| rho^j, so |x(eta)| >= B^(1-d): an interval of eta below 2^-bits decides the sign
        once bits exceeds (d - 1) log2 B by the slope of the polynomial.  The precision doubles from 64 bits up to that cap; `ArithmeticError`
        naming `what` when it is reached (a reducible `minpoly` can do that).  Never a guess."""
        c = [int(v) for v in coeffs]
        if not any(c):
            return 0
        d, rho = len(self.h) - 1, _root_bound(self.h)
        B = sum(abs(v) * rho ** j for j, v in enumerate(c))
        slope = sum(j * abs(v) * rho ** max(j - 1, 0) for j, v in enumerate(c))
        cap = (d - 1) * B.bit_length() + slope.bit_length() + 8
        bits = 64
        while True:
            self.refine(bits)
            lo, hi = _poly_range(c, self.lo, self.hi)
            if lo > 0:
                return 1
            if hi < 0:
                return -1
            if bits > cap:
                raise ArithmeticError(f"checkpd_field: the sign of {what} is undecided at {bits} bits, beyond what a non-zero element of the field allows: is minpoly irreducible?")
            bits *= 2


@dataclasses.dataclass
class FieldPDCertificate:
    """What `checkpd_field` proves about a symmetric matrix A over QQ(g).  `pd`: A is positive definite at the embedding g -> the real root gamma that
    `NumberField.g` approximates.  `minpoly`, `generator_scale`: the monic integer minimal polynomial of h = generator_scale g (generator_scale = |lc| of
    the field's minimal polynomial, 1 where that is monic) in which everything below is expressed.  `scale`: the positive integer D with D A = sum_j M_j h^j,
    M_j integer.  `minors`: the exact leading principal minors of D A, from order 1 up to where the walk stopped, each a list of d integers c_0 .. c_(d-1),
    the minor being sum_j c_j h^j.  `failed_order`: None, or the order of the first minor that is <= 0 at gamma (`minors[-1]`); when a diagonal entry <= 0
    decided on the host, `minors` is empty and `failed_order` is the 1-based index of that entry.  `primes`: every prime given to the device, in order, and
    `roots` their roots of `minpoly`, row by row; `discarded`: `(prime, root, order)` for every pair that broke down (a zero pivot at that order: that
    image of the minor is 0 mod the prime); the prime was left out of every minor behind the first of its breakdowns.  `interval`: rationals (lo, hi)
    with lo < gamma < hi, holding no other root of the minimal polynomial, as narrow as the signs needed."""
    pd: bool
    minors: list
    failed_order: Optional[int]
    scale: int
    primes: list
    roots: list
    discarded: list
    interval: tuple
    minpoly: list
    generator_scale: int

    def __bool__(self):
        return self.pd


def _mod_matrix_inverse(V, p: int):
    """the inverse of a small square matrix over F_p (Gauss-Jordan); `ArithmeticError` when singular"""
    d = len(V)
    a = [[int(v) % p for v in row] + [int(i == j) for j in range(d)] for i, row in enumerate(V)]
    for c in range(d):
        piv = next((r for r in range(c, d) if a[r][c]), None)
        if piv is None:
            raise ArithmeticError(f"two equal roots mod {p}")
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, p)
        a[c] = [v * inv % p for v in a[c]]
        for r in range(d):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(v - f * w) % p for v, w in zip(a[r], a[c])]
    return [row[d:] for row in a]


def checkpd_field(A, field, device: int = 0, minors=None, primes=None) -> FieldPDCertificate:
    """Is the symmetric matrix `A` over QQ(g) positive definite at the real embedding g -> gamma of `field` (a `NumberField`; gamma the real root its `g`
    approximates)?  `A`: (n, n) coefficient tuples (x_0 .. x_(d-1)) of `Fraction`s or integers, entry = sum_j x_j g^j (what `vectors_to_field` uses), n <=
    128.  An exact answer with its proof, where the reference's checkpd_cholesky(A; FF, g) (src/rounding.jl:417-472) embeds A at Arb balls and doubles the
    precision until 2^14 bits.  `ValueError` unless A is square and symmetric.

    The block is cleared of denominators and, where the minimal polynomial is not monic, rewritten in h = |lc| g, so that its leading principal minors lie
    in Z[h]; A is positive definite iff every one of them is positive at gamma.  An empty block is positive definite; a diagonal entry <= 0 at gamma
    answers from the host.  Otherwise: primes at which the minimal polynomial splits (`primes(field, count, start)` -> `(primes, roots)`, default
    `split_primes`, the host scan; `functools.partial(split_primes, frobenius=field_frobenius)` scans on the device), the minors of the d residue matrices
    of every prime (`minors(coeff_matrices, primes, roots, device=...)`, default `leading_minors_field_mod`), the coefficients mod p by the inverse
    Vandermonde matrix of the roots, lifted by `crt_tree` against `field_minor_bounds`, and the sign of each minor at gamma by interval arithmetic on an
    isolating interval of gamma (`ArithmeticError` naming the order if a sign stays undecided at the precision a non-zero element allows).  The walk is
    that of `checkpd`: a prime one of whose pairs breaks down at order k is usable up to and including k."""
    minors_fn = leading_minors_field_mod if minors is None else minors
    primes_fn = split_primes if primes is None else primes
    h, lc = _field_monic(field)
    d = len(h) - 1
    if d < 2:
        raise ValueError("checkpd_field: a field of degree at least 2 is needed (checkpd is the check over QQ)")
    neg, man, exp, _ = field.g._mpf_                                # the mpmath number exactly: (-1)^neg man 2^exp
    root = _RealRoot(h, Fraction(-int(man) if neg else int(man)) * Fraction(2) ** int(exp) * lc, int(field.prec))
    interval = lambda: (root.lo / lc, root.hi / lc)
    empty = lambda pd, order, scale: FieldPDCertificate(pd, [], order, scale, [], [], [], interval(), h, lc)
    try:
        rows_in = [list(r) for r in A]
    except TypeError:
        raise ValueError("checkpd_field: the block must be an (n, n) array of coefficient tuples") from None
    n = len(rows_in)
    if n == 0:
        return empty(True, None, 1)
    if any(len(r) != n for r in rows_in):
        raise ValueError(f"checkpd_field: the block must be square, got rows of {sorted({len(r) for r in rows_in})} entries for {n} rows")
    try:
        rows = [[[Fraction(x) for x in e] for e in r] for r in rows_in]
    except TypeError:
        rows = None
    if rows is None or any(len(e) != d for r in rows for e in r):
        raise ValueError(f"checkpd_field: every entry must be a tuple of {d} coefficients")
    if any(rows[i][j] != rows[j][i] for i in range(n) for j in range(i)):
        raise ValueError("checkpd_field: the block must be symmetric")
    Af = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            Af[i, j] = tuple(rows[i][j])
    scale, M = _field_integer_form(Af, h, lc)
    for i in range(n):
        if root.sign([M[c, i, i] for c in range(d)], f"diagonal entry {i + 1}") <= 0:
            return empty(False, i + 1, scale)
    if n > MINORS_MAX_N:
        raise ValueError(f"checkpd_field: blocks of more than {MINORS_MAX_N} rows are not supported, got {n}")
    bounds = field_minor_bounds(M, field)
    plist, rlist, breaks, pair_breaks, coeffs = [], [], [], [], []   # per prime: roots, first breakdown, the breakdowns of its pairs, (d, n) coefficients mod p
    exact, done = [], 0
    while done < n:
        need, have = 2 * max(max(bounds[done:]), 1), _product(p for p, k in zip(plist, breaks) if k == 0)
        count = max(1, -(-(need.bit_length() - have.bit_length() + 2) // 22))      # every prime drawn exceeds 2^22 while they last
        count = min(count, MINORS_MAX_PRIMES)
        batch, batch_roots = primes_fn(field, count, plist[-1] if plist else None)
        batch = [int(p) for p in batch]
        batch_roots = [[int(r) * lc % p for r in rr] for p, rr in zip(batch, batch_roots)]            # the roots of h: lc times those of the field's polynomial
        res, brk = minors_fn(M, batch, batch_roots, device=device)
        res, brk = np.asarray(res).reshape(len(batch), d, n), np.asarray(brk).reshape(len(batch), d)
        for q, p in enumerate(batch):
            Vinv = np.array(_mod_matrix_inverse([[pow(r, j, p) for j in range(d)] for r in batch_roots[q]], p), dtype=np.int64)
            img = np.where(res[q] < 0, 0, res[q]).astype(np.int64)                                  # (-1 behind a breakdown: never read, see `usable`)
            coeffs.append((Vinv @ img) % p)                                                         # d products below 2^46 each
            ks = [int(k) for k in brk[q]]
            pair_breaks.append(ks)
            breaks.append(min((k for k in ks if k), default=0))
        plist += batch
        rlist += batch_roots
        groups, products, order = {}, {}, done + 1
        while order <= n:
            usable = tuple(q for q, k in enumerate(breaks) if k == 0 or k >= order)
            if usable not in products:
                products[usable] = _product(plist[q] for q in usable)
            if not usable or products[usable] <= 2 * bounds[order - 1]:
                break
            groups.setdefault(usable, []).append(order)
            order += 1
        stop = False
        for usable, orders in groups.items():                      # (insertion order: ascending orders)
            residues = np.array([[int(coeffs[q][c, k - 1]) for k in orders for c in range(d)] for q in usable], dtype=np.int64)
            values, _ = crt_tree(residues, [plist[q] for q in usable])
            for t, k in enumerate(orders):
                minor = [int(v) for v in values[t * d:(t + 1) * d]]
                exact.append(minor)
                done = k
                if root.sign(minor, f"the minor of order {k}") <= 0:
                    stop = True
                    break
            if stop:
                break
        if stop:
            break
    discarded = [(p, rr[i], ks[i]) for p, rr, ks in zip(plist, rlist, pair_breaks) for i in range(d) if ks[i] != 0]
    failed = done if stop else None
    return FieldPDCertificate(failed is None, exact, failed, scale, plist, rlist, discarded, interval(), h, lc)


# ---- the basis change over a number field: adjugate and determinant in Z[h] from split primes (src/rounding.jl:834-836, 1017-1050; clrs_modp_field_adjugate) ----
def _square_coeff_matrices(coeff_matrices, what):
    """-> object array (d, n, n) of Python integers: d >= 2 square matrices of one shape, not necessarily symmetric"""
    mats = [_integer_matrix(M, what) for M in coeff_matrices]
    if len(mats) < 2 or any(m.shape != mats[0].shape for m in mats) or mats[0].shape[0] != mats[0].shape[1]:
        raise ValueError(f"{what}: at least two square coefficient matrices of one shape are needed")
    n = mats[0].shape[0]
    out = np.empty((len(mats), n, n), dtype=object)
    for j, m in enumerate(mats):
        out[j].flat = [int(v) for v in m.flat]
    return out


def field_adjugate_mod(coeff_matrices, primes, roots, device: int = 0):
    """The determinant and the adjugate of M = sum_j M_j g^j evaluated at g = roots[q][i] mod primes[q], for every pair, on the device: one call of
    clrs_modp_field_adjugate.  `coeff_matrices`: the d (2 .. 4) square integer matrices M_0 .. M_(d-1) (n <= 128, Python integers of any size, not
    necessarily symmetric); `primes` descending, in [2, 2^23), at most 65535; `roots` (len(primes), d): distinct numbers in [0, p) per prime (for the
    images of det M and adj M in Z[g]: the roots of the monic minimal polynomial of g mod p).  Returns `(adj, det, breakdown)`: int32
    (len(primes), d, n, n), (len(primes), d) and (len(primes), d).  Per pair: det M(r) mod p and adj M(r) = det M(r) M(r)^-1 mod p with breakdown 0; or,
    where M(r) is singular mod p, det 0, adj -1 throughout and breakdown c + 1, c the first column that depends on the columns before it.  The counters
    are kept in `field_adjugate_mod.last_info` (`[LDS bytes per workgroup, workgroups, singular pairs, 0]`)."""
    a = _square_coeff_matrices(coeff_matrices, "field_adjugate_mod")
    d, n = a.shape[0], a.shape[1]
    pr = np.ascontiguousarray([int(p) for p in primes], dtype=np.int64)
    if d not in FIELD_MINORS_DEGREES:
        raise ValueError(f"field_adjugate_mod: the degree must be one of {FIELD_MINORS_DEGREES}, got {d}")
    if n < 1 or n > MINORS_MAX_N:
        raise ValueError(f"field_adjugate_mod: n must lie in [1, {MINORS_MAX_N}], got {n}")
    if pr.size < 1 or pr.size > MINORS_MAX_PRIMES or pr.min() < 2 or pr.max() >= MODP_PRIME_LIMIT:
        raise ValueError(f"field_adjugate_mod: between 1 and {MINORS_MAX_PRIMES} primes in [2, 2^23) are needed")
    rt = np.ascontiguousarray(np.asarray([[int(r) for r in row] for row in roots], dtype=np.int64).reshape(pr.size, -1))
    if rt.shape != (pr.size, d) or rt.min() < 0 or np.any(rt >= pr[:, None]):
        raise ValueError(f"field_adjugate_mod: roots must be ({pr.size}, {d}) with every root in [0, p)")
    pr, rt = pr.astype(np.int32), rt.astype(np.int32)
    digits = np.ascontiguousarray(np.swapaxes(to_balanced_digits(a), 0, 1))                 # (d, nd, n, n)
    adj, det = np.full((pr.size, d, n, n), -2, np.int32), np.full((pr.size, d), -2, np.int32)
    breakdown, info = np.full((pr.size, d), -2, np.int32), np.zeros(4, np.int32)
    ptr = lambda v: v.ctypes.data_as(_lib.p_i32)
    _lib.check(_lib.load().clrs_modp_field_adjugate(int(device), n, d, digits.shape[1], ptr(digits), pr.size, ptr(pr), ptr(rt), ptr(adj), ptr(det), ptr(breakdown),
                                                    ptr(info)))
    field_adjugate_mod.last_info = [int(v) for v in info]
    return adj, det, breakdown


field_adjugate_mod.last_info = None


def _field_hadamard(a, h):
    """(H, factor) for the integer coefficient matrices `a` (d, n, n) of M = sum_j M_j h^j, h a root of the monic integer polynomial `h`: with rho >= every
    |conjugate of h| and E = sum_j |M_j| rho^j entry by entry, H = prod_i max(1, ceil ||row i of E||_2) bounds every conjugate of every minor of M of
    order n - 1 and n (Hadamard, rows of norm below 1 counted as 1 so that leaving a row out never raises the bound); `factor` (a `Fraction`) turns a
    bound on the conjugates of an element of Z[h] into one on its coefficients, max_j d sum_b |T^-1[j][b]| rho^b (`field_minor_bounds`)."""
    d, n = a.shape[0], a.shape[1]
    rho = _root_bound(h)
    H = 1
    for i in range(n):
        s = sum(sum(abs(int(a[j, i, c])) * rho ** j for j in range(d)) ** 2 for c in range(n))
        r = _isqrt(s)
        H *= max(1, r if r * r == s else r + 1)
    Tinv = _trace_matrix_inverse(h)
    factor = max(sum((abs(Tinv[j][b]) * d * rho ** b for b in range(d)), Fraction(0)) for j in range(d))
    return H, factor


def field_adjugate_bounds(coeff_matrices, field) -> int:
    """A Python integer `C` with |c| <= C for every coefficient c in Z[h] of det M and of every entry of adj M, M = sum_j M_j h^j with the square integer
    matrices `coeff_matrices` and h the generator `inverse_field` normalises to (lc(f) g: g itself where the minimal polynomial of `field` is monic):
    C = ceil(H factor) with `(H, factor)` of `_field_hadamard`.  DESIGN.md section 25."""
    a = _square_coeff_matrices(coeff_matrices, "field_adjugate_bounds")
    h, _ = _field_monic(field)
    if a.shape[0] != len(h) - 1:
        raise ValueError(f"field_adjugate_bounds: {len(h) - 1} coefficient matrices are needed for a field of degree {len(h) - 1}, got {a.shape[0]}")
    H, factor = _field_hadamard(a, h)
    return -((-H * factor.numerator) // factor.denominator)


def _minpoly_of(field) -> list:
    return [int(c) for c in (field.minpoly if hasattr(field, "minpoly") else field)]


def _field_matrix(M, d: int, what: str) -> np.ndarray:
    """a matrix of coefficient tuples (nested lists, or an object array of tuples, or an array (rows, cols, d)) -> an object array (rows, cols) whose
    entries are tuples of d `Fraction`s"""
    try:
        rows = [list(r) for r in M]
    except TypeError:
        raise ValueError(f"{what}: a matrix of coefficient tuples is needed") from None
    cols = len(rows[0]) if rows else (M.shape[1] if isinstance(M, np.ndarray) and M.ndim >= 2 else 0)
    out = np.empty((len(rows), cols), dtype=object)
    for i, r in enumerate(rows):
        if len(r) != cols:
            raise ValueError(f"{what}: rows of {cols} and of {len(r)} entries")
        for j, e in enumerate(r):
            try:
                t = tuple(Fraction(x) for x in e)
            except TypeError:
                t = ()
            if len(t) != d:
                raise ValueError(f"{what}: every entry must be a tuple of {d} coefficients")
            out[i, j] = t
    return out


def _field_fold(t, f) -> tuple:
    """the coefficients t_0 .. t_(2d-2) of a polynomial in g reduced by the minimal polynomial f (degree d, not necessarily monic): a tuple of d Fractions"""
    d = len(f) - 1
    t = list(t)
    for k in range(len(t) - 1, d - 1, -1):
        c = t[k] if f[d] == 1 else t[k] / f[d]                       # (a monic f keeps integers integers)
        if c:
            for j in range(d):
                t[k - d + j] -= c * f[j]
    return tuple(t[:d])


def field_matmul(A, B, field, matmul=None, device: int = 0) -> np.ndarray:
    """The product of two matrices over QQ(g): `A` (m, k) and `B` (k, n) of coefficient tuples of `Fraction`s or integers in g (what `vectors_to_field`
    uses), `field` a `NumberField` or the coefficient list of its minimal polynomial.  Returns an object array (m, n) of tuples of `Fraction`s.
    With `matmul` None everything is done in `Fraction`s.  With `matmul(A, B, device=...)` (`zz_matmul`) the coefficient planes A_0 .. A_(d-1) and B_0 ..
    B_(d-1), each operand over the common denominator of its entries, are stacked and multiplied as ONE integer product `[A_0; ..; A_(d-1)] [B_0 | .. |
    B_(d-1)]`: block (a, b) is A_a B_b, the blocks with a + b = e add up to the coefficient of g^e, and the 2d - 1 coefficients are folded by the
    minimal polynomial."""
    f = _minpoly_of(field)
    d = len(f) - 1
    Af, Bf = _field_matrix(A, d, "field_matmul"), _field_matrix(B, d, "field_matmul")
    m, k, n = Af.shape[0], Af.shape[1], Bf.shape[1]
    if Bf.shape[0] != k:
        raise ValueError(f"field_matmul: the shapes {Af.shape} and {Bf.shape} do not match")
    out = np.empty((m, n), dtype=object)
    if m == 0 or n == 0:
        return out
    if matmul is None or k == 0:
        for i in range(m):
            for j in range(n):
                t = [Fraction(0)] * (2 * d - 1)
                for l in range(k):
                    x, y = Af[i, l], Bf[l, j]
                    for a in range(d):
                        if x[a]:
                            for b in range(d):
                                t[a + b] += x[a] * y[b]
                out[i, j] = _field_fold(t, f)
        return out
    (an, al), (bn, bl) = _common_denominator(x for e in Af.flat for x in e), _common_denominator(x for e in Bf.flat for x in e)
    an, bn = an.reshape(m, k, d), bn.reshape(k, n, d)
    left, right = np.empty((d * m, k), dtype=object), np.empty((k, d * n), dtype=object)
    for a in range(d):
        left[a * m:(a + 1) * m] = an[:, :, a]
        right[:, a * n:(a + 1) * n] = bn[:, :, a]
    prod = _matmul_matrix(matmul, left, right, device)
    den = al * bl
    for i in range(m):
        for j in range(n):
            t = [0] * (2 * d - 1)
            for a in range(d):
                for b in range(d):
                    t[a + b] += int(prod[a * m + i, b * n + j])
            out[i, j] = _field_fold([Fraction(v, den) for v in t], f)
    return out


@dataclasses.dataclass
class FieldInverse:
    """What `inverse_field` computes for a square matrix B over QQ(g).  `inverse`: B^-1, an object array (n, n) of tuples of `Fraction`s in g.  `minpoly`,
    `generator_scale`: the monic integer minimal polynomial of h = generator_scale g (generator_scale = |lc| of the field's minimal polynomial) in which the
    next two are expressed.  `scale`: the positive integer D with D B = M = sum_j M_j h^j, M_j integer.  `adjugate`: adj M, an object array (n, n) of tuples
    of d integers, and `det` = det M, a list of d integers, both exact: M adj M = det M I in Z[h], and B^-1 = scale adj M / det M.  `primes`: every prime
    given to the device, in order, `roots` their roots of `minpoly`, row by row; `discarded`: the primes one of whose pairs was singular (they divide the
    norm of det M) and took no part in the lifting."""
    inverse: np.ndarray
    adjugate: np.ndarray
    det: list
    scale: int
    minpoly: list
    generator_scale: int
    primes: list
    roots: list
    discarded: list


def _field_element_inverse(c, h) -> tuple:
    """the inverse in QQ[x] / (h) of the element with coefficients c (h monic of degree d): the d x d `Fraction` solve (multiplication by c) y = 1;
    `ZeroDivisionError` for a zero divisor"""
    d = len(h) - 1
    cols, cur = [], tuple(Fraction(v) for v in c)
    for _ in range(d):                                               # column j: c x^j
        cols.append(cur)
        cur = _field_fold((Fraction(0),) + cur, h)
    A = [[cols[j][i] for j in range(d)] + [Fraction(int(i == 0))] for i in range(d)]
    for k in range(d):
        piv = next((r for r in range(k, d) if A[r][k] != 0), None)
        if piv is None:
            raise ZeroDivisionError("the element is not invertible in the field")
        A[k], A[piv] = A[piv], A[k]
        A[k] = [v / A[k][k] for v in A[k]]
        for r in range(d):
            if r != k and A[r][k] != 0:
                A[r] = [v - A[r][k] * w for v, w in zip(A[r], A[k])]
    return tuple(A[i][d] for i in range(d))


def _field_integer_form(Bf, h, lc):
    """(scale, M): the object array (d, rows, cols) of the integers M_j with scale B = sum_j M_j h^j, h = lc g, for a matrix B of tuples of `Fraction`s in g:
    sum_j x_j g^j = sum_j x_j lc^-j h^j, and times scale = L lc^(d-1), L the least common denominator of the coefficients, every coefficient is an integer
    (the normal form of `checkpd_field` and `inverse_field`)"""
    from math import gcd
    d = len(h) - 1
    L = 1
    for e in Bf.flat:
        for x in e:
            L = L * x.denominator // gcd(L, x.denominator)
    M = np.empty((d,) + Bf.shape, dtype=object)
    for i in range(Bf.shape[0]):
        for j in range(Bf.shape[1]):
            for c in range(d):
                M[c, i, j] = int(Bf[i, j][c] * L) * lc ** (d - 1 - c)
    return L * lc ** (d - 1), M


def inverse_field(B, field, device: int = 0, adjugate=None, primes=None, matmul=None, check: bool = True):
    """The inverse of a square matrix `B` over QQ(g) (the reference's `inv(B)` over `FF`, src/rounding.jl:836), exactly and with a proven bound: a
    `FieldInverse`.  `B`: (n, n) coefficient tuples of `Fraction`s or integers in g, n <= 128; `field` a `NumberField`.  A field of degree 1, or entries
    that are not tuples, go to `inverse_qq` (whose result is returned).

    B is cleared of denominators and rewritten in h = |lc| g exactly as `checkpd_field` does: scale B = M = sum_j M_j h^j.  det M and the entries of adj M lie
    in Z[h] with coefficients of size at most C = `field_adjugate_bounds(M, field)`.  Split primes are drawn with `primes(field, count, start)` ->
    `(primes, roots)` (default `split_primes`) until their product exceeds 2 C -- the fewest that do, every prime being below 2^23 -- and go to
    `adjugate(coeff_matrices, primes, roots, device=...)` (default `field_adjugate_mod`, one device call).  A prime with a singular pair divides the norm of
    det M; it is recorded in `discarded`, left out, and replaced by further primes.  |Norm(det M)| <= H^d (H the Hadamard bound of `_field_hadamard`), so once
    the product of the discarded primes exceeds H^d the matrix is singular: `SingularSystemError`, a proof.  Per prime the d images give the coefficients
    mod p by the inverse Vandermonde matrix of the roots; `crt_tree` lifts them to the symmetric range, where they are the coefficients themselves.
    With `check`, M adj M == det M I is verified exactly through `field_matmul(..., matmul=matmul)` (`ArithmeticError` otherwise).  Finally
    B^-1 = scale adj M / det M, the inverse of det M by a d x d `Fraction` solve, rewritten in g."""
    d = field.degree if hasattr(field, "degree") else 1
    rows_in = [list(r) for r in B]
    if d < 2 or not any(isinstance(x, tuple) for r in rows_in for x in r):
        return inverse_qq([[x[0] if isinstance(x, tuple) else x for x in r] for r in rows_in], device=device, check=check, matmul=matmul)
    adj_fn = field_adjugate_mod if adjugate is None else adjugate
    primes_fn = split_primes if primes is None else primes
    h, lc = _field_monic(field)
    Bf = _field_matrix(rows_in, d, "inverse_field")
    n = Bf.shape[0]
    if Bf.shape[1] != n:
        raise ValueError(f"inverse_field: the matrix must be square, got {Bf.shape[0]} x {Bf.shape[1]}")
    if n == 0:
        return FieldInverse(np.empty((0, 0), dtype=object), np.empty((0, 0), dtype=object), [1] + [0] * (d - 1), 1, h, lc, [], [], [])
    if n > MINORS_MAX_N:
        raise ValueError(f"inverse_field: matrices of more than {MINORS_MAX_N} rows are not supported, got {n}")
    scale, M = _field_integer_form(Bf, h, lc)
    H, factor = _field_hadamard(M, h)
    need = 2 * (-((-H * factor.numerator) // factor.denominator))
    plist, rlist, discarded, good, coeffs, pending, pending_roots = [], [], [], [], [], [], []
    while True:
        have = _product(good) * _product(pending)
        if have <= need:                                             # every prime is below 2^23: no fewer than this many more will do
            count = max(1, -(-(need // have).bit_length() // 23))
            batch, batch_roots = primes_fn(field, count, (pending or plist or [None])[-1])
            pending += [int(p) for p in batch]
            pending_roots += [[int(r) * lc % int(p) for r in rr] for p, rr in zip(batch, batch_roots)]     # the roots of h: lc times those of the field's polynomial
            continue
        if not pending:
            break
        for at in range(0, len(pending), MINORS_MAX_PRIMES):
            pp, rr = pending[at:at + MINORS_MAX_PRIMES], pending_roots[at:at + MINORS_MAX_PRIMES]
            adj, det, brk = adj_fn(M, pp, rr, device=device)
            adj, det, brk = np.asarray(adj).reshape(len(pp), d, n * n), np.asarray(det).reshape(len(pp), d), np.asarray(brk).reshape(len(pp), d)
            for q, p in enumerate(pp):
                if np.any(brk[q] != 0):
                    discarded.append(p)
                    continue
                Vinv = np.array(_mod_matrix_inverse([[pow(r, j, p) for j in range(d)] for r in rr[q]], p), dtype=np.int64)
                img = np.concatenate([det[q].reshape(d, 1), adj[q]], axis=1).astype(np.int64)
                good.append(p)
                coeffs.append(((Vinv @ img) % p).reshape(-1))                                       # d products below 2^46 each; [coefficient][det, entries]
        plist += pending
        rlist += pending_roots
        pending, pending_roots = [], []
        if _product(discarded) > H ** d:
            raise SingularSystemError(f"inverse_field: the matrix is singular: the split primes {discarded} divide the norm of its determinant, and their "
                                      f"product exceeds the bound H^d on that norm")
    coeffs, values = np.array(coeffs, dtype=np.int64), []
    for at in range(0, coeffs.shape[1], 8192):                       # (in slices: crt_tree holds its leaves as Python integers)
        values += crt_tree(coeffs[:, at:at + 8192], good)[0]
    values = np.array([int(v) for v in values], dtype=object).reshape(d, 1 + n * n)
    detc = [int(v) for v in values[:, 0]]
    adjM = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            adjM[i, j] = tuple(int(v) for v in values[:, 1 + i * n + j])
    if not any(detc):
        raise ArithmeticError("inverse_field: the determinant lifted to zero although no pair was singular")
    if check:
        Mh = np.empty((n, n), dtype=object)
        for i in range(n):
            for j in range(n):
                Mh[i, j] = tuple(int(M[c, i, j]) for c in range(d))
        prod = field_matmul(Mh, adjM, h, matmul=matmul, device=device)
        want, zero = tuple(Fraction(v) for v in detc), (Fraction(0),) * d
        if any(prod[i, j] != (want if i == j else zero) for i in range(n) for j in range(n)):
            raise ArithmeticError("inverse_field: M adj(M) != det(M) I")
    num, den = _common_denominator(_field_element_inverse(detc, h))                              # 1 / det M = (sum_b num_b h^b) / den: the products below stay integers
    inv = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            t = [0] * (2 * d - 1)
            for a, x in enumerate(adjM[i, j]):
                if x:
                    for b in range(d):
                        t[a + b] += x * int(num[b])
            inv[i, j] = tuple(Fraction(scale * y * lc ** c, den) for c, y in enumerate(_field_fold(t, h)))      # sum_c y_c h^c = sum_c y_c lc^c g^c
    return FieldInverse(inv, adjM, detc, scale, h, lc, plist, rlist, discarded)


def _field_completions(V, field, maxprimes, device, batch, primes):
    """the generator behind `complete_basis_field`: yields a `PivotList` for every (split prime, root) pair, in order, at which the columns of V stay
    independent; at most `maxprimes` primes; `ValueError` when there is none"""
    batch = rref_mod_p if batch is None else batch
    primes_fn = split_primes if primes is None else primes
    if int(maxprimes) < 1:
        raise ValueError(f"complete_basis_field: maxprimes must be at least 1, got {maxprimes}")
    h, lc = _field_monic(field)
    d = len(h) - 1
    Vf = _field_matrix(V, d, "complete_basis_field")
    N, s = Vf.shape
    if s > N:
        raise ValueError(f"complete_basis_field: {s} vectors of {N} entries cannot be independent")
    if s == 0:
        yield PivotList(range(N))
        return
    rows = [_field_integer_form(Vf[r:r + 1], h, lc)[1][:, 0, :] for r in range(N)]           # every row over its own denominator: (d, s) integers in h
    tried, start, accepted = [], None, False
    for _ in range(int(maxprimes)):
        (p,), (rr,) = primes_fn(field, 1, start)
        p, start = int(p), int(p)
        tried.append(p)
        for r in rr:
            rh = int(r) * lc % p
            M = np.zeros((N, s + N), dtype=object)
            for i in range(N):
                M[i, :s] = [sum(int(rows[i][c, j]) * pow(rh, c, p) for c in range(d)) % p for j in range(s)]
                M[i, s + i] = 1
            pivots = [int(c) for c in batch(M, p, device=device)[0]]
            if pivots[:s] == list(range(s)):
                if len(pivots) != N:
                    raise ArithmeticError(f"complete_basis_field: {len(pivots)} pivots for {N} rows at p = {p}")
                out = PivotList([c - s for c in pivots[s:]], tried, p)
                out.root = int(r)
                accepted = True
                yield out
    if not accepted:
        raise ValueError(f"complete_basis_field: the columns of V are dependent at every root of every prime tried ({tried})")


def complete_basis_field(V, field, maxprimes: int = 3, device: int = 0, batch=None, primes=None) -> PivotList:
    """`complete_basis` for vectors over QQ(g): the standard basis vectors that complete the independent columns of `V` ((N, s) coefficient tuples) to a
    basis of QQ(g)^N, by the greedy choice of the reference (src/rounding.jl:1032-1049), decided at ONE (split prime, root) pair: g -> r is a ring map
    to F_p, so the pivot columns of the reduced row-echelon form of the residue matrix `[V(r) mod p | I_N]` (every row of V cleared of denominators first)
    are those over the field unless p divides a deciding minor at that root, which `basis_transformations` rules out afterwards from the inverse.  The pairs
    are taken prime by prime (`primes(field, count, start)`, default `split_primes`; at most `maxprimes` primes) and root by root; a pair is accepted only
    when the first s pivots are the columns 0 .. s - 1.  `batch(A, p, device=...)` -> `(pivots, rank)` replaces the device call (default `rref_mod_p`).
    Returns a `PivotList` of N - s indices with `.p`, `.primes` and `.root` (the root of the field's minimal polynomial); `ValueError` when no pair is
    accepted."""
    return next(_field_completions(V, field, maxprimes, device, batch, primes))


def _field_transform_products(P, M, field, matmul, device):
    return field_matmul(field_matmul(P, M, field, matmul=matmul, device=device), P.T, field, matmul=matmul, device=device)


def transform_field(M, Binv, s: int, field, matmul=None, device: int = 0) -> np.ndarray:
    """`transform` over QQ(g): `Binv[s:, :] M Binv^T[:, s:]` for (N, N) matrices of coefficient tuples, an object array (N - s, N - s) of tuples; the two
    products through `field_matmul` (`matmul` as there)."""
    d = len(_minpoly_of(field)) - 1
    Mf, Bf, s = _field_matrix(M, d, "transform_field"), _field_matrix(Binv, d, "transform_field"), int(s)
    N = Bf.shape[0]
    if Bf.shape[1] != N or Mf.shape != (N, N) or not 0 <= s <= N:
        raise ValueError(f"transform_field: M and Binv must be (N, N) and 0 <= s <= N, got {Mf.shape}, {Bf.shape} and s = {s}")
    return _field_transform_products(Bf[s:, :], Mf, field, matmul, device)


def undo_transform_field(Mt, Binv, s: int, field, matmul=None, device: int = 0) -> np.ndarray:
    """`undo_transform` over QQ(g): `Mt` ((N - s, N - s) coefficient tuples) padded with s zero rows and columns in front and multiplied by `Binv^T` from
    the left and `Binv` from the right, through `field_matmul`."""
    d = len(_minpoly_of(field)) - 1
    Bf, Mf, s = _field_matrix(Binv, d, "undo_transform_field"), _field_matrix(Mt, d, "undo_transform_field"), int(s)
    N = Bf.shape[0]
    if Bf.shape[1] != N or not 0 <= s <= N or Mf.shape != (N - s, N - s):
        raise ValueError(f"undo_transform_field: Binv must be (N, N) and Mt (N - s, N - s), got {Bf.shape}, {Mf.shape} and s = {s}")
    padded = np.empty((N, N), dtype=object)
    for i in range(N):
        for j in range(N):
            padded[i, j] = Mf[i - s, j - s] if i >= s and j >= s else (Fraction(0),) * d
    return _field_transform_products(Bf.T, padded, field, matmul, device)


def _basis_transformations_field(kernels, field, device, maxprimes, batch, check, matmul, adjugate, primes) -> dict:
    """the unreduced branch of `basis_transformations` over QQ(g): B = [V | E], Binv = inverse_field(B).inverse, not normalised"""
    d = field.degree
    zero, one = (Fraction(0),) * d, (Fraction(1),) + (Fraction(0),) * (d - 1)
    out = {}
    for key, (N, vectors) in kernels.items():
        N, s = int(N), len(vectors)
        B = np.empty((N, N), dtype=object)
        for i in range(N):
            for j in range(N):
                B[i, j] = one if i == j and s == 0 else zero
        if s == 0:
            out[key] = (B.T.copy(), B.copy(), 0)
            continue
        for c, v in enumerate(vectors):
            if len(v) != N:
                raise ValueError(f"basis_transformations: block {key!r}: vector {c} has {len(v)} entries for a block of size {N}")
            column = _field_matrix([[x if isinstance(x, tuple) else (x,) + (0,) * (d - 1) for x in v]], d, "basis_transformations")
            for i in range(N):
                B[i, c] = column[0, i]
        Binv = None
        completions = _field_completions(B[:, :s], field, maxprimes, device, batch, primes)
        for extra in completions:
            for i in range(N):
                for c, j in enumerate(extra):
                    B[i, s + c] = one if i == j else zero
            Binv = inverse_field(B, field, device=device, adjugate=adjugate, primes=primes, matmul=matmul, check=check).inverse
            taken = set(extra)
            if all(not any(Binv[s + c, i]) for i in range(N) if i not in taken for c, j in enumerate(extra) if j > i):
                break
            Binv = None
        completions.close()
        if Binv is None:
            raise ArithmeticError(f"basis_transformations: block {key!r}: no pair gave the greedy completion of the kernel vectors")
        out[key] = (B.T.copy(), Binv, s)
    return out


# ---- the system over QQ(g) as a system over QQ, and its approximate solution in the extension (src/rounding.jl:1256-1282, 537-568) ----
def convert_system(A, b, field):
    """The reference's `convert_system` (src/rounding.jl:1256-1282): the system `A x = b` over QQ(g) -- `A` (n, m) and `b` (n,) of coefficient tuples, `field`
    a `NumberField` or the coefficient list of its minimal polynomial, degree d -- as the system `Atot [x_0; ..; x_(d-1)] = btot` over QQ in the coefficients
    `x = sum_j x_j g^j`: `Atot` an object array (n d, m d) of `Fraction`s, block (k, j) -- rows `n k + i`, columns `m j + c` -- the sum over i of
    `coeff(g^(i+j), k) A_i`; `btot` the list of the coefficients of b, coefficient after coefficient."""
    f = _minpoly_of(field)
    d = len(f) - 1
    Af = _field_matrix(A, d, "convert_system")
    n, m = Af.shape
    bf = _field_matrix([list(b)], d, "convert_system")[0] if len(b) else np.empty(0, dtype=object)
    if bf.shape[0] != n:
        raise ValueError(f"convert_system: b has {bf.shape[0]} entries for {n} rows")
    power = [_field_fold([Fraction(int(t == e)) for t in range(2 * d - 1)], f) for e in range(2 * d - 1)]      # g^e in the basis 1 .. g^(d-1)
    Atot = np.empty((n * d, m * d), dtype=object)
    Atot.fill(Fraction(0))
    for i in range(d):
        for j in range(d):
            for k in range(d):
                ck = power[i + j][k]
                if ck:
                    for r in range(n):
                        for c in range(m):
                            if Af[r, c][i]:
                                Atot[n * k + r, m * j + c] += ck * Af[r, c][i]
    return Atot, [bf[r][k] for k in range(d) for r in range(n)]


def xrational_to_field(x, field) -> list:
    """The reference's `xrational_to_field` (src/rounding.jl:1332-1342): the concatenation `[x_0; ..; x_(d-1)]` of `convert_system` as the list of the
    m = len(x) / d coefficient tuples `(x_0[c], .., x_(d-1)[c])`."""
    d = len(_minpoly_of(field)) - 1
    if len(x) % d:
        raise ValueError(f"xrational_to_field: {len(x)} numbers are no multiple of the degree {d}")
    m = len(x) // d
    return [tuple(Fraction(x[m * j + c]) for j in range(d)) for c in range(m)]


def _planar_matrix(values, rows: int, cols: int, limbs: int) -> np.ndarray:
    """mpmath numbers, row-major -> planar (limbs, rows, cols)"""
    from .mw import to_limbs
    return np.ascontiguousarray(to_limbs(values, limbs).reshape(limbs, rows, cols))


def field_least_squares(Atot, btot, x, field, limbs: int, regularization: float = 1e-30, decimals: int = 40, form: str = "auto", gemm=None, solve=None,
                        device: int = 0) -> list:
    """The reference's `roundx(A, b, x, g, deg)` (src/rounding.jl:537-568) at `limbs` limbs on the device: an approximate solution of the converted system
    `Atot [x_0; ..; x_(d-1)] = btot` of `convert_system` near the numeric solution `x` (m numbers: `Fraction`s or mpmath numbers) of the system over the
    field.  With `Acols = Atot[:, :m]`, `rhs = btot - Acols x` and `B = [Atot_j - g^j Acols]_(j >= 1)` (converted to limbs once) the coefficients
    `y = (x_1, .., x_(d-1))` solve the regularised least-squares problem min |B y - rhs|^2 + reg |y|^2 and `x_0 = x - sum_j g^j x_j`:
      form "primal": `(B^T B + reg I) y = B^T rhs`, order m (d - 1), the reference's form;
      form "dual":   `(B B^T + reg I) z = rhs`, `y = B^T z`, order n d -- the same y for reg > 0;
      form "auto":   the smaller order.
    The Gram matrix, `B^T rhs` and `B^T z` are products of `gemm` (default `mw.gemm_batch`), the solve is `solve` (default `mw.posv`, clrs_mw_posv: the
    system has condition number about 1 / reg).  Returns `[floor(x_0 10^dec) / 10^dec; floor(y 10^dec) / 10^dec]` as `Fraction`s, dec = `decimals`."""
    import mpmath as mp
    from . import mw
    gemm = mw.gemm_batch if gemm is None else gemm
    solve = mw.posv if solve is None else solve
    limbs, d = int(limbs), field.degree
    At = np.asarray(Atot, dtype=object)
    rows, m = At.shape[0], len(x)
    if At.ndim != 2 or At.shape[1] != m * d or len(btot) != rows or d < 2:
        raise ValueError(f"field_least_squares: Atot must be (n d, m d) = (.., {m * d}) with one entry of btot per row and d >= 2, got {At.shape} and {len(btot)}")
    if form not in ("auto", "primal", "dual"):
        raise ValueError(f"field_least_squares: form must be 'auto', 'primal' or 'dual', got {form!r}")
    if not regularization > 0:
        raise ValueError("field_least_squares: the regularization must be positive")
    ncol = m * (d - 1)
    form = ("primal" if ncol <= rows else "dual") if form == "auto" else form
    scale = 10 ** int(decimals)
    with mp.workprec(64 * limbs + 128):
        num = lambda v: mp.mpf(v.numerator) / mp.mpf(v.denominator) if isinstance(v, Fraction) else mp.mpf(v)
        gp = field.power_values(prec=64 * limbs + 128)
        xs = [num(v) for v in x]
        Am = [[num(At[r, c]) if At[r, c] else mp.mpf(0) for c in range(m * d)] for r in range(rows)]
        rhs = [num(btot[r]) - mp.fsum(Am[r][c] * xs[c] for c in range(m) if At[r, c]) for r in range(rows)]
        Bm = [Am[r][m * j + c] - gp[j] * Am[r][c] for r in range(rows) for j in range(1, d) for c in range(m)]
        Bp, rp = _planar_matrix(Bm, rows, ncol, limbs), _planar_matrix(rhs, rows, 1, limbs)
        reg = mp.mpf(regularization)
        order = ncol if form == "primal" else rows
        if order == 0:
            y = []
        else:
            if form == "primal":
                G, v = gemm([(Bp, Bp, None, 1, 0, 1, 0), (Bp, rp, None, 1, 0, 1, 0)], limbs, device=device)
            else:
                (G,), v = gemm([(Bp, Bp, None, 0, 1, 1, 0)], limbs, device=device), rp
            diag = mw.from_limbs(np.ascontiguousarray(G[:, range(order), range(order)]))
            G = np.array(G, dtype=np.float64)
            G[:, range(order), range(order)] = mw.to_limbs([t + reg for t in diag], limbs)
            z, _ = solve(G, v, limbs, device=device)
            if form == "dual":
                (z,) = gemm([(Bp, z, None, 1, 0, 1, 0)], limbs, device=device) if ncol else (np.zeros((limbs, 0, 1)),)
            y = list(mw.from_limbs(np.ascontiguousarray(np.asarray(z)[:, :, 0])))
        x0 = [xs[c] - mp.fsum(gp[j] * y[m * (j - 1) + c] for j in range(1, d)) for c in range(m)]
        return [Fraction(int(mp.floor(v * scale)), scale) for v in x0 + list(y)]


# ---- the system over QQ(g) itself (src/interface.jl:1354-1535 with FF != QQ) ----
def field_array(values, shape=None) -> np.ndarray:
    """a (nested) list whose leaves are coefficient tuples or rationals -> an object array whose ELEMENTS are those leaves (numpy would unpack the tuples)"""
    def leaves(v):
        if isinstance(v, tuple) or not isinstance(v, (list, np.ndarray)):
            return [v], ()
        parts = [leaves(x) for x in v]
        return [y for part in parts for y in part[0]], (len(parts),) + (parts[0][1] if parts else ())
    flat, shp = leaves(values)
    out = np.empty(len(flat), dtype=object)
    for i, v in enumerate(flat):
        out[i] = tuple(Fraction(x) for x in v) if isinstance(v, tuple) else Fraction(v)
    return out.reshape(shp if shape is None else shape)


def _elem(v, d: int) -> tuple:
    """a rational or a coefficient tuple as a tuple of d `Fraction`s"""
    if isinstance(v, tuple):
        if len(v) != d:
            raise ValueError(f"a field element of {len(v)} coefficients in a field of degree {d}")
        return tuple(Fraction(x) for x in v)
    return (Fraction(v),) + (Fraction(0),) * (d - 1)


def _elem_mul(x, y, f) -> tuple:
    d = len(f) - 1
    t = [Fraction(0)] * (2 * d - 1)
    for a in range(d):
        if x[a]:
            for b in range(d):
                t[a + b] += x[a] * y[b]
    return _field_fold(t, f)


def _elem_matrix(M, d: int) -> np.ndarray:
    src = np.asarray(M, dtype=object) if not isinstance(M, np.ndarray) else M
    out = np.empty(src.shape, dtype=object)
    for idx in np.ndindex(*src.shape):
        out[idx] = _elem(src[idx], d)
    return out


def _linear_system_field(problem, Bs, columns, assemble, matmul, device, field):
    """`linear_system` over QQ(g).  Per low-rank block `U = P [lam v]` and `W = P w` are matrices of field elements (`field_matmul`); per constraint they are
    cleared of denominators and their d coefficient planes U_a, W_b are stacked along the term axis: row (p, e), e = 0 .. 2d - 2, of the ONE `assemble` call holds
    the terms (t, a, b) of constraint p with a + b = e, so its entry is the coefficient of g^e, and the 2d - 1 coefficients are folded by the minimal polynomial."""
    f = _minpoly_of(field)
    d = len(f) - 1
    zero = (Fraction(0),) * d
    add = lambda x, y: tuple(u + v for u, v in zip(x, y))
    kept = _kept_rows(problem, Bs, d)
    index = system_index(problem, Bs, field)
    take = list(range(len(index))) if columns is None else [int(c) for c in columns]
    if any(not 0 <= c < len(index) for c in take):
        raise ValueError(f"linear_system: a column outside [0, {len(index)})")
    where = {}
    for pos, c in enumerate(take):
        where.setdefault(c, []).append(pos)
    sizes = [len(cj) for cj in problem.c]
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    A = np.empty((int(row0[-1]), len(take)), dtype=object)
    A.fill(zero)
    first = {}
    for ci, e in enumerate(index):
        first.setdefault(e[0], ci)
    for bi, (j, bl) in enumerate(problem.flat_blocks()):
        P, nk = kept[bi]
        cols = [(a, b) for a in range(nk) for b in range(a, nk)]
        sel = [(t, ab) for t, ab in enumerate(cols) if first.get(bi, 0) + t in where] if nk else []
        if not sel:
            continue
        Pj, n, delta = sizes[j], bl.n, bl.delta
        if bl.high_rank:
            for p, M in bl.entries.get((0, 0), {}).items():
                Me = _elem_matrix(M, d)
                Mt = Me if P is None else transform_field(Me, Bs[bi][1], Bs[bi][2], field, matmul=matmul, device=device)
                for t, (a, b) in sel:
                    v = Mt[a, b] if a == b else add(Mt[a, b], Mt[b, a])
                    for pos in where[first[bi] + t]:
                        A[row0[j] + p, pos] = v
            continue
        terms = [[] for _ in range(Pj)]
        for (r, s_), dct in bl.entries.items():
            for p, e in dct.items():
                for k in range(e.rank):
                    terms[p].append((r, s_, k, e))
        vcols, wcols, owner = [], [], []
        for p in range(Pj):
            terms[p].sort(key=lambda t: t[:3])
            for r, s_, k, e in terms[p]:
                v, w = [zero] * n, [zero] * n
                lam = _elem(e.lam[k], d)
                v[r * delta:(r + 1) * delta] = [_elem_mul(lam, _elem(x, d), f) for x in e.vs[k]]
                w[s_ * delta:(s_ + 1) * delta] = [_elem(x, d) for x in e.ws[k]]
                vcols.append(v); wcols.append(w); owner.append(p)
        T = len(vcols)
        Vf, Wf = np.empty((n, T), dtype=object), np.empty((n, T), dtype=object)
        for t in range(T):
            for i in range(n):
                Vf[i, t], Wf[i, t] = vcols[t][i], wcols[t][i]
        if P is not None and T:
            Vf, Wf = field_matmul(P, Vf, field, matmul=matmul, device=device), field_matmul(P, Wf, field, matmul=matmul, device=device)
        nn = Vf.shape[0]
        rowptr, Uc, Wc, mult = [0], [], [], []
        for p in range(Pj):
            mine = [t for t in range(T) if owner[t] == p]
            lv = _lcm_of(x for t in mine for i in range(nn) for x in Vf[i, t])
            lw = _lcm_of(x for t in mine for i in range(nn) for x in Wf[i, t])
            mult.append(lv * lw)
            for e in range(2 * d - 1):
                for t in mine:
                    for a in range(max(0, e - d + 1), min(d, e + 1)):
                        Uc.append([int(Vf[i, t][a] * lv) for i in range(nn)])
                        Wc.append([int(Wf[i, t][e - a] * lw) for i in range(nn)])
                rowptr.append(len(Uc))
        Ui = np.array(Uc, dtype=object).reshape(len(Uc), nn).T
        Wi = np.array(Wc, dtype=object).reshape(len(Wc), nn).T
        G = np.asarray(assemble(Ui, Wi, rowptr, [ab for _, ab in sel], device=device), dtype=object)
        if G.shape != (Pj * (2 * d - 1), len(sel)):
            raise ArithmeticError(f"linear_system: assemble returned shape {G.shape} for {Pj * (2 * d - 1)} rows and {len(sel)} columns")
        for p in range(Pj):
            for q, (t, _) in enumerate(sel):
                coeffs = [Fraction(int(G[p * (2 * d - 1) + e, q]), mult[p]) for e in range(2 * d - 1)]
                if any(coeffs):
                    v = _field_fold(coeffs, f)
                    for pos in where[first[bi] + t]:
                        A[row0[j] + p, pos] = v
    nY = len(index) - problem.b.size
    for k in range(problem.b.size):
        for pos in where.get(nY + k, ()):
            for j in range(len(sizes)):
                for p in range(sizes[j]):
                    A[row0[j] + p, pos] = _elem(problem.B[j][p, k], d)
    b = [_elem(v, d) for cj in problem.c for v in cj]
    return A, b, [index[c] for c in take]


def _exact_solution_field(problem, result, settings, limbs, transformed, rng, device, batch, lift, reconstruct, matmul, minors, round_batch, assemble, field, gemm,
                          solve, adjugate, primes) -> ExactSolution:
    """`exact_solution` over QQ(g) (src/rounding.jl:1366-1409 with FF a number field): 1. `kernel_vectors(rationalize=True, field=)`; 2.
    `basis_transformations(field=)`; 3. `Yt = P Y P^T`, P = B^T[s:, :] embedded at g, numerically in `limbs` limbs (`gemm`, default `mw.gemm_batch`); 4.
    `select_columns`; 5. `get_rational_system(field=)` and the QQ `project_to_affine_space` on the converted system, `extra += 2` as over QQ; 6.
    `xrational_to_field`; 7. `checkpd_field` of every transformed block (`minors`, `primes`); 8. `undo_transform_field`; 9. the objective as a field element.
    `Y`, `y` and `objective` of the result hold coefficient tuples.  The reduction of kernel vectors over a field is not built: `NotImplementedError` unless
    `settings.reduce_kernelvectors` is false."""
    import mpmath as mp
    from . import mw
    if settings.reduce_kernelvectors:
        raise NotImplementedError("exact_solution: the reduction of kernel vectors over a number field is not built; pass RoundingSettings(reduce_kernelvectors=False)")
    if limbs is None:
        limbs = np.atleast_2d(np.asarray(result.Y)).shape[0]             # the planes the solution carries
    if int(limbs) not in LIMBS:
        raise ValueError(f"exact_solution: field= needs a solution in limbs, or limbs in {LIMBS}")
    gemm = mw.gemm_batch if gemm is None else gemm
    f = _minpoly_of(field)
    d, limbs = len(f) - 1, int(limbs)
    zero = (Fraction(0),) * d
    add = lambda x, y: tuple(u + v for u, v in zip(x, y))
    block_n = problem.block_n
    kernels = kernel_vectors(block_n, result, result, limbs=limbs, settings=settings, device=device, rationalize=True, round_batch=round_batch, field=field)
    Bs = basis_transformations({bi: (int(n), vectors_to_field(k)) for bi, (n, k) in enumerate(zip(block_n, kernels))}, settings, device=device, batch=batch,
                               matmul=matmul, field=field, adjugate=adjugate, primes=primes)
    Yp = np.atleast_2d(np.asarray(result.Y, dtype=np.float64))[:limbs]
    off = np.concatenate([[0], np.cumsum(np.asarray(block_n, dtype=np.int64) ** 2)])
    with mp.workprec(64 * limbs + 128):
        gp = field.power_values(prec=64 * limbs + 128)
        q = lambda v: mp.mpf(v.numerator) / mp.mpf(v.denominator)
        jobs, keys = [], []
        for bi, (Bt, _, s_) in Bs.items():
            n, nk = int(block_n[bi]), int(block_n[bi]) - int(s_)
            if nk == 0:
                continue
            Pm = [mp.fsum(q(c) * g for c, g in zip(_elem(Bt[i, j], d), gp) if c) for i in range(int(s_), n) for j in range(n)]
            Pp = _planar_matrix(Pm, nk, n, limbs)
            Yb = np.zeros((limbs, n, n))
            Yb[:Yp.shape[0]] = np.transpose(Yp[:, off[bi]:off[bi + 1]].reshape(Yp.shape[0], n, n), (0, 2, 1))
            jobs.append((Pp, (Yb + np.transpose(Yb, (0, 2, 1))) / 2, None, 0, 0, 1, 0))
            keys.append((bi, Pp))
        half = gemm(jobs, limbs, device=device) if jobs else []
        full = gemm([(T, Pp, None, 0, 1, 1, 0) for T, (_, Pp) in zip(half, keys)], limbs, device=device) if jobs else []
        Yt = {}
        for (bi, _), M in zip(keys, full):
            vals = mw.from_limbs(np.ascontiguousarray(M.reshape(limbs, -1)))
            Yt[bi] = np.array(list(vals), dtype=object).reshape(M.shape[1], M.shape[2])
        yv = np.atleast_2d(np.asarray(getattr(result, "y", np.zeros(0)), dtype=np.float64))
        y = [mp.fsum(mp.mpf(float(v)) for v in yv[:, k]) for k in range(problem.b.size)]
    index = system_index(problem, Bs, field)
    m = len(index)
    nconstraints = sum(len(cj) for cj in problem.c)
    objective = []
    for bi, (j, bl) in enumerate(problem.flat_blocks()):
        nk = int(block_n[bi]) - int(Bs[bi][2])
        if not nk:
            continue
        l = bi - sum(len(cl) for cl in problem.blocks[:j])
        Ct = transform_field(_elem_matrix(problem.C[j][l], d), Bs[bi][1], Bs[bi][2], field, matmul=matmul, device=device)
        objective += [any(Ct[a, b]) or any(Ct[b, a]) for a in range(nk) for b in range(a, nk)]
    objective += [any(_elem(v, d)) for v in problem.b]
    extra = 0
    while True:
        columns = select_columns(index, settings.redundancyfactor + extra, rng, nconstraints=nconstraints, objective=objective)
        A, rhs, x, cols = get_rational_system(problem, Yt, y, Bs, columns, settings, assemble=assemble, matmul=matmul, device=device, field=field, limbs=limbs,
                                              gemm=gemm, solve=solve)
        x_extra, correct_slacks, finished = project_to_affine_space(A, rhs, settings=settings, rng=rng, device=device, batch=batch, lift=lift,
                                                                    reconstruct=reconstruct, matmul=matmul)
        if finished:
            break
        if len(columns) >= m:
            raise ArithmeticError("exact_solution: the system is inconsistent but all columns were taken")
        extra += 2
    for pos, c in enumerate(cols):
        x[c] += x_extra[pos]
    xf = xrational_to_field(x, field)
    sol_t, free = {}, [zero] * problem.b.size
    for bi, (_, _, s_) in Bs.items():
        nk = int(block_n[bi]) - int(s_)
        sol_t[bi] = np.empty((nk, nk), dtype=object)
    for e, v in zip(index, xf):
        if e[0] == "free":
            free[e[1]] = v
        else:
            sol_t[e[0]][e[1], e[2]] = sol_t[e[0]][e[2], e[1]] = v
    certificates = [checkpd_field(sol_t[bi], field, device=device, minors=minors, primes=primes) for bi in sol_t if sol_t[bi].shape[0]]
    success = bool(correct_slacks) and all(cert.pd for cert in certificates)
    full = [undo_transform_field(sol_t[bi], Bs[bi][1], Bs[bi][2], field, matmul=matmul, device=device) for bi in sorted(sol_t)]
    value = _elem(problem.constant, d)
    for k, v in enumerate(problem.b):
        value = add(value, _elem_mul(_elem(v, d), free[k], f))
    for (j, l), M in zip(((j, l) for j, cl in enumerate(problem.blocks) for l in range(len(cl))), full):
        for a in range(M.shape[0]):
            for b in range(M.shape[0]):
                c = _elem(problem.C[j][l][a, b], d)
                if any(c) and any(M[a, b]):
                    value = add(value, _elem_mul(c, M[a, b], f))
    return ExactSolution(success, [sol_t[bi] for bi in sorted(sol_t)] if transformed else full, free, value, bool(correct_slacks), certificates, Bs)


# ---- find_field: the number field of a solution from minimal polynomials of kernel entries (src/find_field.jl; clrs_mw_minpoly) ---------
MINPOLY_KERNEL_DEGREES = (1, 2, 3, 4)     # what k_mw_minpoly is instantiated for
MINPOLY_POWER_LIMIT = 2.0 ** 22           # FR_V_LIMIT: every power of a number must stay below this


@dataclasses.dataclass
class MinPolySearch:
    """What `minimal_polynomials` returns.  Per number i: `degree[i]` the degree its search closed at (0: none up to `max_degree`); `minpoly[i]` the
    polynomial as Python ints, low to high, primitive, leading coefficient > 0 (None where `degree` is 0).  Per number and tried degree d (column d - 1):
    `status` (the codes of clrs_mw_minpoly; -1 not tried), `rung` (the bits of the rung the number ended at), `err` (the residual there) and `path`
    (0 the kernel, 1 `relations`, -1 not tried).  `rel[i][d - 1]`: the relation as found, or None."""
    degree: np.ndarray
    minpoly: list
    status: np.ndarray
    rung: np.ndarray
    err: np.ndarray
    path: np.ndarray
    rel: list


def _minpoly_call_device(limbs, deg, count, v, plane, bits, errbound, nd, device=0):
    """one call of clrs_mw_minpoly: returns (rel (nd, deg + 1, plane) int32, status, rung, err, info (2, plane))"""
    p1 = max(plane, 1)
    rel, status, rung = np.zeros((nd, deg + 1, p1), np.int32), np.zeros(p1, np.int32), np.zeros(p1, np.int32)
    err, info = np.zeros(p1), np.zeros((2, p1), np.int32)
    pi, pd = (lambda a: a.ctypes.data_as(_lib.p_i32)), (lambda a: a.ctypes.data_as(_lib.p_d))
    _lib.check(_lib.load().clrs_mw_minpoly(int(device), int(limbs), int(deg), int(count), pd(v), int(plane), int(bits), float(errbound), int(nd), pi(rel), pi(status),
                                           pi(rung), pd(err), pi(info)))
    return rel, status, rung, err, info


def _primitive(a) -> list:
    """an integer relation as a polynomial: divided by its content, leading coefficient > 0"""
    a = [int(x) for x in a]
    g = _gcd_of(a) or 1
    sign = -1 if a[-1] < 0 else 1
    return [sign * x // g for x in a]


def minpoly_relations_lll(values, degree: int, limbs: int, errbound: float = 1e-15, bits: Optional[int] = None, device: int = 0, lll=None):
    """The contract of one clrs_mw_minpoly call through `lll_batch` (clrs_zz_lll), as `field_relations_lll` is for `round_to_field`: per rung p = 1, 6,
    11, .. one batched call over the numbers still open, each on [I | floor(2^p (1, v, .., v^degree))] from scratch; the first row is accepted on the host, in
    mpmath, when |sum a_k v^k| < errbound.  Degrees 1 .. 8.  Returns (rel (count, degree + 1) Python integers low to high, status, rung, err) with the
    statuses of the kernel (5: a_0 = 0 or a_degree = 0).  The rescue of `minimal_polynomials` for statuses 3 and 4, its path for degrees 5 .. 8, and an
    independent device-side cross-check of k_mw_minpoly.  `lll` replaces `lll_batch` (the tests' host build)."""
    import mpmath as mp
    from .mw import from_limbs
    limbs, deg = int(limbs), int(degree)
    if limbs not in LIMBS:
        raise ValueError(f"minpoly_relations_lll: limbs must be one of {LIMBS}, got {limbs}")
    if not 1 <= deg <= FIELD_LLL_MAX_DEGREE:
        raise ValueError(f"minpoly_relations_lll: the degree must lie in [1, {FIELD_LLL_MAX_DEGREE}], got {deg}")
    bits = 100 * deg if bits is None else int(bits)
    if not errbound > 0 or bits < 1:
        raise ValueError("minpoly_relations_lll: errbound must be positive and bits at least 1")
    lll = lll_batch if lll is None else lll
    v, count = _field_values(values, limbs, "minpoly_relations_lll")
    D, P = deg + 1, field_top_bits(bits, limbs)
    with mp.workprec(64 * limbs + 128):
        finite = np.all(np.isfinite(v[:, :count]), axis=0)
        us = [[mp.mpf(x) ** k for k in range(D)] if finite[i] else None for i, x in enumerate(from_limbs(v[:, :count]))]
        large = [u is not None and any(abs(x) >= MINPOLY_POWER_LIMIT for x in u) for u in us]
        rel, status, rung, err = _relation_ladder([None if big else u for u, big in zip(us, large)], D, P, errbound, lll, device)
    for i in range(count):
        if large[i]:
            status[i] = FIELD_OVERFLOW
        elif status[i] == FIELD_FOUND and (rel[i, 0] == 0 or rel[i, deg] == 0):
            status[i] = FIELD_NO_FIELD
    return rel, status, rung, err


def minimal_polynomials(values, limbs: int, max_degree: int = 4, bits: Optional[int] = None, errbound: float = 1e-15, max_coeff: int = 10 ** 5, device: int = 0,
                        call=None, relations=None, nd: Optional[int] = None, min_degree: int = 1) -> MinPolySearch:
    """Minimal polynomials of numbers on the device (clrs_mw_minpoly, one lane per number): `values` planar (planes <= limbs, count) or fp64 (count,).
    Degree by degree d = `min_degree`, .., `max_degree`, one call over the numbers still open: per number the first rung p = 1, 6, 11, .. <= min(bits,
    53 limbs - 16) at which the first row a of the LLL-reduced basis of [I | floor(2^p (1, v, .., v^d))] has |sum a_k v^k| < errbound.  A number is closed at
    the first d whose relation is found (status 0) with max |a_k| <= max_coeff (the inner loop of the reference's select_vals, src/find_field.jl:23-40);
    a number that is not finite is closed with degree 0 at once, and one that is 0 to errbound (status 5 at degree 1: 0 + a_1 v ~ 0) with the polynomial
    x.  Status 5 at any other degree is "nothing at this degree".  `bits` defaults to 100 max_degree.  Degrees 1 .. 4 run in the kernel; numbers it ends with
    status 3 or 4, and degrees 5 .. 8, go to `relations` (default `minpoly_relations_lll`; False: nowhere, and max_degree > 4 is then a ValueError).  `nd`:
    the base-2^24 digits per lattice entry (default `field_default_digits`); `call` replaces the device call (the tests' host build)."""
    limbs, max_degree, min_degree = int(limbs), int(max_degree), int(min_degree)
    if limbs not in LIMBS:
        raise ValueError(f"minimal_polynomials: limbs must be one of {LIMBS}, got {limbs}")
    if not 1 <= min_degree <= max_degree <= FIELD_LLL_MAX_DEGREE:
        raise ValueError(f"minimal_polynomials: 1 <= min_degree <= max_degree <= {FIELD_LLL_MAX_DEGREE} is required, got {min_degree} and {max_degree}")
    if relations is False and max_degree > MINPOLY_KERNEL_DEGREES[-1]:
        raise ValueError(f"minimal_polynomials: the kernel takes degrees {MINPOLY_KERNEL_DEGREES}, got max_degree = {max_degree}")
    bits = 100 * max_degree if bits is None else int(bits)
    if not errbound > 0 or bits < 1:
        raise ValueError("minimal_polynomials: errbound must be positive and bits at least 1")
    relations = minpoly_relations_lll if relations is None else relations
    call = _minpoly_call_device if call is None else call
    v, count = _field_values(values, limbs, "minimal_polynomials")
    nd = field_default_digits(bits, limbs) if nd is None else int(nd)
    out = MinPolySearch(np.zeros(count, np.int32), [None] * count, np.full((count, max_degree), -1, np.int32), np.zeros((count, max_degree), np.int32),
                        np.zeros((count, max_degree)), np.full((count, max_degree), -1, np.int32), [[None] * max_degree for _ in range(count)])
    opened = np.arange(count)
    for d in range(min_degree, max_degree + 1):
        if not opened.size:
            break
        m = opened.size
        sub = np.ascontiguousarray(v[:, opened])
        if d in MINPOLY_KERNEL_DEGREES:
            reld, status, rung, err, _ = call(limbs, d, m, sub, m, bits, float(errbound), nd, device=device)
            status, rung, err, path = status[:m].copy(), rung[:m].copy(), err[:m].copy(), np.zeros(m, np.int32)
            rel = planes_to_ints(reld[:, :, :m]).T.copy()
            again = np.flatnonzero((status == FIELD_STEER) | (status == FIELD_OVERFLOW))
            if again.size and relations is not False:
                r = relations(sub[:, again], d, limbs, errbound=errbound, bits=bits, device=device)
                rel[again], status[again], rung[again], err[again], path[again] = r[0], r[1], r[2], r[3], 1
        else:
            rel, status, rung, err = relations(sub, d, limbs, errbound=errbound, bits=bits, device=device)
            path = np.ones(m, np.int32)
        out.status[opened, d - 1], out.rung[opened, d - 1], out.err[opened, d - 1], out.path[opened, d - 1] = status, rung, err, path
        keep = []
        for t, i in enumerate(opened):
            a = [int(x) for x in rel[t]]
            out.rel[i][d - 1] = a if status[t] in (FIELD_FOUND, FIELD_NO_FIELD) else None
            if status[t] == FIELD_FOUND and max(abs(x) for x in a) <= max_coeff:
                out.degree[i], out.minpoly[i] = d, _primitive(a)
            elif d == 1 and status[t] == FIELD_NO_FIELD and a[0] == 0:             # (0 + a_1 v ~ 0: v is 0 to this accuracy, with minimal polynomial x)
                out.degree[i], out.minpoly[i] = 1, [0, 1]
            elif status[t] != FIELD_NOT_FINITE:
                keep.append(i)
        opened = np.asarray(keep, dtype=np.int64)
    return out


def _solution_blocks(block_n_or_sdp, dualsol, primalsol, limbs, what):
    """(block sizes, limbs, X, Y planar) of a solution, as `kernel_vectors` reads its arguments"""
    if hasattr(block_n_or_sdp, "block_n"):
        block_n = block_n_or_sdp.block_n
    elif hasattr(block_n_or_sdp, "blocks"):
        from .sdp import flatten
        block_n = flatten(block_n_or_sdp).block_n
    else:
        block_n = block_n_or_sdp
    block_n = np.ascontiguousarray(block_n, np.int32).reshape(-1)
    primalsol = dualsol if primalsol is None else primalsol
    if limbs is None:
        planes = max(np.asarray(a).shape[0] if np.asarray(a).ndim == 2 else 1 for a in (dualsol.X, primalsol.Y))
        limbs = 5 if planes == 1 else planes
    limbs = int(limbs)
    if limbs not in LIMBS:
        raise ValueError(f"{what}: limbs must be one of {LIMBS}, got {limbs}")
    plane = int(np.sum(block_n.astype(np.int64) ** 2))
    return block_n, limbs, _planes(dualsol.X, limbs, plane, "X"), _planes(primalsol.Y, limbs, plane, "Y")


def select_vals(block_n_or_sdp, dualsol, primalsol=None, limbs: Optional[int] = None, valbound: float = 1e-15, errbound: float = 1e-15, sizebound: float = 1e6,
                device: int = 0, batch=None):
    """The numbers `find_field` looks for minimal polynomials of (the reference's select_vals, src/find_field.jl:1-22): one generic entry per kernel vector
    of every block.  ONE `kernel_vectors_batch` call without the checks of `kernel_vectors` (tau = errbound, use_dual, dual_max = sizebound); its echelon
    form [I W] is the reference's Rp = R11^-1 R (dual branch: the row space of X_b; primal branch: the kernel of Y_b, where the reference takes an SVD), over
    the pivots of the diagonally pivoted elimination instead of those of a column-norm QR.  Per vector the first entry outside the identity part, in `perm`
    order, whose head exceeds `valbound` in magnitude.  Returns (values planar (limbs, m), origins: m tuples (block, vector, row))."""
    if not valbound >= 0 or not errbound > 0 or not sizebound > 0:
        raise ValueError("select_vals: valbound must not be negative, errbound and sizebound must be positive")
    block_n, limbs, X, Y = _solution_blocks(block_n_or_sdp, dualsol, primalsol, limbs, "select_vals")
    batch = kernel_vectors_batch if batch is None else batch
    out = batch(block_n, X, Y, limbs, float(errbound), True, float(sizebound), device=device)
    cols, origins = [], []
    for b, k in enumerate(out):
        n, perm = int(block_n[b]), np.asarray(k.perm)
        free = perm[k.rank:] if k.branch == "dual" else perm[:k.rank]           # (the rows of W: everything outside the identity part)
        vec = np.asarray(k.vectors)
        for c in range(k.count):
            row = next((int(r) for r in free if abs(vec[0, int(r), c]) > valbound), None)
            if row is not None:
                cols.append(vec[:, row, c])
                origins.append((b, c, row))
    values = np.ascontiguousarray(np.stack(cols, axis=1)) if cols else np.zeros((limbs, 0))
    return values, origins


def _refined_field(minpoly, near, limbs: int) -> NumberField:
    """QQ(g) with g the real root of `minpoly` nearest the numeric value `near`, at 64 limbs + 128 bits (mpmath: all roots, then Newton on the chosen one).
    `ArithmeticError` when no root is real or the nearest real root is not unique at that accuracy."""
    import mpmath as mp
    prec = 64 * int(limbs) + 128
    c = [int(x) for x in minpoly]
    with mp.workprec(prec + 64):
        near = mp.mpf(near)
        if len(c) == 2:
            return NumberField(c, mp.mpf(-c[0]) / c[1], prec=prec)
        roots = mp.polyroots([mp.mpf(x) for x in reversed(c)], maxsteps=500, extraprec=2 * prec)
        scale = max(1, max(abs(r) for r in roots))
        real = sorted((mp.re(r) for r in roots if abs(mp.im(r)) <= mp.ldexp(scale, -prec // 2)), key=lambda r: abs(r - near))
        if not real:
            raise ArithmeticError("find_field: the minimal polynomial of the generator has no real root")
        if len(real) > 1 and abs(real[1] - near) - abs(real[0] - near) <= mp.ldexp(scale, -prec // 2):
            raise ArithmeticError("find_field: the real root of the minimal polynomial nearest the generator is not unique")
        g = real[0]
        for _ in range(8):                                                       # Newton: the root to the working precision
            f, df = mp.polyval(list(reversed(c)), g, derivative=True)
            if df == 0:
                raise ArithmeticError("find_field: the generator is a multiple root of its minimal polynomial")
            g = g - f / df
        return NumberField(c, g, prec=prec)


def find_common_minpoly(generators, limbs: int, max_coeff: int = 10 ** 5, bits: Optional[int] = None, errbound: float = 1e-15, max_degree: int = 4, device: int = 0,
                        call=None, relations=None, round_call=None, round_relations=None) -> NumberField:
    """One field that holds every generator (the loop of the reference's find_common_minpoly, src/find_field.jl:46-84).  `generators`: tuples (v, degree,
    minpoly) with v the limbs of a number (1-d fp64, at most `limbs` long) or an mpmath number, and its minimal polynomial as `minimal_polynomials` gives
    it.  Starts from the generator of largest degree with the smallest sum |coeffs| (ties: the first); g is refined at once to the real root of its minimal
    polynomial nearest the numeric value, so `decompose(v, g, d)` is `round_to_field` on a `NumberField` (accepted when found with every |a| < max_coeff).
    All remaining generators are decomposed against the current g in one batched call, and again only after g changed.  A generator that does not
    decompose extends the field: g <- g + v, and `minimal_polynomials` looks at degrees max(d, d_v) .. d + d_v; `ArithmeticError` when that range leaves
    `max_degree`.  A generator of larger degree than g in which g decomposes replaces g.  No generators: the degree-1 field `NumberField([-1, 1], 1)`.
    `call`, `relations`: those of `minimal_polynomials`; `round_call`, `round_relations`: `call` and `relations` of `round_to_field`."""
    import mpmath as mp
    from .mw import from_limbs, to_limbs
    limbs, max_degree = int(limbs), int(max_degree)
    bits = 100 * max_degree if bits is None else int(bits)
    prec = 64 * limbs + 128

    def number(v):
        if isinstance(v, (np.ndarray, list, tuple)):
            return from_limbs(np.asarray(v, np.float64).reshape(-1, 1))[0]
        return mp.mpf(v)

    with mp.workprec(prec):
        gens = [(+number(v), int(d), [int(x) for x in poly]) for v, d, poly in generators]
        gens = [g for g in gens if g[1] >= 2]
        if not gens:
            return NumberField([-1, 1], 1)
        start = max(range(len(gens)), key=lambda i: (gens[i][1], -sum(abs(x) for x in gens[i][2]), -i))
        g, d, poly = gens[start]
        field = _refined_field(poly, g, limbs)
        rest = [x for i, x in enumerate(gens) if i != start]

        def decomposes(values, fld):
            r = round_to_field(to_limbs(values, limbs), fld, limbs, errbound=errbound, bits=bits, device=device, call=round_call, relations=round_relations)
            return [r.status[i] == FIELD_FOUND and all(abs(int(x)) < max_coeff for x in r.rel[i]) for i in range(len(values))]

        while rest:
            small = [x for x in rest if x[1] <= d]
            ok = dict(zip((id(x) for x in small), decomposes([x[0] for x in small], field))) if small else {}
            changed = False
            for pos, x in enumerate(rest):
                v, dv, pv = x
                if dv <= d and ok[id(x)]:
                    continue
                if dv > d:                                                       # g may lie in QQ(v)
                    fv = _refined_field(pv, v, limbs)
                    if decomposes([field.g], fv)[0]:
                        g, d, poly, field = v, dv, pv, fv
                        rest, changed = rest[pos + 1:], True
                        break
                lo, hi = max(d, dv), d + dv
                if hi > max_degree:
                    raise ArithmeticError("find_field: the common field has degree above max_degree")
                g = field.g + v
                s = minimal_polynomials(to_limbs([g], limbs), limbs, max_degree=hi, bits=bits, errbound=errbound, max_coeff=max_coeff - 1, device=device,
                                        call=call, relations=relations, min_degree=lo)
                if s.degree[0] == 0:
                    raise ArithmeticError("find_field: no minimal polynomial of the extended generator was found")
                d, poly = int(s.degree[0]), s.minpoly[0]
                field = _refined_field(poly, g, limbs)
                rest, changed = rest[pos + 1:], True
                break
            if not changed:
                break
        return field


def find_field(block_n_or_sdp, dualsol, primalsol=None, max_degree: int = 4, valbound: float = 1e-15, errbound: float = 1e-15, bits: Optional[int] = None,
               max_coeff: int = 10 ** 5, limbs: Optional[int] = None, device: int = 0, batch=None, call=None, relations=None, round_call=None,
               round_relations=None) -> NumberField:
    """Heuristically the number field the kernel of a solution is defined over (the reference's find_field, src/find_field.jl:97-108; DESIGN.md section
    27): `select_vals` -> `minimal_polynomials` (on the device, clrs_mw_minpoly) -> `find_common_minpoly`.  Returns a `NumberField` whose generator is
    known to 64 limbs + 128 bits, ready for `kernel_vectors(field=...)`, `basis_transformations(field=...)`, `exact_solution(field=...)`; with no generator
    of degree >= 2 the degree-1 field `NumberField([-1, 1], 1)`, which those route to the path over QQ.  `bits` defaults to 100 max_degree.  `batch`: the
    device call of `select_vals`; `call`, `relations`, `round_call`, `round_relations`: those of `find_common_minpoly`."""
    block_n, limbs, _, _ = _solution_blocks(block_n_or_sdp, dualsol, primalsol, limbs, "find_field")
    bits = 100 * int(max_degree) if bits is None else int(bits)
    values, _ = select_vals(block_n, dualsol, primalsol, limbs=limbs, valbound=valbound, errbound=errbound, device=device, batch=batch)
    s = minimal_polynomials(values, limbs, max_degree=max_degree, bits=bits, errbound=errbound, max_coeff=max_coeff, device=device, call=call, relations=relations)
    gens = [(values[:, i], int(s.degree[i]), s.minpoly[i]) for i in range(values.shape[1]) if s.degree[i] >= 2]
    return find_common_minpoly(gens, limbs, max_coeff=max_coeff, bits=bits, errbound=errbound, max_degree=max_degree, device=device, call=call,
                               relations=relations, round_call=round_call, round_relations=round_relations)


def to_field(values, field: NumberField, limbs: Optional[int] = None, bits: int = 100, errbound: float = 1e-15, device: int = 0, call=None, relations=None) -> list:
    """Numbers as elements of `field` (the reference's to_field, src/find_field.jl:124-129): `round_to_field`, returning per number the tuple of
    `Fraction`s (x_0, .., x_(deg-1)), value = sum_k x_k g^k.  `values`: planar limbs, fp64, or a sequence of mpmath numbers; `limbs` defaults to the planes of
    a planar input, else 5.  `ValueError` "clindep failed to find a relation" where a value has no relation.  A field of degree 1 goes through `rationalize`."""
    from .mw import to_limbs
    a = np.asarray(values)
    if a.dtype == object:
        limbs = 5 if limbs is None else int(limbs)
        v = to_limbs(a.reshape(-1), limbs)
    else:
        a = np.asarray(values, dtype=np.float64)
        a = a.reshape(1, -1) if a.ndim <= 1 else a
        limbs = (a.shape[0] if a.shape[0] in LIMBS else 5) if limbs is None else int(limbs)
        v = a
    if field.degree == 1:
        num, den, status, _ = rationalize(v, limbs, errbound=errbound, device=device)
        if np.any(status != 0):
            raise ValueError(f"{CLINDEP_MESSAGE}: value {int(np.flatnonzero(status != 0)[0])} (status {int(status[status != 0][0])})")
        return [(Fraction(int(n), int(q)),) for n, q in zip(num, den)]
    r = round_to_field(v, field, limbs, errbound=errbound, bits=bits, device=device, call=call, relations=relations)
    bad = np.flatnonzero(r.status != FIELD_FOUND)
    if bad.size:
        raise ValueError(f"{CLINDEP_MESSAGE}: value {int(bad[0])} (status {int(r.status[bad[0]])})")
    return [tuple(r.coeffs[i]) for i in range(r.coeffs.shape[0])]

"""CPU side of the kernel vectors of solution blocks (clrs_amd.rounding, clrs_mw_kernel_vectors): the Python layer on the 256-bit oracle's solutions with an
mpmath stand-in for the device call (the package has no CPU implementation of it), the errors it raises, the scatter's index map compiled for the host
against a Python restatement, and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clrs_amd
from clrs_amd import _lib
from clrs_amd.rounding import KernelVectorError, RoundingSettings, kernel_vectors, vectors_to_mp
from tests import kernel_vectors_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sol:
    def __init__(self, X, Y):
        self.X, self.Y = X, Y


@pytest.fixture(scope="module")
def oracle_solutions(oracle_built):
    """name -> (flat, solution of the 256-bit oracle at gap 1e-30: X and Y rounded to fp64), solved once"""
    from oracle.oracle import Oracle
    out = {}
    for name in ku.RANKS:
        f = ku.problem(name)
        r = Oracle(f, mp_bits=256).solvesdp(duality_gap_threshold=1e-30)
        assert r["error_code"] == 0, name
        out[name] = (f, _Sol(r["X"], r["Y"]))
    return out


@pytest.mark.parametrize("name", list(ku.RANKS))
def test_python_layer_on_oracle_solutions(name, oracle_solutions):
    f, sol = oracle_solutions[name]
    assert [int(n) for n in f.block_n] and len(f.block_n) == len(ku.RANKS[name])
    dual = kernel_vectors(f, sol, sol, limbs=5, check_dimensions=True, batch=ku.host_batch)
    print(name, "branches", [k.branch for k in dual], "largest residual", max([float(np.max(k.resid_max)) for k in dual if k.count] + [0.0]))
    assert all(k.branch == "dual" for k in dual)
    assert [k.count for k in dual] == ku.RANKS[name] and [k.rank for k in dual] == ku.RANKS[name]
    assert all(np.all(k.resid_max < 1e-10) for k in dual)
    assert all(k.vectors.shape == (5, int(n), k.count) for k, n in zip(dual, f.block_n))
    primal = kernel_vectors(f.block_n, sol, None, limbs=5, settings=RoundingSettings(kernel_use_dual=False), check_dimensions=True, batch=ku.host_batch)
    assert all(k.branch == "primal" for k in primal)
    assert [k.count for k in primal] == [k.count for k in dual]
    assert [k.rank for k in primal] == [int(n) - c for n, c in zip(f.block_n, ku.RANKS[name])]
    assert all(np.all(k.resid_max < 1e-10) for k in primal)
    # mpmath numbers: one list of n per vector, the heads those of the planes
    for k in dual:
        vs = vectors_to_mp(k)
        assert len(vs) == k.count and all(len(v) == k.vectors.shape[1] for v in vs)
        assert all(float(v[i]) == k.vectors[0, i, c] for c, v in enumerate(vs) for i in range(len(v)))


def test_settings_defaults_are_the_references():
    s = RoundingSettings()
    assert (s.kernel_errbound, s.kernel_round_errbound, s.kernel_use_dual) == (1e-10, 1e-15, True)
    assert clrs_amd.kernel_vectors is kernel_vectors and clrs_amd.rounding.RoundingSettings is RoundingSettings


def test_large_dual_block_takes_the_primal_branch():
    """max |X_b| > 1 / sqrt(kernel_round_errbound) (src/rounding.jl:581): that block alone is taken from Y"""
    X = np.concatenate([np.diag([1.0, 0.0]).reshape(-1), np.diag([1e8, 0.0]).reshape(-1)])
    Y = np.concatenate([np.diag([0.0, 1.0]).reshape(-1)] * 2)
    out = kernel_vectors([2, 2], _Sol(X, Y), limbs=4, check_dimensions=True, batch=ku.host_batch)
    assert [k.branch for k in out] == ["dual", "primal"] and [k.count for k in out] == [1, 1]
    assert all(np.array_equal(k.vectors[0, :, 0], [1.0, 0.0]) for k in out)


def test_raises_on_a_vector_that_is_not_in_the_kernel():
    X, Y = np.diag([1.0, 0.0]).reshape(-1), np.eye(2).reshape(-1)
    with pytest.raises(KernelVectorError, match="wrong vector detected"):
        kernel_vectors([2], _Sol(X, Y), limbs=5, batch=ku.host_batch)


def test_check_dimensions_raises_where_both_blocks_are_full_rank():
    sol = _Sol(np.eye(3).reshape(-1), np.eye(3).reshape(-1))
    primal = RoundingSettings(kernel_use_dual=False)
    out = kernel_vectors([3], sol, limbs=5, settings=primal, batch=ku.host_batch)          # Y has full rank: no vectors, nothing to object to
    assert out[0].count == 0 and out[0].rank == 3
    with pytest.raises(KernelVectorError, match="wrong vector detected"):
        kernel_vectors([3], sol, limbs=5, settings=primal, check_dimensions=True, batch=ku.host_batch)
    with pytest.raises(KernelVectorError, match="wrong vector detected"):                   # dual branch: the unit vectors are no kernel vectors of Y = I
        kernel_vectors([3], sol, limbs=5, check_dimensions=True, batch=ku.host_batch)


def test_arguments_are_checked():
    sol = _Sol(np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError, match="limbs"):
        kernel_vectors([2], sol, limbs=7, batch=ku.host_batch)
    with pytest.raises(ValueError, match="per limb plane"):
        kernel_vectors([3], sol, limbs=5, batch=ku.host_batch)
    # planes beyond `limbs` are cut, fewer are padded with zeros (as the warm start of solvesdp_mw does)
    seen = []

    def spy(block_n, X, Y, limbs, *a, **kw):
        seen.append((X.shape, Y.shape))
        return ku.host_batch(block_n, X, Y, limbs, *a, **kw)
    kernel_vectors([2], _Sol(np.zeros((6, 4)), np.zeros(4)), limbs=4, batch=spy)
    assert seen == [((4, 4), (4, 4))]


@pytest.mark.parametrize("branch", ["dual", "primal"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_index_map_of_the_scatter_against_its_restatement(n, branch):
    """kv_entry (compiled with g++) for every (vector, position) of blocks with ranks 0, 1 and n under a random permutation: the row it names, and zero /
    one / +-W[c, a] as the restatement places them; then the kernel's loop on the host: n * count stores, every entry of n x count, nothing else."""
    L = ku.host_lib()
    rng = np.random.default_rng(10 * n + (branch == "dual"))
    code = 1 if branch == "dual" else 0
    for r in sorted({0, 1, n}):
        perm = np.ascontiguousarray(rng.permutation(n), np.int32)
        count = r if branch == "dual" else n - r
        # W[c, a] = 1000 + 10 c + a names its own place; a symbolic restatement from it
        Wsym = np.array([[1000.0 + 10 * c + a for a in range(n - r)] for c in range(r)]).reshape(r, n - r)
        want = ku.restate_vectors(branch, perm, r, Wsym)
        for v in range(count):
            for j in range(n):
                row, widx = C.c_int(-5), C.c_long(-5)
                f = L.mw_kv_entry(code, perm.ctypes.data_as(_lib.p_i32), r, v, j, C.byref(row), C.byref(widx))
                assert row.value == perm[j] and f in (-1, 0, 1)
                if widx.value < 0:
                    got = float(f)
                else:
                    c, a = widx.value % r, widx.value // r                  # column-major r x (n - r)
                    assert 0 <= widx.value < r * (n - r)
                    got = f * Wsym[c, a]
                assert got == want[row.value, v], (branch, n, r, v, j)
        K = 4
        W = rng.standard_normal((K, r, n - r))
        Wcm = np.ascontiguousarray(np.transpose(W, (0, 2, 1)).reshape(K, -1)) if r * (n - r) else np.zeros((K, 1))
        V = np.full((K, max(n * count, 1) + 3), -7.25)                        # three sentinels behind every plane
        stores = L.mw_kv_scatter_host(K, code, n, r, perm.ctypes.data_as(_lib.p_i32), Wcm.ctypes.data_as(_lib.p_d), Wcm.shape[1], V.ctypes.data_as(_lib.p_d))
        assert stores == n * count
        # (the host loop treats V as planar with plane n * count: the sentinels are behind the last plane)
        flatV = V.reshape(-1)
        got = np.transpose(flatV[:K * n * count].reshape(K, count, n), (0, 2, 1))
        assert np.array_equal(got, ku.restate_vectors(branch, perm, r, W))
        assert np.all(flatV[K * n * count:] == -7.25)


def test_maximum_keeps_a_nan():
    L = ku.host_lib()
    assert L.mw_kv_max(1.0, 2.0) == 2.0 and L.mw_kv_max(2.0, 1.0) == 2.0 and L.mw_kv_max(0.0, 0.0) == 0.0
    assert np.isnan(L.mw_kv_max(1.0, float("nan"))) and np.isnan(L.mw_kv_max(float("nan"), 1.0))


def test_lib_binds_clrs_mw_kernel_vectors_with_the_headers_types():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clrs_hip.h")).read(), flags=re.S)
    ret, args = re.search(r"^\s*(\w+)\s+clrs_mw_kernel_vectors\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M).groups()
    table = {"int": C.c_int, "double": C.c_double, "const double *": _lib.p_d, "double *": _lib.p_d, "const int32_t *": _lib.p_i32, "int32_t *": _lib.p_i32}
    names = [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")]
    assert names == ["device", "limbs", "nblk", "n", "X", "Y", "plane", "tau", "use_dual", "dual_max", "branch", "perm", "rank", "count", "V", "resid_max",
                     "v_max", "pivot_resid"]
    want = [table[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
    assert ret == "int" and _lib.SYMBOLS["clrs_mw_kernel_vectors"] == (C.c_int, want)
    from clrs_amd import rounding
    assert callable(rounding.kernel_vectors_batch)
    jl = open(os.path.join(ROOT, "julia", "ClusteredLowRankHIP", "src", "ClusteredLowRankHIP.jl")).read()
    assert ":clrs_mw_kernel_vectors" in jl and "function kernel_vectors(" in jl

"""clrs_amd -- MI355X-native hot path of ClusteredLowRankSolver.jl (Schur assembly + block-Cholesky
solve of the interior-point normal equations), behind a C ABI (include/clrs_hip.h).

Import through the repo-root shim:  `import clrs_amd`.
"""
from . import sdp  # noqa: F401
from .sdp import Block, ClusteredLowRankSDP, HiLo, LowRankMat, flatten  # noqa: F401
from . import rounding  # noqa: F401
from .rounding import KernelVectorError, RoundingSettings, kernel_vectors, rationalize, vectors_to_fractions, vectors_to_mp  # noqa: F401

__all__ = ["sdp", "Block", "ClusteredLowRankSDP", "HiLo", "LowRankMat", "flatten", "rounding", "KernelVectorError", "RoundingSettings", "kernel_vectors",
           "vectors_to_mp", "rationalize", "vectors_to_fractions"]

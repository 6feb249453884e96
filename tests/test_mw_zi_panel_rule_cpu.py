"""CPU test (no GPU) of how k_mwi_Zi is launched: the host-only rule csrc/clrs_mw_zi_panels.h::mw_zi_panels, compiled with g++ through
tests/mw_host/mw_zi_panels_host.cpp, against the kernel's own panel arithmetic (restated in that file from mwi_Zi_body) and against the rule of the
wide form written out here as it stood before the narrow form existed.

`pc` below is the rule's column count of a panel, max(1, (T / 8) / n): what fills one pass of T threads at eight lanes per entry.  The wide form caps
the number of panels at 320 / NB, so with many blocks its panels are wider than `pc` and take several passes -- that is the old launch, kept as it was;
the narrow form is refused instead of capped."""
import ctypes as C
import functools
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mw_host", "mw_zi_panels_host.cpp")
_LIB = os.path.join(_HERE, "mw_host", "libmw_zi_panels_host.so")
_HDR = os.path.join(_HERE, "..", "clusteredlowranksolver.jl_amd", "csrc", "clrs_mw_zi_panels.h")

SIDES = range(1, 25)
BLOCKS = (1, 4, 19, 64)
K = 5


@functools.lru_cache(maxsize=None)
def host_lib():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, _SRC], check=True)
    L = C.CDLL(_LIB)
    L.mwz_rule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    L.mwz_rule.restype = None
    L.mwz_kernel_panel.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_long)]
    L.mwz_kernel_panel.restype = None
    return L


def rule(n, NB, allow_narrow):
    out = (C.c_long * 5)()
    host_lib().mwz_rule(n, NB, K, int(allow_narrow), out)
    return dict(zip(("zs", "threads", "pc", "narrow", "sm"), out))


def panel(n, zs, y, threads):
    out = (C.c_long * 5)()
    host_lib().mwz_kernel_panel(n, zs, y, threads, K, out)
    return dict(zip(("c0", "pc", "pc0", "passes", "lds_doubles"), out))


def wide_zs(n, NB):
    """the launch before the narrow form: MW_PT = 512 threads, panels of one pass unless 320 / NB caps them, at least four panels"""
    pc = max(1, 64 // n)
    want = -(-n // pc)
    old_rule = max(4, (n + 7) // 8)
    return max(old_rule, min(want, 320 // NB))


def test_the_header_includes_nothing_from_hip():
    text = open(_HDR).read()
    assert "hip" not in "".join(l for l in text.splitlines() if l.lstrip().startswith("#include")).lower()
    assert host_lib().mwz_lanes() == 8


@pytest.mark.parametrize("allow_narrow", [0, 1], ids=["wide", "narrow"])
@pytest.mark.parametrize("NB", BLOCKS)
def test_panels_cover_every_column_once_and_fit_the_lds_of_the_launch(NB, allow_narrow):
    for n in SIDES:
        r = rule(n, NB, allow_narrow)
        T = r["threads"]
        assert T in (256, 512) and r["zs"] >= 1
        assert r["pc"] == max(1, (T // 8) // n)
        assert r["pc"] * n * 8 <= T                         # the rule's panel is one pass of the workgroup (n <= 24 < T / 8)
        one_pass_rule = r["zs"] >= -(-n // r["pc"])            # (the wide form's cap 320 / NB is the one way to fewer panels than that)
        if r["narrow"]:
            assert one_pass_rule
        for m in range(1, n + 1):                             # every block of the context, sides up to the largest, is launched with the same zs
            seen = [0] * m
            for y in range(r["zs"]):
                k = panel(m, r["zs"], y, T)
                assert 0 <= k["pc"] <= k["pc0"] and (k["pc"] == 0 or k["c0"] + k["pc"] <= m)
                for c in range(k["c0"], k["c0"] + k["pc"]):
                    seen[c] += 1
                assert k["lds_doubles"] * 8 <= r["sm"], (n, m, NB, T)
                if m == n:
                    assert k["lds_doubles"] * 8 == r["sm"]          # sm_Zi is exactly what the largest block's workgroups index
                if one_pass_rule:
                    assert k["passes"] <= 1 and k["pc"] * m * 8 <= T, (n, m, NB, T)
            assert seen == [1] * m, (n, m, NB, T)


@pytest.mark.parametrize("NB", BLOCKS)
def test_narrow_form_only_while_every_workgroup_has_a_compute_unit(NB):
    bound = host_lib().mwz_narrow_max_wgs()
    assert 0 < bound < 256                                    # below the chip's 256 compute units, with a margin
    took = 0
    for n in SIDES:
        pc = max(1, 32 // n)
        zs = -(-n // pc)
        r = rule(n, NB, 1)
        if NB * zs <= bound:
            assert (r["narrow"], r["threads"], r["zs"], r["pc"]) == (1, 256, zs, pc), (n, NB)
            took += 1
        else:                                                 # refused: the wide launch exactly as before
            assert (r["narrow"], r["threads"], r["zs"]) == (0, 512, wide_zs(n, NB)), (n, NB)
            assert r == rule(n, NB, 0)
    assert took == {1: 24, 4: 24, 19: 10, 64: 5}[NB]        # (19 blocks: up to 5 panels, sides to 10; 64 blocks: one panel, sides to 5)


@pytest.mark.parametrize("NB", BLOCKS)
def test_switch_off_is_the_wide_launch_as_it_was(NB):
    for n in SIDES:
        r = rule(n, NB, 0)
        zs = wide_zs(n, NB)
        assert (r["narrow"], r["threads"], r["zs"], r["sm"]) == (0, 512, zs, 2 * n * -(-n // zs) * K * 8), (n, NB)


def test_the_flagship_shape():
    """cohnelkies(8,15): 4 blocks, the largest 16 x 16 -- eight panels of two columns in workgroups of 256 threads, 32 workgroups"""
    r = rule(16, 4, 1)
    assert (r["narrow"], r["threads"], r["zs"], r["pc"]) == (1, 256, 8, 2)
    assert rule(16, 4, 0)["zs"] == 4

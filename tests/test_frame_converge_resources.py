"""Compile-time figures of the one-launch convergence kernel (csrc/frame_converge.hip), in the manner of
tests/test_converge_resources.py: eight instantiations -- 1 .. 4 points per lane x 1 or 2 terms, 1024 lanes each -- inside the 128
registers per lane a 1024-lane workgroup has; no scratch up to 3 points per lane and with one term, the bar
k_frame<1024, PPT, K, false> holds for the same shapes; at 4 points per lane with two terms -- where k_frame itself has 112 bytes
of scratch and 50 spilled vector registers in the same build -- pinned at what the compiler gives, as an upper bound.  And no
scalar spills in any of them (notes/convergence.md section 2: what the body does for that in its convergence form)."""
import re
import shutil

import pytest

from kernel_resources import HIPCC, resource_usage

# (points per lane, terms) -> (scratch bytes per lane, spilled vector registers) allowed; everything else: none
PINNED = {(4, 2): (124, 61)}

_USE = {}


def _kernels():
    """{(points per lane, terms): the compiler's figures}, the unit compiled once"""
    if not _USE:
        use = resource_usage("frame_converge.hip")
        assert all("k_frame_converge" in k for k in use), sorted(use)
        for name, r in use.items():
            nt, ppt, K, dual = (int(x) for x in re.search(r"k_frame_convergeILi(\d+)ELi(\d)ELi(\d)ELb(\d)E", name).groups())
            assert nt == 1024 and dual == 0 and (ppt, K) not in _USE, name
            _USE[(ppt, K)] = r
    return _USE


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_converge_kernel_has_eight_instantiations_within_the_register_file():
    use = _kernels()
    assert set(use) == {(p, k) for p in (1, 2, 3, 4) for k in (1, 2)}, sorted(use)
    for shape, r in use.items():
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (shape, r)
        scratch, spills = PINNED.get(shape, (0, 0))
        assert shape == (4, 2) or (scratch, spills) == (0, 0)     # nothing is pinned up to 3 points per lane or with one term
        assert r["ScratchSize [bytes/lane]"] <= scratch and r["VGPRs Spill"] <= spills, (shape, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_converge_kernel_has_no_scalar_spills():
    """No scalar spills in any of the eight (k_frame<1024, 1 .. 4, 2, false> of the same build has 34 / 30 / 46 / 65, and
    k_frame<1024, 4, 1, false> 8): one spilled scalar register reserves a vector register for the whole kernel, and at 128 the
    convergence form has none to give.  csrc/frame_body.inc reads the arguments where they are used, keeps the argument segment's
    address in LDS and fences the lane index between phases for this."""
    spilled = {shape: r["SGPRs Spill"] for shape, r in _kernels().items() if r["SGPRs Spill"]}
    assert not spilled, spilled


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_engine_unit_holds_no_convergence_kernel():
    """the new kernels live in their own unit: frame_engine.hip compiles the sixteen k_frame kernels it always did"""
    use = resource_usage("frame_engine.hip")
    assert len(use) == 16 and all("k_frameILi" in k for k in use), sorted(use)

"""Compile-time figures of the one-launch frame kernels for terms with a matrix or a normalisation mode (csrc/frame_general.hip), in
the manner of tests/test_frame_converge_resources.py: eight kernels -- k_frame_general and k_frame_general_converge, 1 or 2 points per
lane x 1 or 2 terms, 1024 lanes each -- inside the 128 registers per lane a 1024-lane workgroup has, without scratch, without spilled
vector registers and without spilled scalar registers: the bar k_frame_converge holds at the same shapes.

One shape is pinned at what the compiler gives, as an upper bound: k_frame_general_converge at 2 points per lane with 2 terms spills
ONE scalar register (no scratch, no vector spill).  Its loop holds the general form's two matrices, the convergence form's stop rule
and every LDS offset of two lattices at once; with the matrices as scalars it spills 8, with all eight entries in vector registers 2
vector registers (12 bytes of scratch), with six the same, with four 3 scalars; five -- what the kernel does -- leaves one
(notes/frame_general.md section 3).

And the units the body is shared with still hold the kernels they held."""
import re
import shutil

import pytest

from kernel_resources import HIPCC, resource_usage

# (kernel, points per lane, terms) -> spilled scalar registers allowed; everything else: none
PINNED_SCALAR = {("k_frame_general_converge", 2, 2): 1}

_USE = {}


def _kernels():
    """{(kernel, points per lane, terms): the compiler's figures}, the unit compiled once"""
    if not _USE:
        for name, r in resource_usage("frame_general.hip").items():
            m = re.search(r"(k_frame_general(?:_converge)?)ILi(\d+)ELi(\d)ELi(\d)ELb(\d)E", name)
            assert m, name
            kernel, (nt, ppt, K, dual) = m.group(1), (int(x) for x in m.groups()[1:])
            assert nt == 1024 and dual == 0 and (kernel, ppt, K) not in _USE, name
            _USE[(kernel, ppt, K)] = r
    return _USE


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_general_unit_holds_exactly_its_eight_kernels():
    assert set(_kernels()) == {(k, p, t) for k in ("k_frame_general", "k_frame_general_converge") for p in (1, 2) for t in (1, 2)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_general_kernels_fit_the_register_file_without_scratch_or_spills():
    for shape, r in _kernels().items():
        print(shape, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (shape, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (shape, r)
        assert r["SGPRs Spill"] <= PINNED_SCALAR.get(shape, 0), (shape, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_the_units_that_share_the_body_hold_the_kernels_they_held():
    use = resource_usage("frame_engine.hip")
    assert len(use) == 16 and all("k_frameILi" in k for k in use), sorted(use)
    use = resource_usage("frame_converge.hip")
    assert len(use) == 8 and all("k_frame_convergeILi" in k for k in use), sorted(use)

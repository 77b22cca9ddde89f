"""Compile-time figures of the kernel that runs a batch's frames with matrices or normalisation modes until converged
(csrc/fused_general_converge.hip), in the manner of tests/test_fused_general_resources.py: eight instantiations -- 1 or 2 points per
lane x 1 or 2 terms x {short rows, chain rows}, 1024 lanes each -- inside the 128 registers per lane a 1024-lane workgroup has, with
no scratch, no spilled vector register and no spilled scalar register (each of which costs the kernel a vector register).  And
csrc/fused_general.hip, whose launcher now takes batches: still its eight kernels, without scratch."""
import re
import shutil

import pytest

from kernel_resources import HIPCC, resource_usage

SHAPES = {(p, k, ch) for p in (1, 2) for k in (1, 2) for ch in (0, 1)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_general_converge_kernel_has_eight_instantiations_without_scratch_or_spills():
    use = resource_usage("fused_general_converge.hip")
    conv = {k: v for k, v in use.items() if "k_general_converge" in k}
    assert len(use) == len(conv) == 8, sorted(use)
    shapes = set()
    for name, r in conv.items():
        shapes.add(tuple(int(x) for x in re.search(r"k_general_convergeILi(\d)ELi(\d)ELi(\d)E", name).groups()))
        print(name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    assert shapes == SHAPES


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_general_kernel_still_has_its_eight_without_scratch():
    use = resource_usage("fused_general.hip")
    assert len(use) == 8 and all("k_general" in k and "converge" not in k for k in use), sorted(use)
    shapes = set()
    for name, r in use.items():
        shapes.add(tuple(int(x) for x in re.search(r"k_generalILi(\d)ELi(\d)ELi(\d)E", name).groups()))
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    assert shapes == SHAPES

"""Compile-time figures of the convergence kernel (csrc/fused_converge.hip), in the manner of tests/test_fused_general_resources.py:
16 instantiations -- 1 .. 4 points per lane x 1 or 2 terms x {short rows, chain rows}, 1024 lanes each -- inside the 128 registers
per lane a 1024-lane workgroup has; no scratch up to 3 points per lane; at 4 the one kernel that spills (two terms on chain rows,
as k_fused<1024, 4, 2, 1, 0> does: 64 bytes and 15 registers there) pinned at what the compiler gives, as an upper bound."""
import re
import shutil

import pytest

from kernel_resources import HIPCC, resource_usage

# (points per lane, terms, chain rows) -> (scratch bytes per lane, spilled registers) allowed; everything else: none
PINNED = {(4, 2, 1): (100, 24)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_converge_kernel_has_sixteen_instantiations_within_the_register_file():
    use = resource_usage("fused_converge.hip")
    conv = {k: v for k, v in use.items() if "k_converge" in k}
    assert len(use) == len(conv) == 16, sorted(use)
    shapes = set()
    for name, r in conv.items():
        shape = tuple(int(x) for x in re.search(r"k_convergeILi(\d)ELi(\d)ELi(\d)E", name).groups())
        shapes.add(shape)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        scratch, spills = PINNED.get(shape, (0, 0))
        assert shape[0] == 4 or (scratch, spills) == (0, 0)       # nothing is pinned for up to 3 points per lane
        assert r["ScratchSize [bytes/lane]"] <= scratch and r["VGPRs Spill"] <= spills and r["SGPRs Spill"] == 0, (name, r)
    assert shapes == {(p, k, ch) for p in (1, 2, 3, 4) for k in (1, 2) for ch in (0, 1)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_tracking_unit_has_four_small_kernels_without_scratch():
    use = resource_usage("converge_track.hip")
    assert len(use) == 4 and all("k_track" in k for k in use), sorted(use)
    for name, r in use.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)

"""Compile-time figures of the kernels behind lccrf_batch_inference_backward_all (include/lccrf.h section 2h), in the manner of
tests/test_compat_kernel_resources.py: no scratch memory and no spill in the new k_sum_frames and in the kernels the batch form
changed (k_compat_bwd, k_compat_reduce), and the LDS footprints they were designed to."""
import shutil

import pytest

from kernel_resources import HIPCC, lds_bytes, resource_usage

UNIT = "meanfield_backward.hip"


def _one(use, key):
    hit = {k: v for k, v in use.items() if key in k}
    assert len(hit) == 1, (key, sorted(hit))
    return next(iter(hit.values()))


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_batch_learned_kernels_use_no_scratch_and_their_planned_lds():
    use, lds = resource_usage(UNIT), lds_bytes(UNIT)
    for name in ("k_sum_frames", "k_compat_bwd", "k_compat_reduce"):
        r = _one(use, name)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    # k_sum_frames: a tile of 64 frames x 64 entries, rows padded to 65 floats; eight wavefronts per SIMD by registers
    assert _one(lds, "k_sum_frames") == 4 * 64 * 65
    r = _one(use, "k_sum_frames")
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r
    # k_compat_bwd keeps its footprint (mu + the y and Phi tiles); the reduction has no LDS
    assert _one(lds, "k_compat_bwd") == 4 * (64 * 65 + 2 * 384)
    assert _one(lds, "k_compat_reduce") == 0

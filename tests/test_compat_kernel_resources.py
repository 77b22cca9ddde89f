"""Compile-time figures of the label-compatibility kernels (include/lccrf.h section 1e), in the manner of
tests/test_kernel_resources.py: no scratch memory, registers that allow eight wavefronts per SIMD in the forward slice, and the LDS
footprint the kernels were designed to (several workgroups per CU)."""
import shutil

import pytest

from kernel_resources import HIPCC, lds_bytes, resource_usage


def _one(use, key):
    hit = {k: v for k, v in use.items() if key in k}
    assert len(hit) == 1, (key, sorted(hit))
    return next(iter(hit.values()))


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_compat_slice_uses_no_scratch_and_its_planned_lds():
    """k_slice_compat: 64 x 65 floats of mu + four tiles of 384 floats in LDS = 22 784 bytes (seven workgroups in a CU's 160 KB)."""
    r = _one(resource_usage("stream_filter.hip"), "k_slice_compat")
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r          # (eight wavefronts per SIMD by registers: LDS sets the occupancy)
    assert _one(lds_bytes("stream_filter.hip"), "k_slice_compat") == 4 * (64 * 65 + 4 * 384)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_compat_backward_kernels_use_no_scratch():
    use = resource_usage("meanfield_backward.hip")
    r = _one(use, "k_compat_bwd")
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
    assert _one(lds_bytes("meanfield_backward.hip"), "k_compat_bwd") == 4 * (64 * 65 + 2 * 384)   # mu + the y and Phi tiles
    compat = {k: v for k, v in use.items() if "k_compat_softmax" in k}
    assert len(compat) == 5                                  # 1, 2, 4, 8, 16 lanes per row
    for name, r in compat.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)

"""Compile-time figures of the kernels the normalisation modes add (include/lccrf.h section 1g), in the manner of
tests/test_compat_kernel_resources.py: the scaled instantiations of the generic splat kernels, the kernel that forms the factors and
the scaled k_bwd_combine use no scratch memory and spill no register, and the scaled splats keep the LDS footprint of the unscaled."""
import shutil

import pytest

from kernel_resources import HIPCC, lds_bytes, resource_usage


def _one(use, key):
    hit = {k: v for k, v in use.items() if key in k}
    assert len(hit) == 1, (key, sorted(hit))
    return next(iter(hit.values()))


def _clean(r):
    return r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_scaled_splats_use_no_scratch_and_the_unscaled_ones_lds():
    """(template <bool PRE>: the mangled names carry ILb1E for the scaled instantiation, ILb0E for the unscaled one)"""
    use, lds = resource_usage("stream_scaled.hip"), lds_bytes("stream_scaled.hip")        # PRE = true lives there ...
    use0, lds0 = resource_usage("stream_filter.hip"), lds_bytes("stream_filter.hip")      # ... PRE = false where it always was
    assert not any("ILb0E" in k for k in use)
    for kernel in ("k_splat", "k_splat4", "k_splat_long"):
        scaled, plain = "%d%sILb1E" % (len(kernel), kernel), "%d%sILb0E" % (len(kernel), kernel)
        r = _one(use, scaled)
        assert _clean(r), (kernel, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (kernel, r)      # (four wavefronts per SIMD at the least)
        assert _clean(_one(use0, plain)) and not any(scaled in k for k in use0), kernel
        assert _one(lds, scaled) == _one(lds0, plain), kernel
    assert _one(lds, "12k_splat_longILb1E") == 2 * 8192 * 4            # the two product tiles


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_factor_and_combine_kernels_use_no_scratch():
    r = _one(resource_usage("stream_scaled.hip"), "k_norm_factor")
    assert _clean(r) and r["VGPRs"] <= 32, r
    use = resource_usage("meanfield_backward.hip")
    for inst in ("k_bwd_combineILb1E", "k_bwd_combineILb0E"):
        r = _one(use, inst)
        assert _clean(r) and r["VGPRs"] <= 32, (inst, r)

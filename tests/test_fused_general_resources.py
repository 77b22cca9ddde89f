"""Compile-time figures of the fused engine's kernel for terms with a matrix or a normalisation mode (csrc/fused_general.hip), in
the manner of tests/test_kernel_resources.py, and the handle's engine probe lccrf_get_engine: declared, exported, bound."""
import ctypes as C
import importlib
import re
import shutil

import pytest

from abi_support import assert_declared_exported_bound, lib  # noqa: F401
from kernel_resources import HIPCC, resource_usage

pkg = importlib.import_module("lc-crf-slam_amd")
E_INVALID = -1


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_general_kernel_has_eight_instantiations_without_scratch():
    """1 or 2 points per lane x 1 or 2 terms x {short rows, chain rows}, 1024 lanes each: 128 registers per lane fill the CU's
    register file, chain_rows' ring wants v96..v127 free around it, and scratch traffic inside the loop costs more than the launches
    the kernel saves."""
    use = resource_usage("fused_general.hip")
    gen = {k: v for k, v in use.items() if "k_general" in k}
    assert len(use) == len(gen) == 8, sorted(use)
    shapes = set()
    for name, r in gen.items():
        shapes.add(tuple(int(x) for x in re.search(r"k_generalILi(\d)ELi(\d)ELi(\d)E", name).groups()))
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    assert shapes == {(p, k, ch) for p in (1, 2) for k in (1, 2) for ch in (0, 1)}


def test_get_engine_is_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, ("lccrf_get_engine",))
    assert lib.lccrf_abi_version() == 3
    assert hasattr(pkg.DenseCRFHIP, "engine")


def test_get_engine_rejects_null(lib):
    e, s = C.c_int(7), C.c_int(7)
    assert lib.lccrf_get_engine(None, C.byref(e), C.byref(s)) == E_INVALID
    assert lib.lccrf_get_engine(None, None, None) == E_INVALID
    assert (e.value, s.value) == (7, 7)

"""The C-ABI library: builds for gfx950, loads, exports every symbol include/lccrf.h
declares, and fails LOUDLY (no CPU fallback) when no GPU is usable.  No compute here."""
import ctypes as C
import importlib
import re

import pytest

from abi_support import header_source, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")


def declared_symbols():
    return sorted(set(re.findall(r"\b(lccrf_[a-z0-9_]+)\s*\(", header_source())))


def test_header_declares_the_reference_operator_surface():
    names = declared_symbols()
    # DenseCRF / PairwisePotential methods used at src/Tracking.cc:1920-1930
    for n in ("lccrf_create", "lccrf_destroy", "lccrf_set_unary", "lccrf_set_unary_from_label",
              "lccrf_add_pairwise", "lccrf_add_appearance_kernel", "lccrf_add_smooth_kernel",
              "lccrf_inference", "lccrf_start_inference", "lccrf_step_inference",
              "lccrf_get_map", "lccrf_get_probability"):
        assert n in names


def test_library_exports_every_declared_symbol(lib):
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.lccrf_abi_version() == 3


def test_python_binding_covers_every_declared_symbol(lib):
    bound = {n for n in declared_symbols() if getattr(getattr(lib, n), "argtypes", None) is not None}
    unbound = set(declared_symbols()) - bound - {"lccrf_abi_version", "lccrf_last_error"}
    assert not unbound, unbound


def test_fails_loudly_without_a_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    rc = lib.lccrf_create(C.byref(h), 0, 16, 2)
    assert rc == -2 and not h.value                     # LCCRF_E_NO_DEVICE, nothing created
    assert b"no CPU fallback" in lib.lccrf_last_error()
    with pytest.raises(pkg.LccrfError):
        pkg.DenseCRFHIP(16, 2)


def test_argument_checks_do_not_need_a_gpu(lib):
    assert lib.lccrf_create(None, 0, 16, 2) == -1
    h = C.c_void_p()
    assert lib.lccrf_create(C.byref(h), 0, -1, 2) == -1
    assert lib.lccrf_create(C.byref(h), 0, 4, 0) == -1
    assert lib.lccrf_set_unary(None, None) == -1
    assert lib.lccrf_batch_create(C.byref(h), 0, None) == -1

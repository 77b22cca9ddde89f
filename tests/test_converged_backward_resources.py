"""lccrf_batch_inference_backward_converged without a GPU (include/lccrf.h section 2j): the symbol, the ABI version, the argument
checks that need no device, the compile-time figures of the one-launch kernel it changed, and the torch functions' signatures.
(The pins on k_backward's instantiation count and on every other user of the shared loop: tests/test_fused_backward_resources.py.)"""
import ctypes as C
import importlib
import inspect
import re

import kernel_resources as kr
from abi_support import assert_declared_exported_bound, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
E_INVALID = -1
NAME = "lccrf_batch_inference_backward_converged"


def test_entry_point_is_declared_exported_and_bound(lib):
    src = assert_declared_exported_bound(lib, [NAME])
    decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % NAME, src).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["b", "max_iterations", "relax", "d_iterations", "d_grad_prob",
                                                                     "d_grad_unary", "d_grad_weights", "stream"]
    assert "const int32_t *d_iterations" in decl
    assert len(getattr(lib, NAME).argtypes) == 8
    assert hasattr(pkg.BatchCRF, "inference_backward_converged_device")
    sig = list(inspect.signature(pkg.BatchCRF.inference_backward_converged_device).parameters)
    assert sig == ["self", "max_iterations", "relax", "d_iterations", "d_grad_prob", "d_grad_unary", "d_grad_weights", "stream"]


def test_abi_version_is_still_3(lib):
    assert lib.lccrf_abi_version() == 3
    assert re.search(r"#define\s+LCCRF_ABI_VERSION\s+3\b", open(pkg.HEADER_PATH).read())


def test_argument_checks_need_no_device(lib):
    fn, err = getattr(lib, NAME), lambda: lib.lccrf_last_error().decode()
    one = C.c_void_p(8)                                           # (never dereferenced: every call below fails before the batch is looked at)
    assert fn(None, 5, 1.0, one, one, one, None, None) == E_INVALID and "handle" in err(), err()
    assert fn(None, -1, 1.0, one, one, one, None, None) == E_INVALID and "max_iterations" in err(), err()
    for relax in (float("nan"), float("inf"), -float("inf")):
        assert fn(None, 5, relax, one, one, one, None, None) == E_INVALID and "relax" in err(), (relax, err())
    assert fn(None, 5, 1.0, None, one, one, None, None) == E_INVALID and "d_iterations" in err(), err()
    assert fn(None, 0, 0.5, one, one, one, one, None) == E_INVALID and "handle" in err(), err()


def test_k_backward_with_counts_stays_within_the_register_budget():
    use = {k: v for k, v in kr.resource_usage("fused_backward.hip").items() if "k_backward" in k}
    assert len(use) == 8, sorted(use)
    for name, v in use.items():
        print(name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 128 and v["AGPRs"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)


def test_torch_functions_exist_with_the_stated_signatures():
    ag = importlib.import_module("lc-crf-slam_amd.autograd")

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(ag.mean_field_batch_converged) == [("batch", E), ("unary", E), ("weights", E), ("max_iterations", E),
                                                     ("criterion", pkg.STOP_LABELS), ("tol", 0.0), ("relax", 1.0)]
    assert params(ag.mean_field_converged)[:4] == [("crf", E), ("unary", E), ("weights", E), ("max_iterations", E)]
    assert params(ag.mean_field_converged)[4:] == [("criterion", pkg.STOP_LABELS), ("tol", 0.0), ("relax", 1.0)]
    last = list(inspect.signature(ag.BatchConvergedMeanFieldCRF.__init__).parameters.values())[-1]
    assert last.name == "fused_backward" and last.default is False
    # the existing signatures and defaults do not change
    assert params(ag.mean_field) == [("crf", E), ("unary", E), ("weights", E), ("n_iterations", 5), ("relax", 1.0)]
    assert params(ag.mean_field_batch) == [("batch", E), ("unary", E), ("weights", E), ("n_iterations", 5), ("relax", 1.0)]
    assert len([c for c in vars(ag).values() if inspect.isclass(c) and issubclass(c, ag.torch.autograd.Function)
                and c.__module__ == ag.__name__]) == 3       # (notes/torch_layers.md: extended, not multiplied)

"""lccrf_batch_inference_backward_modes_converged without a GPU (include/lccrf.h section 2l): the symbol, the ABI version, the argument
checks that need no device, the binding, the torch functions' and the module's signatures, the compile-time figures of the kernels the
call changed, and a C++ caller.  (k_backward_features' own pins, unchanged: tests/test_fused_backward_features_resources.py.)"""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import kernel_resources as kr
from abi_support import assert_declared_exported_bound, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAME = "lccrf_batch_inference_backward_modes_converged"
E = inspect.Parameter.empty


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_entry_point_is_declared_exported_and_bound(lib):
    src = assert_declared_exported_bound(lib, [NAME])
    decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % NAME, src).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["b", "max_iterations", "relax", "d_iterations", "d_grad_prob",
                                                                     "d_grad_unary", "d_grad_weights", "d_grad_features", "d_grad_compat",
                                                                     "d_grad_model", "stream"]
    assert "const int32_t *d_iterations" in decl and "float *const *d_grad_features" in decl
    assert len(getattr(lib, NAME).argtypes) == 11
    assert lib.lccrf_abi_version() == 3                           # added without a step: callers probe by symbol
    assert re.search(r"#define\s+LCCRF_ABI_VERSION\s+3\b", src)


def test_the_binding_has_the_method():
    assert _params(pkg.BatchCRF.inference_backward_modes_converged_device) == [
        ("self", E), ("max_iterations", E), ("relax", E), ("d_iterations", E), ("d_grad_prob", E), ("d_grad_unary", None),
        ("d_grad_weights", None), ("d_grad_features", None), ("d_grad_compat", None), ("d_grad_model", None), ("stream", None)]


def test_argument_checks_need_no_device(lib):
    fn, err = getattr(lib, NAME), lambda: lib.lccrf_last_error().decode()
    one = C.c_void_p(8)                                           # (never dereferenced: every call below fails before the batch is looked at)
    assert fn(None, 5, 1.0, one, one, one, None, None, None, None, None) == E_INVALID and "handle" in err(), err()
    assert fn(None, -1, 1.0, one, one, one, None, None, None, None, None) == E_INVALID and "max_iterations" in err(), err()
    for relax in (float("nan"), float("inf"), -float("inf")):
        assert fn(None, 5, relax, one, one, one, None, None, None, None, None) == E_INVALID and "relax" in err(), (relax, err())
    assert fn(None, 5, 1.0, None, one, one, None, None, one, one, None) == E_INVALID and "d_iterations" in err(), err()
    assert fn(None, 0, 0.5, one, one, None, None, None, None, one, None) == E_INVALID and "handle" in err(), err()


def test_torch_functions_and_module_have_the_stated_signatures():
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    assert _params(ag.mean_field_batch_features) == [("batch", E), ("n_points", E), ("unary", E), ("features", E), ("weights", E),
                                                     ("n_iterations", 5), ("relax", 1.0), ("compat", None)]
    assert _params(ag.mean_field_batch_features_converged) == [("batch", E), ("n_points", E), ("unary", E), ("features", E), ("weights", E),
                                                               ("max_iterations", E), ("criterion", pkg.STOP_LABELS), ("tol", 0.0),
                                                               ("relax", 1.0), ("compat", None)]
    assert issubclass(ag.BatchLearnedKernelCRF, torch.nn.Module) and callable(ag.BatchLearnedKernelCRF.close)
    assert _params(ag.BatchLearnedKernelCRF.__init__) == [
        ("self", E), ("n_points", E), ("raw_features", E), ("sd", E), ("weights", E), ("groups", None), ("max_iterations", None),
        ("n_iterations", 5), ("criterion", pkg.STOP_LABELS), ("tol", 0.0), ("relax", 1.0), ("device", 0), ("n_labels", 2),
        ("normalization", None), ("fused_backward", False)]
    # the existing functions and layers keep their signatures
    assert _params(ag.mean_field_batch_compat_converged) == [("batch", E), ("unary", E), ("weights", E), ("compat", E), ("max_iterations", E),
                                                             ("criterion", pkg.STOP_LABELS), ("tol", 0.0), ("relax", 1.0)]
    assert _params(ag.mean_field_batch) == [("batch", E), ("unary", E), ("weights", E), ("n_iterations", 5), ("relax", 1.0)]
    assert _params(ag.LearnedKernelCRF.__init__) == [("self", E), ("raw_features", E), ("sd", E), ("weights", E), ("groups", None),
                                                     ("n_iterations", 5), ("relax", 1.0), ("device", 0), ("fused_backward", False)]
    assert list(inspect.signature(ag.mean_field_features).parameters)[:6] == ["unary", "features", "weights", "n_iterations", "relax", "device"]
    assert len([c for c in vars(ag).values() if inspect.isclass(c) and issubclass(c, torch.autograd.Function)
                and c.__module__ == ag.__name__]) == 3       # (notes/torch_layers.md: extended, not multiplied)


def test_the_binding_counts_the_inputs_it_is_given():
    src = inspect.getsource(pkg.BatchCRF)
    assert src.count("self.inputs_serial += 1") == 3              # set_inputs_host, set_inputs_host_async, bind_inputs_device


def test_k_backward_features_with_counts_stays_within_the_register_budget():
    use = {k: v for k, v in kr.resource_usage("fused_backward_features.hip").items() if "k_backward_features" in k}
    assert len(use) == 8, sorted(use)
    for name, v in use.items():
        print(name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 128 and v["AGPRs"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)


def test_the_streaming_kernels_with_counts_use_no_scratch():
    use = kr.resource_usage("meanfield_backward.hip")
    for kernel in ("k_corner_dot", "k_bwd_combine_adjoint"):
        hits = {k: v for k, v in use.items() if kernel in k}
        assert hits, kernel
        for name, v in hits.items():
            print(name, v)
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)


def test_a_cpp_caller_compiles(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "lccrf.h"
int feature_gradients_at_the_reported_counts(lccrf_batch_handle b, const float *d_grad_prob, float *d_grad_unary, float *d_gf0, float *d_gf1,
                                             void *stream)
{
    const int32_t *it = nullptr, *changed = nullptr, *converged = nullptr;
    const float *delta = nullptr;
    if (int rc = lccrf_batch_device_convergence(b, &it, &delta, &changed, &converged)) return rc;
    static_assert(LCCRF_ABI_VERSION == 3, "added without a step");
    float *const gf[2] = {d_gf0, d_gf1};
    return lccrf_batch_inference_backward_modes_converged(b, 12, 1.0f, it, d_grad_prob, d_grad_unary, nullptr, gf, nullptr, nullptr, stream);
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)

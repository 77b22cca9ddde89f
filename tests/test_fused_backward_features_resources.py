"""The one-launch backward with feature gradients without a GPU (include/lccrf.h section 1l): the compile-time figures of
k_backward_features' eight instantiations, the option's number and refusals, the bindings, the layers' keyword and the C++ accessors.
(k_backward's and k_backward_general's own figures and those of every other user of the shared loop:
tests/test_fused_backward_resources.py and tests/test_fused_backward_learnt_resources.py, unchanged.)"""
import importlib
import inspect
import os
import re
import subprocess

import kernel_resources as kr
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_backward_features_has_eight_instantiations_within_the_register_budget():
    use = {k: v for k, v in kr.resource_usage("fused_backward_features.hip").items() if "k_backward_features" in k}
    lds = kr.lds_bytes("fused_backward_features.hip")
    shapes = sorted(tuple(int(x) for x in re.search(r"k_backward_featuresILi(\d+)ELi(\d+)ELi(\d+)E", k).groups()) for k in use)
    assert shapes == sorted((p, k, ch) for p in (1, 2) for k in (1, 2) for ch in (0, 1)), shapes
    for name, v in use.items():
        print(name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 128 and v["AGPRs"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert lds[name] == 0, (name, lds[name])                 # (the LDS is dynamic: the plan plus k_backward's 2304 bytes)


def test_the_unit_is_part_of_the_library():
    mk = open(os.path.join(ROOT, "lc-crf-slam_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "csrc/fused_backward_features.hip" in srcs and "csrc/fused_backward.hip" in srcs


def test_the_option_is_number_eight_and_options_six_and_seven_kept_their_numbers(lib):
    src = open(os.path.join(ROOT, "include", "lccrf.h")).read()
    assert "LCCRF_OPT_FUSED_BACKWARD  = 6" in src
    assert re.search(r"LCCRF_OPT_FUSED_BACKWARD_LEARNT\s*=\s*7\b", src)
    assert re.search(r"LCCRF_OPT_FUSED_BACKWARD_FEATURES\s*=\s*8\b", src)
    assert pkg.OPT_FUSED_BACKWARD == 6 and pkg.BatchCRF.OPT_FUSED_BACKWARD == 6
    assert pkg.OPT_FUSED_BACKWARD_LEARNT == 7 and pkg.BatchCRF.OPT_FUSED_BACKWARD_LEARNT == 7
    assert pkg.OPT_FUSED_BACKWARD_FEATURES == 8 and pkg.BatchCRF.OPT_FUSED_BACKWARD_FEATURES == 8
    assert lib.lccrf_abi_version() == 3                         # added without a version step


def test_option_on_a_null_handle_as_a_default_and_an_unknown_one(lib):
    assert lib.lccrf_set_option(None, 8, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_batch_set_option(None, 8, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_set_default_option(8, 1) == -1               # per handle or batch only, as options 6 and 7
    assert b"no process-wide default" in lib.lccrf_last_error()
    assert lib.lccrf_set_default_option(7, 1) == -1 and lib.lccrf_set_default_option(6, 1) == -1
    assert lib.lccrf_set_default_option(99, 1) == -1


def test_the_option_is_accepted_in_the_source_and_99_is_not():
    src = open(os.path.join(ROOT, "lc-crf-slam_amd", "csrc", "api_object.hip")).read()
    body = src[src.index("int lccrf::apply_option"):]
    body = body[:body.index("\n}\n")]
    for name in ("LCCRF_OPT_FUSED_BACKWARD_FEATURES", "LCCRF_OPT_FUSED_BACKWARD_LEARNT", "LCCRF_OPT_FUSED_BACKWARD"):
        assert "case %s:" % name in body, name
    assert 'default: return fail(LCCRF_E_INVALID, "unknown option %d", option);' in body


def test_the_feature_layers_take_the_keyword_and_the_learnt_ones_keep_their_signatures():
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    p = inspect.signature(ag.mean_field_features).parameters
    assert list(p)[-2:] == ["fused_backward", "route_out"] and p["fused_backward"].default is False and p["route_out"].default is None
    assert list(p)[:6] == ["unary", "features", "weights", "n_iterations", "relax", "device"]
    p = list(inspect.signature(ag.LearnedKernelCRF.__init__).parameters.values())[-1]
    assert p.name == "fused_backward" and p.default is False
    assert isinstance(inspect.getattr_static(ag.LearnedKernelCRF, "backward_route"), property)
    assert list(inspect.signature(ag.mean_field_learned).parameters) == ["unary", "features", "weights", "compat", "n_iterations", "relax",
                                                                         "device"]
    assert list(inspect.signature(ag.LearnedCRF.__init__).parameters) == ["self", "raw_features", "sd", "weights", "groups", "n_labels",
                                                                          "n_iterations", "relax", "device"]


def test_cpp_accessors_compile(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text("""
#include "lccrf_densecrf.hpp"
#include "lccrf_densecrf_gpu.hpp"
int route_of(DenseCRF::DenseCRFHIP<2> &a, DenseCRF::DenseCRFGPU<2> &b)
{
    a.setOption(LCCRF_OPT_FUSED_BACKWARD_FEATURES, 1);
    b.setOption(LCCRF_OPT_FUSED_BACKWARD_FEATURES, 1);
    static_assert(LCCRF_OPT_FUSED_BACKWARD == 6 && LCCRF_OPT_FUSED_BACKWARD_LEARNT == 7 && LCCRF_OPT_FUSED_BACKWARD_FEATURES == 8,
                  "option numbers");
    return a.backwardRoute() == LCCRF_BACKWARD_FUSED ? b.backwardRoute() : LCCRF_BACKWARD_NONE;
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)

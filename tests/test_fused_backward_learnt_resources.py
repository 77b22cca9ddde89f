"""The one-launch backward of learnt models without a GPU (include/lccrf.h section 1k): the compile-time figures of
k_backward_general's eight instantiations, the option's number and refusals, the bindings, the layers' keyword and the C++ accessors.
(k_backward's own figures and those of every other user of the shared loop: tests/test_fused_backward_resources.py, unchanged.)"""
import importlib
import inspect
import os
import re
import subprocess

import kernel_resources as kr
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_backward_general_has_eight_instantiations_within_the_register_budget():
    use = {k: v for k, v in kr.resource_usage("fused_backward_general.hip").items() if "k_backward_general" in k}
    lds = kr.lds_bytes("fused_backward_general.hip")
    shapes = sorted(tuple(int(x) for x in re.search(r"k_backward_generalILi(\d+)ELi(\d+)ELi(\d+)E", k).groups()) for k in use)
    assert shapes == sorted((p, k, ch) for p in (1, 2) for k in (1, 2) for ch in (0, 1)), shapes
    for name, v in use.items():
        print(name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 128 and v["AGPRs"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert lds[name] == 0, (name, lds[name])                 # (the LDS is dynamic: the plan plus k_backward's 2304 bytes)


def test_the_option_is_number_seven_and_option_six_kept_its_number(lib):
    src = open(os.path.join(ROOT, "include", "lccrf.h")).read()
    assert "LCCRF_OPT_FUSED_BACKWARD  = 6" in src
    assert re.search(r"LCCRF_OPT_FUSED_BACKWARD_LEARNT\s*=\s*7\b", src)
    assert pkg.OPT_FUSED_BACKWARD == 6 and pkg.BatchCRF.OPT_FUSED_BACKWARD == 6
    assert pkg.OPT_FUSED_BACKWARD_LEARNT == 7 and pkg.BatchCRF.OPT_FUSED_BACKWARD_LEARNT == 7
    assert lib.lccrf_abi_version() == 3


def test_option_on_a_null_handle_as_a_default_and_an_unknown_one(lib):
    assert lib.lccrf_set_option(None, 7, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_batch_set_option(None, 7, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_set_default_option(7, 1) == -1               # per handle or batch only, as option 6
    assert lib.lccrf_set_default_option(6, 1) == -1
    assert lib.lccrf_set_default_option(99, 1) == -1


def test_the_option_is_accepted_in_the_source_and_99_is_not():
    src = open(os.path.join(ROOT, "lc-crf-slam_amd", "csrc", "api_object.hip")).read()
    body = src[src.index("int lccrf::apply_option"):]
    body = body[:body.index("\n}\n")]
    assert "case LCCRF_OPT_FUSED_BACKWARD_LEARNT:" in body and "case LCCRF_OPT_FUSED_BACKWARD:" in body
    assert 'default: return fail(LCCRF_E_INVALID, "unknown option %d", option);' in body


def test_compat_layers_take_the_keyword_and_the_plain_layers_keep_their_signatures():
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    for cls in (ag.CompatMeanFieldCRF, ag.BatchCompatMeanFieldCRF, ag.MeanFieldCRF, ag.BatchMeanFieldCRF):
        p = list(inspect.signature(cls.__init__).parameters.values())[-1]
        assert p.name == "fused_backward" and p.default is False, cls


def test_cpp_accessors_compile(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text("""
#include "lccrf_densecrf.hpp"
#include "lccrf_densecrf_gpu.hpp"
int route_of(DenseCRF::DenseCRFHIP<2> &a, DenseCRF::DenseCRFGPU<2> &b)
{
    a.setOption(LCCRF_OPT_FUSED_BACKWARD_LEARNT, 1);
    b.setOption(LCCRF_OPT_FUSED_BACKWARD_LEARNT, 1);
    static_assert(LCCRF_OPT_FUSED_BACKWARD == 6 && LCCRF_OPT_FUSED_BACKWARD_LEARNT == 7, "option numbers");
    return a.backwardRoute() == LCCRF_BACKWARD_FUSED ? b.backwardRoute() : LCCRF_BACKWARD_NONE;
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)

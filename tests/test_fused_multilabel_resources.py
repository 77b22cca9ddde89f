"""The fused engine's kernel for three to eight labels without a GPU (csrc/fused_multilabel.hip; LCCRF_OPT_FUSED_MULTILABEL): the
compile-time figures of every instantiation, the shipped range they add up to, the option's number, its refusals and its bindings."""
import importlib
import inspect
import os
import re
import subprocess

import kernel_resources as kr
from abi_support import lib  # noqa: F401
from fused_multilabel_cases import PLAN

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lc-crf-slam_amd", "csrc")

# The shipped range, as the header of csrc/fused_multilabel.hip states it: label count -> points per lane of a 1024-lane workgroup.
# Two points per lane of five to eight labels are left out: with two terms on chain rows those kernels need scratch.
SHIPPED = {3: (1, 2), 4: (1, 2), 5: (1,), 6: (1,), 7: (1,), 8: (1,)}


def test_every_instantiation_fits_the_register_file_without_scratch_and_they_are_the_shipped_range():
    """1024 lanes: 128 registers per lane fill the CU's register file; chain_rows' ring wants v96..v127 free around it; scratch
    traffic inside the loop costs more than the launches the kernel saves"""
    use = kr.resource_usage("fused_multilabel.hip")
    mine = {k: v for k, v in use.items() if "k_multilabel" in k}
    assert len(use) == len(mine), sorted(set(use) - set(mine))   # the unit holds nothing else
    shapes = []
    for name, r in mine.items():
        print(name, r)
        shapes.append(tuple(int(x) for x in re.search(r"k_multilabelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups()))
        assert r["VGPRs"] + r["AGPRs"] <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    want = sorted((L, p, k, ch) for L, ppts in SHIPPED.items() for p in ppts for k in (1, 2) for ch in (0, 1))
    assert sorted(shapes) == want, sorted(set(shapes) ^ set(want))


def test_the_table_is_the_header_text_and_the_launch_guard():
    src = open(os.path.join(CSRC, "fused_multilabel.hip")).read()
    assert "//     L = 3, 4        frames of up to 2048 active points (one or two points per lane)" in src
    assert "//     L = 5 .. 8      frames of up to 1024 active points (one point per lane" in src
    assert "constexpr int kMultiMinL = 3, kMultiMaxL = 8;" in src
    assert "constexpr int multi_max_ppt(int L) { return L <= 4 ? 2 : 1; }" in src
    assert PLAN == {L: 1024 * max(p) for L, p in SHIPPED.items()}
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "lc-crf-slam_amd", "Makefile")).read()


def test_the_compiler_left_no_copy_out():
    """the remark hipcc leaves where it turned a register copy into nothing; with names that differ, a value was lost (see `pad` in
    the unit): the unit's assembly holds none"""
    cmd = [kr.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), "-S", os.path.join(CSRC, "fused_multilabel.hip"), "-o", "-"]
    asm = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    assert asm.count("s_endpgm") >= 32
    assert re.findall(r"; kill: def \$vgpr\d+ killed \$vgpr\d+ killed \$exec", asm) == []


def test_the_unit_is_part_of_the_library():
    mk = open(os.path.join(ROOT, "lc-crf-slam_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "csrc/fused_multilabel.hip" in srcs


def test_the_option_is_number_nine_declared_and_bound(lib):
    src = open(os.path.join(ROOT, "include", "lccrf.h")).read()
    assert re.search(r"LCCRF_OPT_FUSED_MULTILABEL\s*=\s*9\b", src)
    assert re.search(r"LCCRF_OPT_FUSED_BACKWARD_FEATURES\s*=\s*8\b", src)          # the others kept their numbers
    assert re.search(r"#define LCCRF_ABI_VERSION 3\b", src) and lib.lccrf_abi_version() == 3   # added without a version step
    assert pkg.OPT_FUSED_MULTILABEL == 9 and pkg.BatchCRF.OPT_FUSED_MULTILABEL == 9


def test_the_option_is_accepted_and_ten_is_not(lib):
    """lccrf_set_option(h, 9, 1) is LCCRF_OK and (h, 10, 1) LCCRF_E_INVALID: on a handle in tests/test_fused_multilabel.py (a handle
    needs a device); here the switch both calls go through, the process-wide default, and the NULL handle"""
    src = open(os.path.join(CSRC, "api_object.hip")).read()
    body = src[src.index("int lccrf::apply_option"):]
    body = body[:body.index("\n}\n")]
    assert "case LCCRF_OPT_FUSED_MULTILABEL:" in body
    assert 'default: return fail(LCCRF_E_INVALID, "unknown option %d", option);' in body
    assert len(re.findall(r"case LCCRF_OPT_", body)) == 7        # options 1, 2, 5 .. 9; 3 and 4 are the batch's own; nothing takes 10
    assert lib.lccrf_set_option(None, 9, 1) == -1 and b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_batch_set_option(None, 9, 1) == -1 and b"NULL" in lib.lccrf_last_error()
    try:
        assert lib.lccrf_set_default_option(9, 1) == 0           # like LCCRF_OPT_FRAME_GENERAL
    finally:
        assert lib.lccrf_set_default_option(9, 0) == 0
    assert lib.lccrf_set_default_option(10, 1) == -1 and b"no process-wide default" in lib.lccrf_last_error()


def test_the_layers_have_the_attribute_and_keep_their_constructors():
    """fused_multilabel is an attribute of the two layers, off until set: the constructors' parameter lists are pinned by
    tests/test_fused_backward_resources.py and its siblings (fused_backward last) and stay as they were"""
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    for layer in (ag.MeanFieldCRF, ag.BatchMeanFieldCRF):
        assert isinstance(inspect.getattr_static(layer, "fused_multilabel"), property), layer
        p = list(inspect.signature(layer.__init__).parameters.values())[-1]
        assert p.name == "fused_backward" and p.default is False, layer


def test_cpp_option_compiles(tmp_path):
    src = tmp_path / "opt.cpp"
    src.write_text("""
#include "lccrf_densecrf.hpp"
int engine_of(DenseCRF::DenseCRFHIP<4> &a)
{
    static_assert(LCCRF_OPT_FUSED_MULTILABEL == 9, "option number");
    a.setOption(LCCRF_OPT_FUSED_MULTILABEL, 1);
    return a.engine();
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)

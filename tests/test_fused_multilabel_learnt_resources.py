"""The fused engine's kernel for learnt models of three to eight labels without a GPU (csrc/fused_multilabel_general.hip;
LCCRF_MULTILABEL_LEARNT): the compile-time figures of every instantiation and the shipped range they add up to, stated in the unit's
header, include/lccrf.h, notes/fused_multilabel.md and the cases' PLAN alike."""
import os
import re
import subprocess

import kernel_resources as kr
from fused_multilabel_learnt_cases import PLAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lc-crf-slam_amd", "csrc")
UNIT = "fused_multilabel_general.hip"

# The shipped range, as the header of the unit states it: label count -> points per lane of a 1024-lane workgroup.
SHIPPED = {3: (1, 2), 4: (1, 2), 5: (1,), 6: (1,), 7: (1,), 8: (1,)}
# ... of which L = 3 and 4 at one point per lane are required; the rest ships because it compiles clean and measured faster than the
# streaming route by more than the runs' spread (notes/fused_multilabel.md section 6 has the table)
REQUIRED = {3: (1,), 4: (1,)}


def _instantiations(table):
    return sorted((L, p, k, ch) for L, ppts in table.items() for p in ppts for k in (1, 2) for ch in (0, 1))


def test_every_instantiation_fits_the_register_file_without_scratch_and_they_are_the_shipped_range():
    """1024 lanes: 128 registers per lane fill the CU's register file; chain_rows' ring wants v96..v127 free around it; no spilling
    kernel ships"""
    use = kr.resource_usage(UNIT)
    mine = {k: v for k, v in use.items() if "k_multilabel_general" in k}
    assert len(use) == len(mine), sorted(set(use) - set(mine))   # the unit holds nothing else
    shapes = []
    for name, r in mine.items():
        print(name, r)
        shapes.append(tuple(int(x) for x in re.search(r"k_multilabel_generalILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups()))
        assert r["VGPRs"] + r["AGPRs"] <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    assert sorted(shapes) == _instantiations(SHIPPED), sorted(set(shapes) ^ set(_instantiations(SHIPPED)))
    assert set(_instantiations(REQUIRED)) <= set(shapes)


def test_the_table_is_the_header_text_the_launch_guard_the_public_header_and_the_note():
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "//     L = 3, 4        frames of up to 2048 active points (one or two points per lane)" in src
    assert "//     L = 5 .. 8      frames of up to 1024 active points (one point per lane)" in src
    assert "constexpr int kMultiMinL = 3, kMultiMaxL = 8;" in src
    assert "constexpr int multi_general_max_ppt(int L) { return L <= 4 ? 2 : 1; }" in src
    assert PLAN == {L: 1024 * max(p) for L, p in SHIPPED.items()}
    api = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "lccrf.h")).read())
    assert "3 or 4 labels on frames of up to 2048 points, 5 to 8 labels on frames of up to 1024" in api[api.index("LCCRF_MULTILABEL_LEARNT   (off"):]
    note = open(os.path.join(ROOT, "notes", "fused_multilabel.md")).read()
    note = note[note.index("## 6."):]
    assert "L = 3, 4: frames of up to 2048 active points" in note and "L = 5 .. 8: frames of up to 1024 active points" in note


def test_the_compiler_left_no_copy_out():
    """the remark hipcc leaves where it turned a register copy into nothing (see `pad` in csrc/fused_multilabel.hip): none here"""
    cmd = [kr.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), "-S", os.path.join(CSRC, UNIT), "-o", "-"]
    asm = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    assert asm.count("s_endpgm") >= len(_instantiations(SHIPPED))
    assert re.findall(r"; kill: def \$vgpr\d+ killed \$vgpr\d+ killed \$exec", asm) == []


def test_the_unit_is_part_of_the_library_with_the_siblings_flags():
    mk = open(os.path.join(ROOT, "lc-crf-slam_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "csrc/" + UNIT in srcs and "csrc/fused_multilabel.hip" in srcs
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS\s*:=(.*)$", mk, re.M).group(1)   # one rule compiles every unit of SRCS

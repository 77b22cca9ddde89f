"""Compile-time figures of the label-code form of the lean inference kernel (csrc/fused_lean_label.hip: k_fused_lean_lbl): two
workgroups share a CU only at 128 registers per lane or fewer, and nothing of the loop may live in scratch."""
import re

import kernel_resources


def test_label_code_kernels_fit_two_per_cu_without_scratch():
    use = kernel_resources.resource_usage("fused_lean_label.hip")
    lbl = {k: v for k, v in use.items() if "k_fused_lean_lblI" in k}
    # every (points per lane, K, chain) the lean plan launches from prepared records: 4 x 2 x 2
    shapes = {tuple(int(x) for x in re.search(r"k_fused_lean_lblILi512ELi(\d)ELi(\d)ELi(\d)ELb\dE", name).groups()) for name in lbl}
    assert len(lbl) == 16 and shapes == {(p, k, ch) for p in (1, 2, 3, 4) for k in (1, 2) for ch in (0, 1)}, sorted(lbl)
    for name, r in lbl.items():
        assert r["VGPRs"] + r["AGPRs"] <= 128, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)

"""The one-launch backward without a GPU (include/lccrf.h section 1j): the compile-time figures of k_backward's eight instantiations,
the figures of every other user of the shared loop (fused_loop.h) pinned at what they were before the loop gained its TRANSPOSE
parameter, the two new symbols, the option, and the C++ accessors."""
import importlib
import os
import re
import subprocess

import pytest

import kernel_resources as kr
from abi_support import assert_declared_exported_bound, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lccrf_get_backward_route", "lccrf_batch_get_backward_route")
FIGURES = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")

# {unit: {kernel: (VGPRs, AGPRs, scratch bytes per lane, VGPR spills, SGPR spills, static LDS bytes)}} of the commit before this
# route existed, from kernel_resources.resource_usage / lds_bytes on a build of that commit (the LDS of these kernels is dynamic: 0)
PARENT = {
    "fused_engine.hip": {
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi0ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (85, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi0ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (46, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi0ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (85, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi1ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi1ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (46, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi1ELi1ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi0ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (70, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi0ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (49, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi0ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (70, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi1ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi1ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (49, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi1ELi2ELi1ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi0ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (97, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi0ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (50, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi0ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (97, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi1ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi1ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (50, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi1ELi1ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi0ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (92, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi0ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (56, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi0ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (94, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi1ELb0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi1ELb0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (56, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi2ELi2ELi1ELb0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi0ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (89, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi0ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (54, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi0ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (89, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi1ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi1ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (54, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi1ELi1ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi0ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (87, 0, 0, 0, 2, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi0ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (63, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi0ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (90, 0, 0, 0, 2, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi1ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi1ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (63, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi3ELi2ELi1ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi0ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (94, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi0ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (58, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi0ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (94, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi1ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi1ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (58, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi1ELi1ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi0ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (109, 0, 0, 0, 2, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi0ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (69, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi0ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (114, 0, 0, 0, 2, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi1ELb1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi1ELb1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (68, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_112k_fused_leanILi512ELi4ELi2ELi1ELb1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (53, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (47, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (53, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (48, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (67, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (59, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (72, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (60, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi1ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (73, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (51, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (76, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (52, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (101, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (64, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (104, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (64, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi2ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (70, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (54, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (73, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (55, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (98, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (67, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (100, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (68, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi3ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (84, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (58, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (87, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (59, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (122, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (71, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 12, 2, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 64, 15, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (72, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi1024ELi4ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 60, 14, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (53, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (47, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (53, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (48, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (73, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (66, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (74, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (68, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi1ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (73, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (51, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (76, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (52, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi1ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi0ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (106, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi0ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (69, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi0ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (109, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi1ELi0EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi1ELi1EEEvNS_6CrfDevENS0_9FusedArgsE":
            (70, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_fusedILi512ELi2ELi2ELi1ELi2EEEvNS_6CrfDevENS0_9FusedArgsE":
            (128, 0, 0, 0, 0, 0),
    },
    "fused_general.hip": {
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi1ELi1ELi0EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (54, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi1ELi1ELi1EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi1ELi2ELi0EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (70, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi1ELi2ELi1EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi2ELi1ELi0EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (75, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi2ELi1ELi1EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi2ELi2ELi0EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (106, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_19k_generalILi2ELi2ELi1EEEvNS_6CrfDevENS0_11GeneralArgsE":
            (128, 0, 0, 0, 0, 0),
    },
    "fused_converge.hip": {
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi1ELi1ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (53, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi1ELi1ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi1ELi2ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (68, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi1ELi2ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi2ELi1ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (74, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi2ELi1ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi2ELi2ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (104, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi2ELi2ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi3ELi1ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (72, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi3ELi1ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi3ELi2ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (100, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi3ELi2ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi4ELi1ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (88, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi4ELi1ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi4ELi2ELi0EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (124, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_110k_convergeILi4ELi2ELi1EEEvNS_6CrfDevENS0_12ConvergeArgsE":
            (128, 0, 100, 24, 0, 0),
    },
    "fused_general_converge.hip": {
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi1ELi1ELi0EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (54, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi1ELi1ELi1EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi1ELi2ELi0EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (68, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi1ELi2ELi1EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi2ELi1ELi0EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (71, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi2ELi1ELi1EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi2ELi2ELi0EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (102, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_118k_general_convergeILi2ELi2ELi1EEEvNS_6CrfDevENS0_19GeneralConvergeArgsE":
            (128, 0, 0, 0, 0, 0),
    },
    # (the scalar spill counts of k_frame as of the reserved-key fix in frame_body.inc, notes/hash_build_tests.md: nine of them moved
    #  by 1 to 8; vector registers, scratch, vector spills and LDS are the earlier ones)
    "frame_engine.hip": {
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi1ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi1ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 35, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi1ELi2ELb1EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 27, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi2ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi2ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 30, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi2ELi2ELb1EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 28, 6, 19, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi3ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 2, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi3ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 53, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi3ELi2ELb1EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 32, 7, 28, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi4ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 8, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi4ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 112, 50, 63, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi1024ELi4ELi2ELb1EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 120, 64, 45, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi512ELi1ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi512ELi1ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 35, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi512ELi2ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_17k_frameILi512ELi2ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsE":
            (128, 0, 0, 0, 30, 0),
    },
    "frame_general.hip": {
        "_ZN5lccrf12_GLOBAL__N_115k_frame_generalILi1024ELi1ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_115k_frame_generalILi1024ELi1ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_115k_frame_generalILi1024ELi2ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_115k_frame_generalILi1024ELi2ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_124k_frame_general_convergeILi1024ELi1ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_9FrameConvENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_124k_frame_general_convergeILi1024ELi1ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_9FrameConvENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_124k_frame_general_convergeILi1024ELi2ELi1ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_9FrameConvENS3_12FrameGeneralE":
            (128, 0, 0, 0, 0, 0),
        "_ZN5lccrf12_GLOBAL__N_124k_frame_general_convergeILi1024ELi2ELi2ELb0EEEvNS_6CrfDevENS_2fb9FrameArgsENS3_9FrameConvENS3_12FrameGeneralE":
            (128, 0, 0, 0, 1, 0),
    },
}


def test_k_backward_has_eight_instantiations_within_the_register_budget():
    use = {k: v for k, v in kr.resource_usage("fused_backward.hip").items() if "k_backward" in k}
    shapes = sorted(tuple(int(x) for x in re.search(r"k_backwardILi(\d+)ELi(\d+)ELi(\d+)E", k).groups()) for k in use)
    assert shapes == sorted((p, k, ch) for p in (1, 2) for k in (1, 2) for ch in (0, 1)), shapes
    for name, v in use.items():
        print(name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 128, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)


@pytest.mark.parametrize("unit", sorted(PARENT))
def test_the_shared_loops_other_users_did_not_move(unit, monkeypatch):
    remarks = kr._remarks(unit)                                   # (one compilation for both readers)
    monkeypatch.setattr(kr, "_remarks", lambda src: remarks)
    use, lds = kr.resource_usage(unit), kr.lds_bytes(unit)
    assert sorted(use) == sorted(PARENT[unit]), "the unit's kernels changed"
    for name, want in PARENT[unit].items():
        got = tuple(use[name][f] for f in FIGURES) + (lds[name],)
        assert got == want, (name, got, want)


def test_symbols_are_declared_exported_and_bound(lib):
    src = assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3
    assert "LCCRF_OPT_FUSED_BACKWARD  = 6" in src
    assert pkg.OPT_FUSED_BACKWARD == 6 and pkg.BatchCRF.OPT_FUSED_BACKWARD == 6
    assert (pkg.BACKWARD_NONE, pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED) == (0, 1, 2)
    for cls in (pkg.DenseCRFHIP, pkg.BatchCRF):
        assert hasattr(cls, "backward_route")


def test_getters_reject_null(lib):
    import ctypes as C
    r = C.c_int(77)
    assert lib.lccrf_get_backward_route(None, C.byref(r)) == -1 and r.value == 77
    assert lib.lccrf_batch_get_backward_route(None, C.byref(r)) == -1 and r.value == 77
    assert lib.lccrf_get_backward_route(None, None) == -1
    assert lib.lccrf_batch_get_backward_route(None, None) == -1


def test_option_on_a_null_handle_and_as_a_default(lib):
    assert lib.lccrf_set_option(None, 6, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_batch_set_option(None, 6, 1) == -1
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_set_default_option(6, 1) == -1               # per handle or batch only


def test_torch_layers_take_the_keyword():
    import inspect
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    for cls in (ag.MeanFieldCRF, ag.BatchMeanFieldCRF):
        p = list(inspect.signature(cls.__init__).parameters.values())[-1]
        assert p.name == "fused_backward" and p.default is False, cls


def test_cpp_accessors_compile(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text("""
#include "lccrf_densecrf.hpp"
#include "lccrf_densecrf_gpu.hpp"
int route_of(DenseCRF::DenseCRFHIP<2> &a, DenseCRF::DenseCRFGPU<2> &b)
{
    a.setOption(LCCRF_OPT_FUSED_BACKWARD, 1);
    b.setOption(LCCRF_OPT_FUSED_BACKWARD, 1);
    return a.backwardRoute() == LCCRF_BACKWARD_FUSED ? b.backwardRoute() : LCCRF_BACKWARD_NONE;
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)

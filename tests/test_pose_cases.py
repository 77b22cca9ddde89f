"""The scene list of tests/pose_cases.py, checked on the CPU before the GPU tests trust it: (a) over the list the restatement takes
every branch its trace counts, (b) on every scene the restatement gives the same answer whatever the order of its points -- and so
of its sums, which is all that the kernel's lane tree changes.  Also here, since they are answered before a device is touched: the
single-frame entry point's capacity and sign checks."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import pose_cases as pc

pkg = importlib.import_module("lc-crf-slam_amd")


def test_restatement_gives_the_recorded_answers(po, wl):
    """tests/golden/pose_restatement.npz: pose bits, flags and both counts of orc_pose_optimization as it stood BEFORE the counters were
    added (built with oracle/Makefile's flags), on the scenes the pose tests used until then and an exact monocular one.  The
    restatement with and without a trace gives those bits: the counters changed no arithmetic."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_restatement.npz"))
    assert len(g["params"]) == 12
    for i, (n, seed, noise, outf, mono, ninv) in enumerate(g["params"]):
        s = wl.pose_scene(int(n), seed=int(seed), noise=noise, outlier_frac=outf, mono_frac=mono, n_invalid=int(ninv))
        flags = np.unpackbits(g["outlier_bits"][g["outlier_offsets"][i]:g["outlier_offsets"][i + 1]])[:int(n)]
        for trace in (False, True):
            r = pc.run_oracle(po, s, trace=trace)
            assert np.array_equal(r[0].reshape(16).view(np.uint32), g["pose_bits"][i]), (i, trace)
            assert np.array_equal(r[1], flags) and (r[2], r[3]) == tuple(g["counts"][i]), (i, trace)
        assert set(r[4]) == set(po.POSE_TRACE)


def test_trace_counts_what_it_should(po, wl):
    """on scenes whose course is known the counters say so: two valid points, nothing runs; an exact scene, accepted trials and no
    failure; every round ends in exactly one way"""
    s = wl.pose_scene(40, seed=2)
    valid = np.zeros(40, np.uint8)
    valid[[3, 17]] = 1
    assert not any(pc.run_oracle(po, s, valid, trace=True)[4].values())
    tr = pc.run_oracle(po, wl.pose_scene(300, seed=300, noise=0.0, outlier_frac=0.0), trace=True)[4]
    assert tr["accepted"] > 0 and tr["solve6_failed"] == tr["tempchi_nonfinite"] == tr["readmitted"] == 0
    assert tr["quat_x"] == tr["quat_y"] == tr["quat_z"] == 0
    # every round ends in exactly one way
    assert tr["stop_qmax"] + tr["stop_rho_zero"] + tr["stop_bad_lm"] + tr["full_round"] == 4


def test_the_list_holds_every_shape_class():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lc-crf-slam_amd", "csrc", "pose_opt.hip")).read()
    kpt, stage = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kPT", "kStageMax"))
    assert (pc.WAVES, pc.STAGE_MAX) == (kpt // 64, stage)                  # the boundaries below are the kernel's
    assert all(any(n.startswith(c + ":") for n in pc.NAMES) for c in pc.CLASSES)
    sizes = {n: pc.scene(n)["Xw"].shape[0] for n in pc.NAMES}
    assert {sizes["unstaged:%d" % n] for n in pc.UNSTAGED} == set(pc.UNSTAGED) and min(pc.UNSTAGED) == pc.STAGE_MAX + 1
    assert max(pc.UNSTAGED) == 16384                                       # the cap of lccrf_pose_optimization
    assert pc.scene("unstaged:4097:all_valid")["valid"].all() and not pc.scene("unstaged:4097")["valid"].all()
    for n in pc.FEW_N:
        for k in pc.FEW_VALID:
            v = pc.scene("few:%d:valid%d" % (n, k))["valid"]
            assert int(v.sum()) == k and v[0] and v[-1]                    # over the whole index range
    # a staged frame of three edges and more in which a wavefront's chunk of compact_level0 holds points but no edge
    assert any(sizes[n] <= pc.STAGE_MAX and pc.scene(n)["valid"].sum() >= 3 and pc.chunks_without_an_edge(sizes[n], pc.scene(n)["valid"])
               for n in pc.NAMES)
    assert len(pc.FAR_NAMES) == len(pc.FAR) * len(pc.FAR_N)


def test_the_list_takes_every_branch_of_the_restatement(po):
    """(a) every counter of orc_pose_optimization_traced is non-zero on some scene of the list, the three quaternion cases each"""
    total = dict.fromkeys(po.POSE_TRACE, 0)
    for name in pc.NAMES:
        for k, v in pc.oracle(po, name)[4].items():
            # a scene of the nonfinite class stands for its own counter alone: its trial poses are NaN, and the "case" its
            # quaternions take is merely where a comparison with NaN falls
            if k == "tempchi_nonfinite" or not name.startswith("nonfinite:"):
                total[k] += v
    missing = [k for k in po.POSE_TRACE if total[k] == 0]
    assert not missing, (missing, total)


@pytest.mark.parametrize("name", pc.NAMES)
def test_the_restatement_does_not_care_about_the_order_of_the_points(po, name):
    """(b) reversed and under two seeded permutations: the same flags (permuted back), the same counts, the pose within the bar the
    kernel is held to (2 ulp or 1e-7)"""
    s = pc.scene(name)
    T, outl, ninl, ninit, _ = pc.oracle(po, name)
    n = s["Xw"].shape[0]
    for what, perm in pc.reorderings(name, n):
        Tp, op, ninl_p, ninit_p = pc.run_oracle(po, pc.reordered(s, perm))
        back = np.empty_like(op)
        back[perm] = op
        on = s["valid"] == 1
        flips = int((back[on] != outl[on]).sum())
        assert flips == 0 and (ninl_p, ninit_p) == (ninl, ninit), (name, what, flips, ninl_p, ninl)
        assert pc.pose_within_bar(Tp, T), (name, what) + pc.pose_distance(Tp, T)


def test_single_frame_capacity_and_sign_checks():
    """answered before a device is looked for: more than 16384 keypoints is E_CAPACITY with its message, a negative count E_INVALID"""
    s = pc.scene("unstaged:16384")
    grow = lambda a: np.concatenate([a, a[:1]])
    with pytest.raises(pkg.LccrfError) as ei:
        pkg.pose_optimization(grow(s["Xw"]), grow(s["kp"]), grow(s["u_right"]), grow(s["inv_sigma2"]), s["K4"], s["bf"], s["T_init"])
    assert ei.value.code == -6 and "at most 16384 keypoints per frame" in str(ei.value)
    f32p, out = C.POINTER(C.c_float), np.zeros(16, np.float32)
    K, T = np.ascontiguousarray(s["K4"]), np.ascontiguousarray(s["T_init"]).reshape(16)
    lib = pkg.lib()
    rc = lib.lccrf_pose_optimization(0, -1, None, None, None, None, None, None, K.ctypes.data_as(f32p), float(s["bf"]),
                                     T.ctypes.data_as(f32p), out.ctypes.data_as(f32p), None, None)
    assert rc == -1 and b"n_points < 0" in lib.lccrf_last_error()
    rc = lib.lccrf_pose_optimization(0, 16385, None, None, None, None, None, None, K.ctypes.data_as(f32p), float(s["bf"]),
                                     T.ctypes.data_as(f32p), out.ctypes.data_as(f32p), None, None)
    assert rc == -6 and b"at most 16384 keypoints per frame" in lib.lccrf_last_error()

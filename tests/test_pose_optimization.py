"""Optimizer::PoseOptimization (reference src/Optimizer.cc:239-450), SURVEY.md section 8f-3 -- PARITY UNPINNED: the
reference runs it on g2o, which needs Eigen (absent in this image), and holds no test or fixture for it.

CPU part: the oracle's restatement (oracle/lccrf_oracle.c: orc_pose_optimization) against hand-derived known answers
-- exact data give back the exact pose, gross outliers are flagged and re-admitted as the schedule prescribes, fewer
than three correspondences leave the pose alone, the schedule is invariant to things it must be invariant to.
GPU part: the HIP kernel (csrc/pose_opt.hip) against that restatement -- identical outlier flags and inlier counts,
poses equal as float32 up to 2 ulp (the 6x6 sums are taken in a different order), and the batch entry point that reads
the CRF's labels where the inference kernel left them."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_cases as pc

pkg = importlib.import_module("lc-crf-slam_amd")


def _arrays_ready():
    """The arrays handed to lccrf_batch_pose_optimization are filled on torch's stream; the call runs on the batch's own non-blocking
    stream, and nothing orders the two.  The caller of an asynchronous entry point owes it finished arrays: this waits for torch's
    stream alone, and is called BEFORE lccrf_batch_run, so that run and pose stay back to back with no synchronisation in between --
    that the pose kernel is ordered behind the CRF on the batch's stream is part of what the batch tests check."""
    import torch
    torch.cuda.current_stream().synchronize()


def _run_oracle(po, s, valid=None):
    return po.oracle_pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["valid"] if valid is None else valid,
                                       s["K4"], s["bf"], s["T_init"])


def test_oracle_recovers_an_exact_pose(po, wl):
    for n, mono in ((300, 0.0), (300, 1.0), (500, 0.3), (12, 0.5)):
        s = wl.pose_scene(n, seed=n, noise=0.0, outlier_frac=0.0, mono_frac=mono)
        T, outl, ninl, ninit = _run_oracle(po, s)
        assert ninit == n and ninl == n and not outl.any()
        assert np.abs(T - s["T_true"]).max() < 5e-6, (n, mono, np.abs(T - s["T_true"]).max())
        assert np.array_equal(T[3], [0, 0, 0, 1])
        np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=2e-6)      # a rotation comes back


def test_oracle_flags_gross_outliers_and_keeps_the_rest(po, wl):
    s = wl.pose_scene(900, seed=5, noise=0.7, outlier_frac=0.15)
    T, outl, ninl, ninit = _run_oracle(po, s)
    assert ninit == 900 and ninl == 900 - int(outl.sum())
    assert np.abs(T - s["T_true"]).max() < 2e-3
    gross = s["gross"]
    assert (outl[gross] == 1).mean() > 0.97                 # 25 px off: far beyond chi2 = 5.991 / 7.815
    assert (outl[~gross] == 1).mean() < 0.08                # chi2(2) / chi2(3) at 95 % each flag ~5 % of honest points


def test_oracle_too_few_correspondences_and_invalid_points(po, wl):
    s = wl.pose_scene(40, seed=2)
    valid = np.zeros(40, np.uint8)
    valid[[3, 17]] = 1
    T, outl, ninl, ninit = _run_oracle(po, s, valid)
    assert (ninit, ninl) == (2, 0) and np.array_equal(T, s["T_init"])          # Optimizer.cc:361-362
    # invalid points contribute nothing: deleting them from the arrays gives the same answer
    s = wl.pose_scene(400, seed=9, n_invalid=150)
    T1, o1, n1, i1 = _run_oracle(po, s)
    keep = s["valid"] == 1
    sub = dict(s, Xw=s["Xw"][keep], kp=s["kp"][keep], u_right=s["u_right"][keep], inv_sigma2=s["inv_sigma2"][keep],
               valid=np.ones(int(keep.sum()), np.uint8))
    T2, o2, n2, i2 = _run_oracle(po, sub)
    assert i1 == i2 == 250 and n1 == n2 and np.array_equal(T1, T2) and np.array_equal(o1[keep], o2)


def test_oracle_fewer_than_ten_edges_run_one_round(po, wl):
    """optimizer.edges().size() < 10 -> break after the first round (Optimizer.cc:434-435): a gross outlier among 8 points is
    flagged by round 0 and never gets the chance to be re-examined; the pose still comes from that single round."""
    s = wl.pose_scene(8, seed=4, noise=0.0, outlier_frac=0.0, mono_frac=0.0)
    s["kp"][2] += 40.0
    T, outl, ninl, ninit = _run_oracle(po, s)
    assert ninit == 8 and outl[2] == 1 and ninl == 8 - int(outl.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n,noise,outf,mono,ninv", [(2000, 0.7, 0.15, 0.2, 300), (500, 0.0, 0.0, 0.0, 0), (333, 1.5, 0.3, 1.0, 10),
                                                     (9, 0.5, 0.2, 0.5, 0), (2, 0.5, 0.0, 0.0, 0), (4096, 0.7, 0.1, 0.2, 0)])
def test_hip_pose_optimization_matches_the_restatement(po, wl, n, noise, outf, mono, ninv):
    s = wl.pose_scene(n, seed=n + 1, noise=noise, outlier_frac=outf, mono_frac=mono, n_invalid=ninv)
    To, oo, no, _ = _run_oracle(po, s)
    Th, oh, nh = pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"], valid=s["valid"])
    assert nh == no and np.array_equal(oh[s["valid"] == 1], oo[s["valid"] == 1])
    ulp = np.abs(Th.view(np.int32).astype(np.int64) - To.view(np.int32).astype(np.int64))
    assert ulp.max() <= 2 or np.abs(Th - To).max() < 1e-7, (ulp.max(), np.abs(Th - To).max())


@pytest.mark.gpu
def test_hip_pose_optimization_reads_the_crf_labels_on_the_device(po, wl):
    """CRF (lccrf_batch_run) -> pose (lccrf_batch_pose_optimization) with the labels staying in HBM: per frame the same as
    the oracle's pose optimisation on the points the oracle's CRF labels static."""
    import torch
    import crf_cases as cc
    F, N = 5, 1500
    dev = torch.device("cuda", 0)
    pbs = [wl.slam_problem(N, seed=900 + f) for f in range(F)]
    scenes = [wl.pose_scene(N, seed=950 + f) for f in range(F)]
    b = pkg.BatchCRF(F, N, 2, [2, 2], [10.0, 30.0])
    b.set_inputs_host([N] * F, [np.stack([pb["kernels"][k][0] for pb in pbs]) for k in range(2)],
                      label=np.stack([pb["label"] for pb in pbs]), conf=0.7)
    t = lambda key, dt: torch.from_numpy(np.stack([np.ascontiguousarray(s[key]) for s in scenes]).astype(dt)).to(dev)
    dX, dk, du, di, dTi = t("Xw", np.float32), t("kp", np.float32), t("u_right", np.float32), t("inv_sigma2", np.float32), t("T_init", np.float32)
    dTo = torch.zeros((F, 16), dtype=torch.float32, device=dev)
    dout = torch.zeros((F, N), dtype=torch.uint8, device=dev)
    dni, dn0 = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    _arrays_ready()
    b.run(5, True)                                        # asynchronous; the pose right behind it, no synchronisation by the caller
    b.pose_optimization(dX.data_ptr(), dk.data_ptr(), du.data_ptr(), di.data_ptr(), scenes[0]["K4"], scenes[0]["bf"], dTi.data_ptr(),
                        dTo.data_ptr(), dout.data_ptr(), dni.data_ptr(), dn0.data_ptr())
    b.synchronize()
    labels = b.map()
    print("n_initial", dn0.cpu().numpy(), "n_inliers", dni.cpu().numpy(), "static labels", (labels != 0).sum(1),
          "pose moved", [not np.array_equal(dTo[f].cpu().numpy(), dTi[f].cpu().numpy()) for f in range(F)])
    for f in range(F):
        o = cc.setup(po.OracleCRF, pbs[f])
        o.inference_native(5, True)
        assert np.array_equal(labels[f], o.map())
        static = (o.map() != 0).astype(np.uint8)
        s = scenes[f]
        To, oo, no, n0 = po.oracle_pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], static, s["K4"], s["bf"], s["T_init"])
        assert int(dn0[f]) == n0 == int(static.sum()) and int(dni[f]) == no
        assert np.array_equal(dout[f].cpu().numpy()[static == 1], oo[static == 1])
        assert np.abs(dTo[f].cpu().numpy().reshape(4, 4) - To).max() < 1e-6


@pytest.mark.gpu
def test_batch_pose_after_a_run_with_a_fallback_frame_and_extra_edges(po, wl):
    """(1) lccrf_batch_pose_optimization right behind an asynchronous lccrf_batch_run in which one frame did
    not fit the one-launch kernel -- the pose must be computed from that frame's REAL labels (the re-run's), not from
    stale ones; (2) with_map = 0 leaves no labels: LCCRF_E_STATE; (3) the CRF-order contract's extra edges: map points the
    CRF skipped (observs == 0, Tracking.cc:1857-1859) ride behind the CRF's points and count as static."""
    import torch
    import crf_cases as cc
    F, N, NX = 3, 1200, 100                               # NX extra non-CRF edges per frame
    dev = torch.device("cuda", 0)
    pbs = [wl.slam_problem(N, seed=400), cc.shaped_problem(wl, N, "sparse", seed=5), wl.slam_problem(N, seed=402)]
    scenes = [wl.pose_scene(N + NX, seed=650 + f) for f in range(F)]
    maxN = N + NX
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(2)]
    label = np.full((F, maxN), -1, np.int16)
    for f, pb in enumerate(pbs):
        for k in range(2):
            feats[k][f, :N] = pb["kernels"][k][0]
        label[f, :N] = pb["label"]
    b = pkg.BatchCRF(F, maxN, 2, [2, 2], [float(pbs[0]["kernels"][k][1]) for k in range(2)])
    b.set_inputs_host([N] * F, feats, label=label, conf=0.7)
    t = lambda key, dt: torch.from_numpy(np.stack([np.ascontiguousarray(s[key]) for s in scenes]).astype(dt)).to(dev)
    dX, dk, du, di, dTi = t("Xw", np.float32), t("kp", np.float32), t("u_right", np.float32), t("inv_sigma2", np.float32), t("T_init", np.float32)
    dTo = torch.zeros((F, 16), dtype=torch.float32, device=dev)
    dout = torch.zeros((F, maxN), dtype=torch.uint8, device=dev)
    dni, dn0 = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    args = (dX.data_ptr(), dk.data_ptr(), du.data_ptr(), di.data_ptr(), scenes[0]["K4"], scenes[0]["bf"], dTi.data_ptr(),
            dTo.data_ptr(), dout.data_ptr(), dni.data_ptr(), dn0.data_ptr())
    _arrays_ready()
    b.run(5, False)
    with pytest.raises(pkg.LccrfError) as ei:
        b.pose_optimization(*args)
    assert ei.value.code == -5
    refs = []
    for pb in pbs:
        o = cc.setup(po.OracleCRF, pb)
        o.inference_native(5, True)
        refs.append(o.map().copy())
        o.close()
    for extra in (False, True):
        dtot = torch.full((F,), N + NX, dtype=torch.int32, device=dev)
        _arrays_ready()
        b.pose_set_crf_counts(dtot.data_ptr() if extra else None)
        b.run(5, True)                                    # asynchronous; frame 1 is flagged for the re-run
        b.pose_optimization(*args)                        # no synchronisation in between by the caller
        b.synchronize()
        assert b.fallback_frames() == 1
        labels = b.map()
        for f in range(F):
            assert np.array_equal(labels[f, :N], refs[f])
            s = scenes[f]
            n = N + NX if extra else N
            gate = np.ones(n, np.uint8)
            gate[:N] = refs[f] != 0
            To, oo, no, n0 = po.oracle_pose_optimization(s["Xw"][:n], s["kp"][:n], s["u_right"][:n], s["inv_sigma2"][:n], gate,
                                                         s["K4"], s["bf"], s["T_init"])
            assert int(dn0[f]) == n0 == int(gate.sum()) and int(dni[f]) == no, (extra, f)
            assert np.array_equal(dout[f].cpu().numpy()[:n][gate == 1], oo[gate == 1])
            assert np.abs(dTo[f].cpu().numpy().reshape(4, 4) - To).max() < 1e-6
    b.close()


@pytest.mark.gpu
def test_hip_pose_optimization_survives_trim_and_growth(po, wl):
    """The single-frame entry point keeps a staging area between calls: growing it, freeing it (lccrf_trim_cache) and calling
    again must give the same answers."""
    out = []
    for n in (300, 3000, 300):
        s = wl.pose_scene(n, seed=77)
        out.append(pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"], valid=s["valid"]))
        if n == 3000:
            pkg.lib().lccrf_trim_cache()
    assert np.array_equal(out[0][0], out[2][0]) and np.array_equal(out[0][1], out[2][1]) and out[0][2] == out[2][2]
    s = wl.pose_scene(3000, seed=77)
    To, oo, no, _ = _run_oracle(po, s)
    assert out[1][2] == no and np.array_equal(out[1][1][s["valid"] == 1], oo[s["valid"] == 1])


TWIN_FAR_SCENE = "far:500:2.5:010:dt1"                    # the pose moves, from a matrix whose largest diagonal element is m11


@pytest.mark.gpu
def test_instrumented_twin_runs_the_same_pose_kernel(po, wl):
    """Round 6: the instrumented library (liblccrf_hip_instr.so) differs from the release one by profiling hooks only -- and its pose kernel's
    hook, a lane-divergent branch beside the reductions' lane exchanges, made the butterfly run under a partial EXEC mask: the pose of
    every frame with ten edges or more stayed at its initial value.  Found by running the whole GPU suite on the twin; the hook's branch
    is uniform now.  Same scene through both libraries: same bits."""
    import crf_cases as cc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import importlib, sys, numpy as np
sys.path.insert(0, %r)
pkg = importlib.import_module("lc-crf-slam_amd"); wl = importlib.import_module("lc-crf-slam_amd.workloads")
sys.path.insert(0, %r)
import pose_cases as pc
# ... and the form that reads its edges from global memory (4097), and a start off the trace > 0 branch of the quaternion
for n in (2000, 500, 64, 9, 4097, %r):
    s = pc.scene(n) if isinstance(n, str) else wl.pose_scene(n, seed=n + 1, noise=0.7, outlier_frac=0.15, mono_frac=0.2, n_invalid=0)
    T, o, ninl = pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"], valid=s["valid"])
    print(n, ninl, int(o.sum()), " ".join("%%08x" %% x for x in np.asarray(T, np.float32).reshape(-1).view(np.uint32)))
""" % (root, os.path.join(root, "tests"), TWIN_FAR_SCENE)
    assert pc.oracle(po, TWIN_FAR_SCENE)[4]["quat_y"] > 0 and not np.array_equal(pc.oracle(po, TWIN_FAR_SCENE)[0], pc.scene(TWIN_FAR_SCENE)["T_init"])
    outs = []
    for env in (dict(os.environ), cc.switch_env(LCCRF_POSE_TWIN="1")):     # (any switch selects the twin)
        env.pop("LCCRF_LIB", None) if env.get("LCCRF_POSE_TWIN") is None else None
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-6:])
    assert outs[0] == outs[1], (outs[0], outs[1])
    s = wl.pose_scene(2000, seed=2001, noise=0.7, outlier_frac=0.15, mono_frac=0.2, n_invalid=0)
    To, oo, no, _ = _run_oracle(po, s)
    assert int(outs[0][0].split()[1]) == no                  # ... and it is the restatement's answer


# ---- the scene list of tests/pose_cases.py (checked on the CPU by tests/test_pose_cases.py) ------------------------------------------
def _assert_matches(Th, oh, nh, To, oo, no, edge, what):
    """the assertions of test_hip_pose_optimization_matches_the_restatement, the figures printed first"""
    ulp, dist = pc.pose_distance(Th, To)
    print("%s: inliers %d / %d, flags differing %d, pose %d ulp %.3g abs" % (what, nh, no, int((oh[edge] != oo[edge]).sum()), ulp, dist))
    assert nh == no and np.array_equal(oh[edge], oo[edge])
    assert ulp <= 2 or dist < 1e-7, (ulp, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_hip_pose_optimization_matches_the_restatement_on_the_scene_list(po, name):
    """Every shape class of tests/pose_cases.py: frames of more than 4096 keypoints (the kernel form that reads its edges from global
    memory, up to the cap of 16384), the thresholds of the schedule and of compact_level0, few valid points among many, initial poses
    far from the truth (a system that is not positive definite, the quaternion of a matrix of trace <= 0, rho == 0, ten iterations),
    points behind the camera (re-admitted edges), a chi2 that is not finite.  Same bar as above: equal counts, equal flags, 2 ulp."""
    s = pc.scene(name)
    To, oo, no, _, _ = pc.oracle(po, name)
    Th, oh, nh = pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"], valid=s["valid"])
    _assert_matches(Th, oh, nh, To, oo, no, s["valid"] == 1, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [600, 5000])
@pytest.mark.parametrize("with_valid", [False, True], ids=["label", "label+valid"])
def test_hip_pose_optimization_label_argument_gates_edges(po, wl, n, with_valid):
    """the single-frame entry point's `label`: a point labelled 0 has no edge, alone and together with `valid` -- the restatement
    run with valid & (label != 0); 600 and 5000 points: both kernel forms read the labels"""
    s = wl.pose_scene(n, seed=n + 1, n_invalid=n // 7 if with_valid else 0)
    label = np.where(np.arange(n) % 3 == 1, 0, np.where(np.arange(n) % 2, 1, 2)).astype(np.int16)    # a third moving; static as 1 or 2
    gate = (s["valid"] & (label != 0)).astype(np.uint8)
    assert 0 < int(gate.sum()) < int(s["valid"].sum())
    To, oo, no, _ = _run_oracle(po, s, gate)
    Th, oh, nh = pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"],
                                       valid=s["valid"] if with_valid else None, label=label)
    _assert_matches(Th, oh, nh, To, oo, no, gate == 1, "n = %d" % n)
    assert not oh[gate == 0].any()                          # the wrapper's zeros, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("n", [600, 5000])
def test_hip_pose_optimization_leaves_flags_of_points_without_an_edge(po, wl, n):
    """include/lccrf.h: entries of outlier_out of points without an edge are left as they were -- preset to 7, in both kernel
    forms, with points gated by `valid` and by `label`; the flags of the edges are the restatement's whatever they held before"""
    s = wl.pose_scene(n, seed=n + 1, n_invalid=n // 7)
    label = np.where(np.arange(n) % 5 == 2, 0, 1).astype(np.int16)
    gate = (s["valid"] & (label != 0)).astype(np.uint8)
    To, oo, no, _ = _run_oracle(po, s, gate)
    Th, oh, nh = pkg.pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["K4"], s["bf"], s["T_init"], valid=s["valid"],
                                       label=label, outlier=np.full(n, 7, np.uint8))
    assert (gate == 0).sum() > n // 7 and np.all(oh[gate == 0] == 7)
    _assert_matches(Th, oh, nh, To, oo, no, gate == 1, "n = %d" % n)


def _run_then_pose(b, scenes, maxN, preset=7):
    """lccrf_batch_run(5, with_map) and, right behind it with no synchronisation in between, lccrf_batch_pose_optimization of one scene
    per frame (device arrays strided by maxN, built and settled before the run) -> (Tcw_in, Tcw_out, outlier, n_inliers, n_initial) on
    the host; the outputs are preset (Tcw_out 9.0, outlier 7, counts -1) so that what the kernel leaves alone shows"""
    import torch
    dev = torch.device("cuda", 0)
    F = len(scenes)

    def t(key, tail):
        a = np.zeros((F, maxN) + tail, np.float32)
        for f, s in enumerate(scenes):
            if s is not None:
                a[f, :s[key].shape[0]] = s[key].reshape((-1,) + tail)
        return torch.from_numpy(a).to(dev)
    dX, dk, du, di = t("Xw", (3,)), t("kp", (2,)), t("u_right", ()), t("inv_sigma2", ())
    some = next(s for s in scenes if s is not None)
    Tin = np.stack([(s or some)["T_init"] for s in scenes]).astype(np.float32).reshape(F, 16)
    dTi = torch.from_numpy(Tin).to(dev)
    dTo = torch.full((F, 16), 9.0, dtype=torch.float32, device=dev)
    dout = torch.full((F, maxN), preset, dtype=torch.uint8, device=dev)
    dni, dn0 = torch.full((F,), -1, dtype=torch.int32, device=dev), torch.full((F,), -1, dtype=torch.int32, device=dev)
    _arrays_ready()
    b.run(5, True)
    b.pose_optimization(dX.data_ptr(), dk.data_ptr(), du.data_ptr(), di.data_ptr(), some["K4"], some["bf"], dTi.data_ptr(),
                        dTo.data_ptr(), dout.data_ptr(), dni.data_ptr(), dn0.data_ptr())
    b.synchronize()
    return Tin.reshape(F, 4, 4), dTo.cpu().numpy().reshape(F, 4, 4), dout.cpu().numpy(), dni.cpu().numpy(), dn0.cpu().numpy()


def _oracle_static(po, pb):
    import crf_cases as cc
    o = cc.setup(po.OracleCRF, pb)
    o.inference_native(5, True)
    m = o.map().copy()
    o.close()
    return m


@pytest.mark.gpu
def test_batch_pose_of_a_ragged_batch(po, wl):
    """F = 6, maxN = 1300, frames of 1300, 0, 2, 9, 10 and 777 points: every frame the restatement of that frame alone on the points the
    oracle's CRF labels static (1e-6 on the pose, the batch tests' bar); a frame with fewer than three edges -- its workgroup
    returns early, next to full frames -- hands Tcw_in back untouched with n_inliers = 0; nothing is written beyond a frame's
    points or on points without an edge."""
    import crf_cases as cc
    sizes, maxN = (1300, 0, 2, 9, 10, 777), 1300
    pbs = [wl.slam_problem(n, seed=1000 + n) if n else cc.empty_problem(2, [2, 2]) for n in sizes]
    scenes = [wl.pose_scene(n, seed=1100 + n) if n else None for n in sizes]
    b = cc.batch_of(pbs, maxN=maxN)
    Tin, Tout, outl, ninl, n0 = _run_then_pose(b, scenes, maxN)
    labels = b.map()
    b.close()
    early = 0
    for f, n in enumerate(sizes):
        ref = _oracle_static(po, pbs[f]) if n else np.zeros(0, np.int16)
        assert np.array_equal(labels[f, :n], ref), f
        static = (ref != 0).astype(np.uint8)
        assert np.all(outl[f, n:] == 7) and np.all(outl[f, :n][static == 0] == 7), f
        assert int(n0[f]) == int(static.sum()), f
        if static.sum() < 3:
            early += 1
            assert int(ninl[f]) == 0 and np.array_equal(Tout[f].view(np.int32), Tin[f].view(np.int32)), f
            assert not outl[f, :n][static == 1].any(), f
            continue
        s = scenes[f]
        To, oo, no, _ = _run_oracle(po, s, static)
        assert int(ninl[f]) == no and np.array_equal(outl[f, :n][static == 1], oo[static == 1]), f
        assert np.abs(Tout[f] - To).max() < 1e-6, f
    assert early >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 100], ids=["4200+4100:crf_points_only", "4200+4100:extra_edges"])
def test_batch_pose_beyond_the_staged_size(po, wl, extra):
    """F = 2, maxN = 4200, frames of 4200 and 4100 keypoints: the kernel form that reads its edges from global memory, behind the
    streaming engine's CRF -- once with every point a CRF point, once with the last 100 of each frame riding behind the CRF's
    points as extra edges (lccrf_batch_pose_set_crf_counts: static whatever the label word holds)."""
    import torch
    import crf_cases as cc
    totals, maxN = (4200, 4100), 4200
    pbs = [wl.slam_problem(n - extra, seed=1200 + f) for f, n in enumerate(totals)]
    scenes = [wl.pose_scene(n, seed=1300 + f) for f, n in enumerate(totals)]
    b = cc.batch_of(pbs, maxN=maxN)
    dtot = torch.tensor(totals, dtype=torch.int32, device=torch.device("cuda", 0))
    b.pose_set_crf_counts(dtot.data_ptr() if extra else None)
    Tin, Tout, outl, ninl, n0 = _run_then_pose(b, scenes, maxN)          # (settles dtot with its own arrays before the run)
    labels, engine = b.map(), b.engine()
    b.close()
    assert engine == 1, engine                             # the streaming engine: frames of this size fit no one-launch kernel
    for f, n in enumerate(totals):
        ref = _oracle_static(po, pbs[f])
        assert np.array_equal(labels[f, :n - extra], ref), f
        gate = np.ones(n, np.uint8)
        gate[:n - extra] = ref != 0
        To, oo, no, ninit = _run_oracle(po, scenes[f], gate)
        assert int(n0[f]) == ninit == int(gate.sum()) and int(ninl[f]) == no, f
        assert np.array_equal(outl[f, :n][gate == 1], oo[gate == 1]), f
        assert np.all(outl[f, n:] == 7) and np.all(outl[f, :n][gate == 0] == 7), f
        assert np.abs(Tout[f] - To).max() < 1e-6, f

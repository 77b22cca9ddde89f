"""The unary builder (first "next" row): Tracking::ComputeMapPointErrAndObserv +
Tracking::RroughClassify for a whole frame.  PARITY UNPINNED against the reference (no fixture exists,
src/Tracking.cc is unbuildable here); the HIP path is checked against the oracle's restatement."""
import importlib

import numpy as np
import pytest

import crf_cases as cc
import next_row_cases as nr

pkg = importlib.import_module("lc-crf-slam_amd")


def test_oracle_unary_build_known_answers(po, wl):
    """CPU: the whole-frame oracle equals its per-point pieces, drops empty points, uses the prior."""
    sc = wl.map_point_scene(300, 10, seed=3)
    obs, err, dep, lab = po.oracle_unary_build(sc["Xw"], sc["obs_ptr"], sc["obs_kf"], sc["obs_kp"],
                                               sc["kf_pose"], sc["kf_intr"], sc["kf_bounds"])
    n = np.diff(sc["obs_ptr"])
    assert np.array_equal(obs, n.astype(np.float32))
    assert np.all(lab[n == 0] == -1) and np.all((lab[n > 0] == 0) | (lab[n > 0] == 1))
    assert np.all(err[n == 0] == 0) and np.all(dep[n == 0] == 0)
    assert 0 < (lab == 0).sum() < (lab == 1).sum()                 # mostly static, some moving
    ref = po.oracle_rough_classify(obs[n > 0], err[n > 0], dep[n > 0])
    assert np.array_equal(ref, lab[n > 0])
    mp = np.full(300, 0.5)
    _, _, _, lab2 = po.oracle_unary_build(sc["Xw"], sc["obs_ptr"], sc["obs_kf"], sc["obs_kp"], sc["kf_pose"],
                                          sc["kf_intr"], sc["kf_bounds"], match_prob=mp)
    assert (lab2 == 0).sum() <= (lab == 0).sum()                   # a positive prior can only help


@pytest.mark.gpu
@pytest.mark.parametrize("n_points,n_kf,seed", [(0, 3, 1), (1, 1, 2), (257, 8, 3), (2000, 15, 4), (5000, 40, 5)])
def test_hip_unary_build_matches_oracle(po, wl, n_points, n_kf, seed):
    sc = wl.map_point_scene(n_points, n_kf, seed)
    args = (sc["Xw"], sc["obs_ptr"], sc["obs_kf"], sc["obs_kp"], sc["kf_pose"], sc["kf_intr"], sc["kf_bounds"])
    for mp in (None, np.random.default_rng(seed).uniform(0, 1, n_points)):
        o = po.oracle_unary_build(*args, match_prob=mp)
        h = pkg.unary_build(*args, match_prob=mp)
        for name, a, b in zip(("observs", "error", "depth"), o, h):
            assert cc.same_bits(a, b), name                        # bit-identical statistics
        assert np.array_equal(o[3], h[3])                          # identical rough labels


@pytest.mark.gpu
def test_hip_unary_build_feeds_the_crf(po, wl):
    """End to end as in Tracking::DynamicDetectionWithCRF: unary builder -> drop empty points -> CRF."""
    sc = wl.map_point_scene(1500, 12, seed=8)
    obs, err, dep, lab = pkg.unary_build(sc["Xw"], sc["obs_ptr"], sc["obs_kf"], sc["obs_kp"], sc["kf_pose"],
                                         sc["kf_intr"], sc["kf_bounds"])
    keep = lab >= 0                                                # Tracking.cc:1858
    xy = np.random.default_rng(1).uniform([0, 0], [640, 480], (int(keep.sum()), 2)).astype(np.float32)
    p = wl.TUM3
    res = []
    for cls in (po.OracleCRF, pkg.DenseCRFHIP):
        c = cls(int(keep.sum()), 2)
        c.set_unary_from_label(lab[keep], p["confidence"])
        f = np.stack([obs[keep] / np.float32(p["stdev_beta"]), err[keep] / np.float32(p["stdev_alpha"])], 1)
        c.add_pairwise(f.astype(np.float32), p["w1"])
        c.add_pairwise((xy / np.float32(p["point2d_stdev"])).astype(np.float32), p["w2"])
        c.inference_native(5, True)
        res.append((c.probability(), c.map()))
    assert cc.same_bits(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", nr.NAMES + ["hetero:%d" % n for n in nr.BLOCK_EDGES])
def test_hip_unary_build_scenes_match_oracle(po, name):
    """Every scene of next_row_cases, with and without match probabilities: the statistics by the scene's rule (the same bits; on
    depth_edges NaN where the oracle has NaN and the same bits elsewhere), the labels equal."""
    s = nr.scene(name)
    for with_mp in (False, True):
        o = nr.oracle(po, name, with_mp)
        h = pkg.unary_build(*nr.scene_args(s), match_prob=nr.match_prob_of(name) if with_mp else None)
        for what, a, b in zip(("observs", "error", "depth"), o, h):
            assert nr.same_statistics(name, a, b), (what, with_mp)
        assert np.array_equal(o[3], h[3]), with_mp
    if name == "bounds_exact":                                     # the verdicts stated by hand
        kept, _ = nr.bounds_verdict()
        assert np.array_equal(h[1] > 0, kept) and np.all(h[1][0::3] == 5.0)
    if name == "all_skipped":
        assert np.all(h[1] == 0) and np.all(h[2] == 0) and np.all(h[0] > 0)
    if name == "none":
        assert np.all(h[3] == -1) and np.all(h[0] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(nr.PARAM_SETS))
def test_hip_unary_build_other_parameters(po, pset):
    """Every field of lccrf_crf_params the kernel reads, away from its default."""
    fields = nr.PARAM_SETS[pset]
    for name in ("hetero:513", "order", "depth_edges", "all_skipped", "random:2000:15:4"):
        s = nr.scene(name)
        for mp in (None, nr.match_prob_of(name)):
            o = po.oracle_unary_build(*nr.scene_args(s), match_prob=mp, params=nr.params(po, **fields))
            h = pkg.unary_build(*nr.scene_args(s), match_prob=mp, params=nr.params(pkg, **fields))
            for what, a, b in zip(("observs", "error", "depth"), o, h):
                assert nr.same_statistics(name, a, b), (name, what)
            assert np.array_equal(o[3], h[3]), name
            assert len(set(o[3][o[3] >= 0].tolist())) == 2 or name in ("depth_edges", "all_skipped"), name   # the set decides something


@pytest.mark.gpu
@pytest.mark.parametrize("name,fields,mp,want", nr.threshold_cases())
def test_hip_threshold_known_answers(name, fields, mp, want):
    """The two thresholds met with equality and one step off: known answers, as on the oracle (test_next_row_cases.py)."""
    s = nr.scene(name)
    n = s["Xw"].shape[0]
    lab = pkg.unary_build(*nr.scene_args(s), match_prob=None if mp is None else np.full(n, mp), params=nr.params(pkg, **fields))[3]
    has = np.diff(s["obs_ptr"]) > 0
    assert np.all(lab[has] == want) and np.all(lab[~has] == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", nr.F64_SCENES)
def test_hip_unary_build_matches_float64(name):
    """The kernel against the float64 reference written from src/Tracking.cc, under the rule the oracle is held to: error and depth
    within the bars and labels equal wherever no observation is within LEAVE_OUT of a branch and the sum is not at its threshold."""
    s = nr.scene(name)
    for fields in [{}] + ([nr.PARAM_SETS["shifted"]] if name in nr.RANDOM or name == "hetero" else []):
        for mp in (None, nr.match_prob_of(name)):
            obs, err, dep, lab = pkg.unary_build(*nr.scene_args(s), match_prob=mp, params=nr.params(pkg, **fields))
            ref = nr.unary_build_f64(s, fields, mp)
            keep, lk = nr.compared(name, ref), nr.labels_compared(name, ref)
            assert np.array_equal(obs, ref["observs"].astype(np.float32))
            assert nr.absdiff(err, ref["error"])[keep].max(initial=0) <= nr.ERROR_BAR
            assert nr.absdiff(dep, ref["depth"])[keep].max(initial=0) <= nr.DEPTH_BAR
            assert np.array_equal(lab[lk], ref["label"][lk]) and np.all(lab[ref["observs"] == 0] == -1)


def test_unary_build_argument_checks():
    lib = pkg.lib()
    assert lib.lccrf_unary_build(0, -1, None, None, None, None, 0, None, None, None, None, None, None, None,
                                 None, None) == -1

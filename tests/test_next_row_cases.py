"""The scenes and references of tests/next_row_cases.py, checked without a GPU before the GPU tests (test_unary_builder.py,
test_bf_match.py, test_next_row_staging.py) rely on them: the oracle's restatement of the unary builder against a float64 reference
written from src/Tracking.cc, the oracle's BfMatch against a numpy one, the known answers of the edge scenes, and that each scene
rejects the fault it was built for (notes/next_row_tests.md)."""
import importlib

import numpy as np
import pytest

import crf_cases as cc
import next_row_cases as nr

pkg = importlib.import_module("lc-crf-slam_amd")

@pytest.mark.parametrize("name", nr.F64_SCENES)
def test_oracle_unary_build_matches_float64(po, name):
    """error and depth within the measured bars, labels equal, on every point whose observations are all further than LEAVE_OUT from
    a branch; on the random scenes few enough are left out and few enough sums are near their threshold."""
    for with_mp in (False, True):
        obs, err, dep, lab = nr.oracle(po, name, with_mp)
        ref = nr.unary_build_f64(nr.scene(name), match_prob=nr.match_prob_of(name) if with_mp else None)
        has = ref["observs"] > 0
        keep = nr.compared(name, ref)
        assert np.array_equal(obs, ref["observs"].astype(np.float32))
        de, dd = nr.absdiff(err, ref["error"])[keep], nr.absdiff(dep, ref["depth"])[keep]
        print(name, with_mp, "left out", int((has & ~keep).sum()), "of", int(has.sum()), "error", de.max(initial=0), "depth", dd.max(initial=0))
        assert de.max(initial=0) <= nr.ERROR_BAR and dd.max(initial=0) <= nr.DEPTH_BAR
        if name not in nr.EDGE:
            assert (has & ~keep).sum() <= nr.LEFT_OUT_SHARE * has.sum()
            close = has & (np.abs(ref["psum"] - ref["threshold"]) <= nr.LABEL_MARGIN)
            assert close.sum() <= nr.LABEL_CLOSE_SHARE * has.size
        lk = nr.labels_compared(name, ref)
        assert np.array_equal(lab[lk], ref["label"][lk])
        assert np.all(lab[~has] == -1) and np.all(ref["label"][~has] == -1)


def test_hetero_scene_depends_on_each_keyframes_camera():
    s, ref = nr.scene("hetero"), nr.f64("hetero")
    assert len(np.unique(s["kf_intr"], axis=0)) == s["kf_intr"].shape[0] and len(np.unique(s["kf_bounds"], axis=0)) >= 4
    assert tuple(s["kf_bounds"][1]) == nr.CROPPED
    for fault in ("bounds0", "intr0"):
        changed = nr.absdiff(nr.unary_build_f64(s, fault=fault)["error"], ref["error"]) > nr.ERROR_BAR
        assert changed.mean() >= 0.05, fault                      # the wrong keyframe's camera changes 5 % of the points at least


def test_order_scene_depends_on_the_order(po):
    s = nr.scene("order")
    per_point = [s["obs_kf"][a:b] for a, b in zip(s["obs_ptr"][:-1], s["obs_ptr"][1:])]
    assert any(np.any(np.diff(k) < 0) for k in per_point) and any(len(np.unique(k)) < len(k) for k in per_point)
    a, b = nr.oracle(po, "order"), nr.oracle(po, "order:reversed")
    assert np.any(cc.bits(a[1]) != cc.bits(b[1])) and np.any(cc.bits(a[2]) != cc.bits(b[2]))   # the fp32 sums follow the order given
    assert np.abs(a[1] - b[1]).max() <= nr.ERROR_BAR and np.array_equal(a[0], b[0])


def test_bounds_exact_known_verdicts(po):
    """On a bound and one step inside: kept (`u < minX` and `u > maxX` are strict); one step outside: skipped.  Stated by hand in
    next_row_cases._bounds_exact, met by the oracle and by the float64 reference."""
    kept, which = nr.bounds_verdict()
    s = nr.scene("bounds_exact")
    assert [w[3] for w in which] == ["on", "inside", "outside"] * 8 and kept.tolist() == [True, True, False] * 8
    for i, (k, axis, bound, side) in enumerate(which):
        got = nr.project_f32(s["kf_intr"][k], s["Xw"][i])["uv".index(axis)]
        if side == "on":
            assert got == bound
        else:                                                     # the nearest float u on that side: within a float step of 512 x (or y)
            assert 0 < abs(float(got) - bound) <= 2.0 ** -14 and ((got > bound) == (bound < 320)) == (side == "inside"), (which[i], got)
    obs, err, dep, lab = nr.oracle(po, "bounds_exact")
    assert np.array_equal(err > 0, kept) and np.all(err[~kept] == 0) and np.all(dep[kept] == 1) and np.all(dep[~kept] == 0)
    assert np.all(err[0::3] == 5.0)                               # on the bound the arithmetic is exact: a 3-4-5 triangle
    ref = nr.f64("bounds_exact")
    assert np.array_equal(ref["error"] > 0, kept) and np.all(ref["error"][0::3] == 5.0)


def test_depth_edges_known_answers(po):
    """z = +0 makes 1/z = +inf: u is NaN for x = 0 (0 * inf; NaN passes the bounds test, the sum turns NaN) and +inf for x != 0
    (skipped).  z = -0 is +0 by the time it is divided (0 x + 0 y + 1 (-0) = +0 in the row sum), so it goes as +0 does.  z < 0: skipped.  A subnormal z overflows 1/z to +inf in float.  1e-38: 1/z fits, u overflows for x != 0.
    1e38 and float max: 1/z is subnormal and u = cx.  z = +inf: xc = 0 * inf = NaN."""
    s = nr.scene("depth_edges")
    obs, err, dep, lab = nr.oracle(po, "depth_edges")
    n1 = len(nr.DEPTH_Z) * len(nr.DEPTH_X)
    want = {(0.0, 0): "nan", (0.0, 1): "skip", (1e-40, 0): "nan", (1e-40, 1): "skip", (1e-38, 0): "keep",
            (1e-38, 1): "skip", (1e38, 0): "keep", (1e38, 1): "keep", (-1e-3, 0): "skip", (-1e-3, 1): "skip", (nr.FLT_MAX, 0): "keep",
            (nr.FLT_MAX, 1): "keep", (np.inf, 0): "nan", (np.inf, 1): "nan"}
    i = 0
    for z in nr.DEPTH_Z:
        for xi in range(len(nr.DEPTH_X)):
            w = want[(z, xi)]                                     # -0.0 finds the entry of 0.0
            assert np.signbit(s["Xw"][i, 2]) == np.signbit(z)
            if w == "nan":
                assert np.isnan(err[i]) and np.isnan(err[i + n1]) and lab[i] == 1 and lab[i + n1] == 1   # a NaN sum compares false
            elif w == "skip":
                assert err[i] == 0 and dep[i] == 0 and err[i + n1] > 0
            else:
                assert err[i] == 5.0 and dep[i] == s["Xw"][i, 2]
            i += 1
    assert np.isnan(err).sum() == 10 and nr.same_bits_or_nan(err, err.copy())
    flipped = err.copy()
    flipped.view(np.uint32)[np.isnan(err)] ^= np.uint32(0x80000000)          # a NaN of the other sign is the same class
    assert nr.same_bits_or_nan(err, flipped) and not cc.same_bits(err, flipped)
    assert not nr.same_bits_or_nan(err, np.nan_to_num(err)) and not nr.same_bits_or_nan(dep, np.nextafter(dep, np.float32(1)))


def test_all_skipped_none_one_known_answers(po):
    obs, err, dep, lab = nr.oracle(po, "all_skipped")
    assert np.all(obs > 0) and np.all(err == 0) and np.all(dep == 0)
    want = po.oracle_rough_classify(obs, np.zeros_like(obs), np.zeros_like(obs))  # the label follows from k2 and k3 of zero
    assert np.array_equal(lab, want) and set(lab.tolist()) == {0, 1}
    obs, err, dep, lab = nr.oracle(po, "none")
    assert np.all(obs == 0) and np.all(err == 0) and np.all(dep == 0) and np.all(lab == -1)
    obs, err, dep, lab = nr.oracle(po, "one")
    assert np.all(obs == 1) and (err > 0).sum() > 30 and (err == 0).sum() > 5
    s = nr.scene("kp_float")
    assert np.array_equal(s["obs_kp"], s["obs_kp"].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name,fields,mp,want", nr.threshold_cases())
def test_oracle_threshold_known_answers(po, name, fields, mp, want):
    """`p1 + p2 + p3 <= pth` in float and `(double)(p1 + p2 + p3) + p4 <= (double)pth + 0.2` met with equality and one step off"""
    s = nr.scene(name)
    n = s["Xw"].shape[0]
    lab = po.oracle_unary_build(*nr.scene_args(s), match_prob=None if mp is None else np.full(n, mp), params=nr.params(po, **fields))[3]
    has = np.diff(s["obs_ptr"]) > 0
    assert has.any() and np.all(lab[has] == want) and np.all(lab[~has] == -1)


FAULT_TARGET = {   # fault -> scene, parameter fields, match_prob
    "intr0": ("hetero", {}, None), "bounds0": ("hetero", {}, None), "inclusive": ("bounds_exact", {}, None),
    "counted": ("hetero", {}, None), "invz_le": ("far_plane", {}, None),
    "label_lt": ("exact", dict(nr.ALL_ONE, pth=3.0, **nr.EXACT_MEANS), None),
    "float_rhs": ("exact", dict(nr.ONE_OF_THREE, u_beta=2.0), 1e-8),
}


@pytest.mark.parametrize("fault", nr.FAULTS)
def test_scenes_reject_each_fault(po, fault):
    """The float64 reference with one mistake put in leaves the bar against the oracle on a point that is not left out; without the
    mistake it stays inside on the same scene."""
    name, fields, mp = FAULT_TARGET[fault]
    s = nr.scene(name)
    mpa = None if mp is None else np.full(s["Xw"].shape[0], mp)
    obs, err, dep, lab = po.oracle_unary_build(*nr.scene_args(s), match_prob=mpa, params=nr.params(po, **fields))
    good, bad = nr.unary_build_f64(s, fields, mpa), nr.unary_build_f64(s, fields, mpa, fault=fault)
    keep, lk = nr.compared(name, good), nr.labels_compared(name, good)
    assert keep.any() and lk.any()

    def outside(ref):
        return int((nr.absdiff(err, ref["error"])[keep] > nr.ERROR_BAR).sum() + (nr.absdiff(dep, ref["depth"])[keep] > nr.DEPTH_BAR).sum() +
                   (lab[lk] != ref["label"][lk]).sum())
    print(fault, name, "outside the bar: unfaulted", outside(good), "faulted", outside(bad))
    assert outside(good) == 0 and outside(bad) >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# BfMatch
# ---------------------------------------------------------------------------------------------------------------------------
def test_bf_match_np_known_answers():
    z = np.zeros((1, 32), np.uint8)
    rows = lambda *k: np.stack([nr.prefix_row(i) for i in k])
    assert [int(cc_) for cc_ in (nr._POP[nr.prefix_row(k)].sum() for k in (0, 1, 8, 9, 255, 256))] == [0, 1, 8, 9, 255, 256]
    assert nr.bf_match_np(z, rows(256, 0, 256))[0].tolist() == [1]
    assert nr.bf_match_np(z, rows(0, 0, 256))[0].tolist() == [-1]
    assert nr.bf_match_np(z, rows(5, 3))[0].tolist() == [-1] and nr.bf_match_np(z, rows(5, 2)) == ([1], 1)
    assert nr.bf_match_np(z, rows(7, 7), 1.01)[0].tolist() == [0]                 # a tie: the lower index
    assert nr.bf_match_np(z, rows(1))[0].tolist() == [-1] and nr.bf_match_np(z, np.zeros((0, 32), np.uint8)) == ([-1], 0)
    assert len(nr.boundary_pairs()) == 564                           # 1128 two-row calls


@pytest.mark.parametrize("n_train", nr.BF_TRAIN)
def test_oracle_bf_match_equals_numpy(po, n_train):
    for n_query in nr.BF_QUERY:
        q, t = nr.planted(n_query, n_train, seed=n_train)
        for ratio in nr.BF_RATIOS:
            o, no = po.oracle_bf_match(q, t, ratio)
            r, nn = nr.bf_match_np(q, t, ratio)
            assert np.array_equal(o, r) and no == nn, (n_query, ratio)


def test_oracle_bf_match_ties_and_distance_256_equal_numpy(po):
    """the tie and top-distance sets of the GPU tests (test_bf_match.py): oracle and numpy agree, the lowest index wins"""
    z = np.zeros((3, 32), np.uint8)
    for n_train in (2, 40, 1030):
        t = np.full((n_train, 32), 0xff, np.uint8)
        for ratio, want in ((0.6, -1), (1.01, 0)):
            assert po.oracle_bf_match(z, t, ratio)[0].tolist() == nr.bf_match_np(z, t, ratio)[0].tolist() == [want] * 3
        t[n_train - 1] = 0
        assert po.oracle_bf_match(z, t)[0].tolist() == nr.bf_match_np(z, t)[0].tolist() == [n_train - 1] * 3
    for rows, n_train in (((3, 19), 64), ((1023, 1024), 1500), ((5, 2053), 2100)):
        q, t = nr.planted(20, n_train, seed=rows[1], share=0.0)
        near = q[4].copy(); near[:6] ^= 0xff
        t[rows[0]] = near; t[rows[1]] = near
        o, r = po.oracle_bf_match(q, t, 1.01), nr.bf_match_np(q, t, 1.01)
        assert np.array_equal(o[0], r[0]) and o[1] == r[1] and o[0][4] == rows[0]
    q, _ = nr.planted(40, 2, seed=5, share=0.0)
    t = np.tile(q[7], (1500, 1))
    assert po.oracle_bf_match(q, t, 1.01)[0].tolist() == nr.bf_match_np(q, t, 1.01)[0].tolist() == [-1 if i == 7 else 0 for i in range(40)]


def test_oracle_bf_match_ratio_boundary_pairs(po):
    """every (d0, d1) within 1 of d0 = 0.6 d1, in both row orders: the oracle, the numpy reference and the plain inequality agree"""
    z = np.zeros((1, 32), np.uint8)
    accepted = 0
    for d0, d1 in nr.boundary_pairs():
        want = d0 < d1 * 0.6
        accepted += want
        for order in ((d0, d1), (d1, d0)):
            t = np.stack([nr.prefix_row(order[0]), nr.prefix_row(order[1])])
            first = 0 if d0 == d1 else order.index(d0)
            o = po.oracle_bf_match(z, t)[0].tolist()
            assert o == nr.bf_match_np(z, t)[0].tolist() == [first if want else -1], (d0, d1, order)
    assert 200 < accepted < 400


def test_next_row_argument_checks():
    """without a GPU: the train index has 22 bits, and a NaN ratio is no ratio"""
    lib = pkg.lib()
    q = np.zeros((1, 32), np.uint8)
    out = np.zeros(1, np.int32)
    i32p = out.ctypes.data_as(lib.lccrf_bf_match.argtypes[6])
    assert lib.lccrf_bf_match(0, 1, q.ctypes.data, 1 << 22, q.ctypes.data, 0.6, i32p, None) == -6       # LCCRF_E_CAPACITY
    assert b"4194303" in lib.lccrf_last_error()
    assert lib.lccrf_bf_match(0, 1, q.ctypes.data, 1, q.ctypes.data, float("nan"), i32p, None) == -1     # LCCRF_E_INVALID
    assert lib.lccrf_bf_match(0, 1, q.ctypes.data, 1, q.ctypes.data, -0.5, i32p, None) == -1

"""The cases of tests/lattice_tie_cases.py, checked without a GPU so that the GPU tests on them (tests/test_lattice_ties.py) mean what
they say: the cases CONTAIN exact rounding ties, double ties and rank ties in the numbers promised; the float32 restatement that
composed and classified them reproduces the oracle's barycentric bits and keys; each mutant rule (round half AWAY from zero for half to
even; '<=' for '<' in the rank compares) moves the keys of points of every case -- and moves none, or few, on the inputs the suite had
before (the gap, kept as a test); the oracle reproduces tests/golden/ties.npz, which the reference build itself wrote.
Figures: notes/lattice_ties.md."""
import os

import numpy as np
import pytest

import crf_cases as cc
import lattice_tie_cases as tc

ALL = tc.GENERIC + tc.SLAM + tc.BIG
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ties.npz")


def _feats(name):
    return [f for f, _ in tc.problem(name)["kernels"]]


@pytest.mark.parametrize("name", tc.GENERIC)
def test_generic_cases_hold_every_class_of_tie(name):
    """>= 32 exact single rounding ties with k of both parities and both signs and the tying coordinate i covering 0, d and one between;
    >= 16 axis double ties; >= 16 exact rank ties away from the origin.  (d = 1: el = (c, -c), both coordinates tie or neither -- every
    rounding tie is a double one, so the 32 + 16 are all counted there; i covers 0 and d = 1, nothing lies between.)"""
    pb = tc.problem(name)
    d = int(name[6:])
    f = pb["kernels"][0][0]
    assert pb["N"] == 256 and pb["L"] == 3 and len(pb["kernels"]) == 1 and f.shape == (256, d)
    c = tc.classify(f)
    info = pb["tie_info"]
    print(name, {k: c[k] for k in ("single", "double", "rank")}, "tries:", info["round"]["tries"], info["axis"]["tries"], info["rank"]["tries"])
    if d == 1:
        assert c["single"] == 0 and c["double"] >= 32 + 16
        s = tc.simplex_f32(f)
        k = s["k"][s["double"], 0]
    else:
        assert c["single"] >= 32 and c["double"] >= 16
        assert {0, d} <= c["i"] and (d < 2 or c["i"] & set(range(1, d)))
        k = c["k"]
    assert {0, 1} <= set((k % 2).tolist()) and (k < 0).any() and (k >= 0).any()
    assert info["round"]["hits"] >= 32 and info["axis"]["hits"] >= 16
    assert c["rank"] >= 16
    # every emitted hit came with its two neighbouring floats (3 rows per hit)
    assert info["round"]["hits"] * 3 + info["axis"]["hits"] + min(info["rank"]["hits"], 24) + info["tail"] <= 256


@pytest.mark.parametrize("name", tc.SLAM)
def test_slam_cases_hold_every_class_in_both_terms_inside_the_frames_ranges(name, wl):
    pb = tc.problem(name)
    N = int(name[9:])
    assert pb["N"] == N and pb["L"] == 2 and [f.shape for f in _feats(name)] == [(N, 2), (N, 2)]
    assert [float(w) for _, w in pb["kernels"]] == [10.0, 30.0]
    assert (N % 4 != 0) == (name == "ties:slam2047")              # the second has a phantom point
    plain = wl.slam_problem(N, seed=50 + N)
    for k, f in enumerate(_feats(name)):
        c = tc.classify(f)
        print(name, k, {x: c[x] for x in ("single", "double", "rank")})
        assert c["single"] >= 12 and c["double"] >= 5 and c["rank"] >= 12
        assert {0, 1} <= set((c["k"] % 2).tolist())
        g = plain["kernels"][k][0]
        on_axis = f[:, 1] == 0                                    # the axis points: on the edge y = 0 of features that are >= 0
        assert on_axis.sum() == c["double"] and (f[~on_axis] >= g.min(0)).all() and (f <= g.max(0)).all() and (f >= 0).all()
        assert (f != g).any(1).sum() >= 50


@pytest.mark.parametrize("name", tc.BIG)
def test_large_cases_are_a_tenth_tie_points(name):
    pb = tc.problem(name)
    f = pb["kernels"][0][0]
    assert pb["N"] == 8192 and len(pb["kernels"]) == 1
    s = tc.simplex_f32(f)
    n = int((s["round_tie"].any(1) | (s["rank_tie"] & (f != 0).any(1))).sum())
    print(name, n, "tie points")
    assert 10 * n >= 8192 and s["single"].sum() >= 32 and s["double"].sum() >= 16


@pytest.mark.parametrize("name", ALL)
def test_restatement_reproduces_the_oracles_simplex(po, name):
    """bary bit for bit, and the key of every corner of every point (the oracle's vertex table read through its offsets)"""
    pb = tc.problem(name)
    o = cc.setup(po.OracleCRF, pb)
    for k, (f, _) in enumerate(pb["kernels"]):
        s, ko = tc.simplex_f32(f), o.kernel(k)
        assert cc.same_bits(s["bary"], ko["bary"]), (name, k)
        assert np.array_equal(ko["keys"][ko["offset"]], s["keys"]), (name, k)
    o.close()


@pytest.mark.parametrize("name", ALL)
def test_both_mutants_move_keys_on_the_new_cases(name):
    """round-half-away moves the keys of >= 6 points of every case; '<=' of >= 8 where a term has d >= 3.  d = 1, d = 2 and the SLAM
    frames have only the bisected rank ties: measured 24 (ties:d1: the keys of 24 bisected ties move, and of 4 points at the origin), 24
    (ties:d2), 24 and 72 (the SLAM frames, 12 and 36 per term) -- every bisected tie moves, asserted as measured."""
    away = sum(tc.classify(f)["away_changed"] for f in _feats(name))
    loose = sum(int((tc.changed_points(f, strict=False) & (f != 0).any(1)).sum()) for f in _feats(name))
    print(name, "round half away:", away, "points; '<=':", loose, "points away from the origin")
    assert away >= 6
    floor = {"ties:d1": 24, "ties:d2": 24, "ties:slam256": 24, "ties:slam2047": 72}.get(name, 8)
    assert loose >= floor


@pytest.mark.parametrize("d", range(1, 9))
def test_the_same_mutants_pass_unseen_on_the_inputs_the_suite_had(wl, d):
    """generic_problem(203, [d], 3, seed=5, lattice_ties=True), the recipe of the golden generators: NO exact rounding tie (the .0 / .5
    features meet irrational elevation scales), so half-away-from-zero changes nothing; '<=' moves 0 to 10 points away from the origin
    where the new case of the same d moves 24 to 73."""
    f = wl.generic_problem(203, [d], 3, seed=5, lattice_ties=True)["kernels"][0][0]
    s = tc.simplex_f32(f)
    assert not s["round_tie"].any()
    assert not tc.changed_points(f, rounding="away").any()
    old = int((tc.changed_points(f, strict=False) & (f != 0).any(1)).sum())
    g = tc.problem("ties:d%d" % d)["kernels"][0][0]
    new = int((tc.changed_points(g, strict=False) & (g != 0).any(1)).sum())
    print("d = %d: '<=' moves %d points of the old inputs, %d of the new" % (d, old, new))
    assert old <= 10 and new >= max(24, 2 * old)


def test_slam_inputs_the_suite_had_hold_no_tie_at_all(wl):
    for f, _ in wl.slam_problem(2000, seed=11)["kernels"]:
        c = tc.classify(f)
        assert c["single"] == c["double"] == c["rank"] == c["away_changed"] == c["loose_changed"] == 0


@pytest.mark.parametrize("name", tc.GENERIC + tc.SLAM)
def test_oracle_reproduces_the_reference_fixture(po, name):
    """tests/golden/ties.npz (written by the reference build: tests/golden/make_golden_ties.py) holds the generators' inputs, and the
    oracle gives its V, norm, offset, bary, nbr, Q trace and labels bit for bit"""
    z = np.load(FIXTURE)
    p = name.replace(":", "_")
    assert name in list(z["cases"])
    pb, gen = cc.case_problem(z, p), tc.problem(name)
    assert pb["N"] == gen["N"] and pb["L"] == gen["L"]
    for (f, w), (g, v) in zip(pb["kernels"], gen["kernels"]):
        assert cc.same_bits(f, g) and np.float32(w) == np.float32(v)
    o = cc.setup(po.OracleCRF, pb)
    for k in range(len(pb["kernels"])):
        ko = o.kernel(k)
        assert ko["V"] == int(z["%s_V%d" % (p, k)])
        for what in ("norm", "offset", "bary", "nbr"):
            assert cc.same_bits(ko[what], z["%s_%s%d" % (p, what, k)]), (name, k, what)
    T, relax = int(z["iters"]), float(z["relax"])
    assert cc.same_bits(o.run_trace(T, relax), z[p + "_trace"])
    o.build_map()
    assert np.array_equal(o.map(), z[p + "_map"])
    o.close()


def test_fixture_is_no_larger_than_the_largest_before_it():
    assert os.path.getsize(FIXTURE) <= 575950

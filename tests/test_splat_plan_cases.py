"""tests/splat_plan_cases.py without a GPU: the restatement describes the REAL lattice (V and the neighbour relation against the oracle
on three shapes), the case table of tests/test_splat_window.py covers every class it claims, and every windowed case sends values
through the halo in its first, an interior and its last window."""
import numpy as np
import pytest

import splat_plan_cases as sp


def test_constants_are_read_from_the_sources():
    c = sp.constants()
    assert c["windows"][0] < c["windows"][1] < c["windows"][2] == c["max_window"] and c["max_dist"] < c["max_window"] // c["halo_share"] + 1
    assert c["max_passes"] == 3 and c["kNdistAxes"] >= 3


@pytest.mark.parametrize("shape", ["box2d", "gauss3d_phantom", "gauss4d"])
def test_restatement_has_the_oracles_vertices_and_neighbours(po, wl, shape):
    import crf_cases as cc
    if shape == "box2d":
        f = sp.BY_NAME["w512_F1"].frames()[0]["kernels"][0][0]
    elif shape == "gauss3d_phantom":
        f = wl.generic_problem(2501, [3], 2, seed=8, spread=3.0)["kernels"][0][0]      # (one point into the last block of four)
    else:
        f = wl.generic_problem(1500, [4], 2, seed=9, spread=2.5)["kernels"][0][0]
    N, d = f.shape
    lat = sp.Lattice(f)
    o = cc.setup(po.OracleCRF, dict(N=N, L=2, unary=np.zeros((N, 2), np.float32), kernels=[(f, np.float32(1.0))]))
    ko = o.kernel(0)
    o.close()
    assert lat.V == ko["V"]
    # same partition of the entries into vertices: a one-to-one map between the two numberings on the real points' vertices
    mine, ref = lat.entry_vertex[:N].ravel(), ko["offset"].ravel()
    pairs = np.unique(np.stack([mine, ref], 1), axis=0)
    assert len(pairs) == len(np.unique(mine)) == len(np.unique(ref))
    to_ref = np.full(lat.V, -2, np.int64)                      # (-2: a vertex of phantom points only, unknown to `offset`)
    to_ref[pairs[:, 0]] = pairs[:, 1]
    assert (to_ref == -2).sum() <= 3 * (d + 1)
    checked = 0
    for j in range(d + 1):
        n2 = lat.nbr[j]
        known = (to_ref >= 0) & ((n2 < 0) | (to_ref[np.maximum(n2, 0)] >= 0))
        want = np.where(n2 >= 0, to_ref[np.maximum(n2, 0)], -1)[known]
        got = ko["nbr"][j, to_ref[known], 1]
        phantom_side = (want < 0) & (got >= 0)                 # (the oracle's neighbour may be a phantom-only vertex)
        assert phantom_side.sum() <= 3 * (d + 1) and np.array_equal(want[~phantom_side], got[~phantom_side]), j
        checked += int(known.sum())
        # ... and n1 is the inverse relation
        has = n2 >= 0
        ok = has & (to_ref >= 0) & (to_ref[np.maximum(n2, 0)] >= 0)
        assert np.array_equal(ko["nbr"][j, to_ref[n2[ok]], 0], to_ref[np.nonzero(ok)[0]]), j
    assert checked > (d + 1) * lat.V * 0.99


def in_class(case, name, p):
    c = sp.constants()
    w256, w512, w1024 = c["windows"]
    lim = c["max_window"] // c["halo_share"]
    p = dict(p, nd=p["nd"] + [0, 0])                           # (d = 1 has no axis 2)
    return {
        "window256": p["window"] == w256, "window512": p["window"] == w512, "window1024": p["window"] == w1024,
        "F1": case.F == 1, "F2": case.F == 2, "F3": case.F == 3, "F8": case.F == 8,
        "P1": p["passes"] == 1, "P2": p["passes"] == 2, "P3": p["passes"] == 3,
        "P==D1": p["passes"] == p["D1"], "P==D1-1": p["passes"] == p["D1"] - 1,
        "halo<=32": w256 // 8 - 2 <= p["halo"] <= w256 // 8 and p["window"] == w256,
        "halo>=33": w256 // 8 < p["halo"] <= w256 // 8 + 2 and p["window"] == w512,
        "halo<=64": w512 // 8 - 2 <= p["halo"] <= w512 // 8 and p["window"] == w512,
        "halo>=65": w512 // 8 < p["halo"] <= w512 // 8 + 2 and p["window"] == w1024,
        "odd_halo": p["halo"] % 2 == 1 and p["window"] > 0,
        "sum<=128": p["passes"] == 3 and lim - 4 <= p["halo"] <= lim,
        "sum>128": p["passes"] == 2 and 1 + p["nd"][1] + p["nd"][2] > lim and p["nd"][2] <= c["max_dist"] and p["window"] == w1024,
        "nd1_120_127": p["passes"] == 2 and 120 <= p["nd"][1] <= c["max_dist"] and p["halo"] <= lim,
        "nd1>127": p["nd"][1] > c["max_dist"] and p["passes"] == 1 and p["window"] == 0,
        "d1": p["D1"] == 2, "d3": p["D1"] == 4, "d4": p["D1"] == 5,
        "left_odd": p["passes"] == 3 and (p["D1"] - 3) % 2 == 1, "left_even": p["passes"] == 3 and p["D1"] - 3 == 2,
        "demoted": case.F == 1 and p["D1"] > c["demote_above_D1"] and p["passes"] == 1 and 1 <= p["nd"][1] <= c["max_dist"]
                   and (case.passes_cap == 2 or p["nd"][2] > c["max_dist"] or 1 + p["nd"][1] + p["nd"][2] > lim),
        "cap2": case.passes_cap == 2,
        "coarse": len(case.terms) == 2 and p["window"] > 0 and case.plan(1)["long_mode"] in (1, 2) and case.plan(1)["passes"] == 0,
        "mixed": case.F == 3 and case.frame_specs[1] is None,
        "object": case.api == "object" and case.F == 1 and p["window"] > 0,
    }[name]


@pytest.mark.parametrize("case", sp.CASES, ids=[c.name for c in sp.CASES])
def test_case_is_what_the_table_says(case):
    c = sp.constants()
    p = case.plan(0)
    assert case.max_points >= c["kPermMinPointsDefault"]
    for name in sorted(case.classes):
        assert in_class(case, name, p), (case.name, name, p)
    assert (p["window"] == 0) == bool(case.classes & sp.NO_WINDOW)
    for k in range(len(case.terms)):
        pk = case.plan(k)
        if "coarse" not in case.classes or k == 0:
            assert pk["long_mode"] == 0 and pk["per_row"] < c["long_per_row"], (case.name, k, pk["per_row"])
    if "mixed" in case.classes:                                  # the halo is the widest frame's; the narrow frame ends far below maxV
        lats = case.lattices(0)
        narrow, wide = sorted((l for l in lats if l), key=lambda l: l.V)
        assert 1 + narrow.ndist(1) + narrow.ndist(2) <= sp.constants()["windows"][0] // 8 < p["halo"]      # (its own distances fit window 256)
        assert sp.plan_of([wide], case.max_points, 3)["halo"] == p["halo"]
        core = p["window"] - 2 * p["halo"]
        assert (narrow.V + core - 1) // core + 2 <= (p["maxV"] + core - 1) // core      # whole trailing workgroups exit
        assert wide.N < narrow.N


def test_table_covers_every_class():
    plans = {c.name: c.plan(0) for c in sp.CASES}
    shapes = {(p["lanes"], p["vertices_per_lane"]) for p in plans.values() if p["window"]}
    assert shapes == {(256, 1), (512, 1), (256, 2), (512, 2), (1024, 1), (256, 4)}
    seen = {(plans[c.name]["window"], c.F) for c in sp.CASES if c.passes_cap is None}
    for w in sp.constants()["windows"]:
        for F in (1, 2, 3):
            assert (w, F) in seen, (w, F)
    assert any(c.F == 8 and plans[c.name]["window"] for c in sp.CASES)
    claimed = set().union(*[c.classes for c in sp.CASES])
    for name in ("halo<=32", "halo>=33", "halo<=64", "halo>=65", "odd_halo", "sum<=128", "sum>128", "nd1_120_127", "nd1>127", "P1", "P2", "P3",
                 "d1", "d3", "d4", "left_odd", "left_even", "demoted", "cap2", "coarse", "mixed", "object"):
        assert name in claimed, name
    assert {plans[c.name]["D1"] for c in sp.CASES if "P==D1" in c.classes} == {2, 3}           # d = 1 and d = 2
    assert any("demoted" in c.classes and c.passes_cap is None for c in sp.CASES) and any("demoted" in c.classes and c.passes_cap == 2 for c in sp.CASES)
    assert {plans[c.name]["window"] for c in sp.CASES if c.passes_cap == 2} >= {0, 256, 512}
    seq = [plans[n] for n in sp.REBUILD_SEQUENCE]
    assert seq[0] == seq[2] and seq[1]["halo"] < seq[0]["halo"] and seq[1]["window"] < seq[0]["window"]
    assert len({sp.BY_NAME[n].F for n in sp.REBUILD_SEQUENCE}) == 1


@pytest.mark.parametrize("case", [c for c in sp.CASES if not c.classes & sp.NO_WINDOW], ids=lambda c: c.name)
def test_values_cross_the_window_edges(case):
    """In the first, an interior and the last window some vertex has a neighbour along a pass of the window that another workgroup
    owns (so a wrong halo changes a result there), and nothing a vertex depends on lies farther away than the halo."""
    p = case.plan(0)
    assert p["window"] > 0
    for lat in (l for l in case.lattices(0) if l):
        assert sp.halo_reach(lat, p) <= p["halo"]
    lat = max((l for l in case.lattices(0) if l), key=lambda l: l.V)
    nw, hit = sp.cross_edge_windows(lat, p)
    assert nw >= 3 and 0 in hit and nw - 1 in hit and any(0 < h < nw - 1 for h in hit), (case.name, nw, hit[:3], hit[-3:])

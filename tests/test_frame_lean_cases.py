"""The deterministic cases of the half-CU frame kernel's grid build (tests/frame_lean_cases.py), checked on the CPU:
  (1) every kind is what its name claims, from the oracle's own lattice (signs of u / v, cell counts on both sides of 32768,
      V = 1344, E against 16 V, row lengths, what the phantom points do to the far clouds), and expected_route() sorts it as listed;
  (2) the oracle equals the reference's own headers on every distinct case, bit for bit: V, norm, Q after 0 and 5 iterations, MAP;
  (3) the comparison the GPU tests use (compare_batch) rejects a reference with one flipped Q bit, one flipped label, V off by one,
      one label bit set beyond n_points.
"""
import numpy as np
import pytest

import crf_cases as cc
import frame_lean_cases as fc

FLAG = {"cells_over", "cells_over0", "cells_tall_over", "cells_flat_over", "far_far_m1", "v_over", "v_over_by_1", "guard_out", "guard_out_neg", "guard_out_u", "k0_wide"}

_MODELS = {}


def _models(wl, po, top):
    if top not in _MODELS:
        cs = fc.cases(wl, top) + (fc.plan_cases(wl) if top == 2048 else [])
        _MODELS[top] = {name: (pb,) + fc.expected_route(pb, po) for name, pb in cs}
    return _MODELS[top]


@pytest.mark.parametrize("top", fc.TOPS)
def test_every_kind_is_what_it_claims(po, wl, top):
    ms = _models(wl, po, top)
    assert len(ms) == len(fc.cases(wl, top)) + (4 if top == 2048 else 0)        # (names are distinct)
    assert max(pb["N"] for pb, _, _, _ in ms.values()) == top == ms["slam"][0]["N"]

    def m(name, k):
        return ms[name][3][k]

    # the routes: the closed rules send exactly the cases built to break them to the fallback
    for name, (pb, route, why, _) in ms.items():
        assert route == ("plan" if name in fc.PLAN_KINDS else "flag" if name in FLAG else "fit"), (name, route, why)
    # sign recovery from the packed word: every point of kernel 1 (kernel 0) has u < 0 and v < 0; boxes with both signs
    for name, k in (("negative", 1), ("negative0", 0)):
        assert m(name, k)["u"].max() < 0 and m(name, k)["v"].max() < 0 and ms[name][0]["N"] % 4 == 0
    for name, k in (("straddle", 1), ("straddle_m1", 1), ("straddle0", 0)):
        x = m(name, k)
        assert x["u"].min() < 0 < x["u"].max() and x["v"].min() < 0 < x["v"].max()
    for name in ("negative0", "straddle0", "ties0"):
        assert m(name, 0)["rowmax"] >= 64 and m(name, 0)["V"] <= fc.MAX_V0
    # far clouds: a small box away from the origin while N % 4 == 0; the phantom points of N - 1 pull the origin in
    for name, lo, hi in (("far_near", 4096, 16384), ("far_far", 49152, 1 << 30)):
        a, b = m(name, 1), m(name + "_m1", 1)
        assert ms[name][0]["N"] % 4 == 0 and ms[name + "_m1"][0]["N"] == top - 1
        assert a["u"].min() > 50 and a["v"].max() < 0 and a["cells"] < 2048
        assert b["u"].min() == 0 and b["v"].max() == 0 and lo < b["cells"] < hi
        assert np.array_equal(b["u"][:-1], a["u"][:top - 1]) and b["V"] >= a["V"] - 3
    # the id map's limit from both sides, on either kernel: within one row of 32768, and one column more
    for sfx, k in (("", 1), ("0", 0)):
        a, b = m("cells_max" + sfx, k), m("cells_over" + sfx, k)
        assert fc.MAX_CELLS - a["Hp"] < a["cells"] <= fc.MAX_CELLS < b["cells"]
        assert (b["Wp"], b["Hp"]) == (a["Wp"] + 1, a["Hp"]) and a["V"] == b["V"] == 6
    # ... the most cells a frame can have (Hp is a multiple of 3), and boxes of one column of u / one row of v, with their twins
    assert m("cells_top", 1)["cells"] == 32766 == fc.MAX_CELLS - 2
    a, b = m("cells_tall", 1), m("cells_tall_over", 1)
    assert (a["Wp"], a["Hp"], b["Wp"], b["Hp"]) == (5, 6552, 5, 6555) and a["cells"] <= fc.MAX_CELLS < b["cells"]
    a, b = m("cells_flat", 1), m("cells_flat_over", 1)
    assert (a["Wp"], a["Hp"], b["Wp"], b["Hp"]) == (3640, 9, 3641, 9) and a["cells"] <= fc.MAX_CELLS < b["cells"] == fc.MAX_CELLS + 1
    # the vertex limit of kernel 1: every point its own three vertices
    assert (ms["v_max"][0]["N"], m("v_max", 1)["V"], m("v_max", 1)["rowmax"]) == (448, fc.MAX_V, 1)
    assert m("v_over", 1)["V"] == 1356 and m("v_over_by_1", 1)["V"] == fc.MAX_V + 1
    assert ms["v_over"][0]["N"] % 4 == 0 and ms["v_over_by_1"][0]["N"] % 4 == 0
    for name in ("v_max", "v_over", "v_over_by_1"):
        assert m(name, 0)["V"] <= fc.MAX_V0 and m(name, 1)["cells"] < fc.MAX_CELLS
    # which kernel ranks by bitmap and which by lists (frame_build.h: E >= 16 V and 5 V W + 64 bytes beside the tables)
    for name in ("bitmap1_line", "bitmap1_cell"):
        x = m(name, 1)
        W = (((top + 31) >> 5) + 3) & ~3
        assert x["E"] >= 16 * x["V"] and 5 * x["V"] * W + 64 + 16384 < fc.LDS
    if top == 2048:
        assert 150 <= m("bitmap1_line", 1)["V"] <= 250 and m("bitmap1_line", 1)["cells"] > 10000
    assert m("bitmap1_cell", 1)["V"] == 3 and m("bitmap1_cell", 1)["cells"] == 45
    assert m("slam", 0)["E"] >= 16 * m("slam", 0)["V"] and m("slam", 1)["E"] < 16 * m("slam", 1)["V"]
    x = m("list0", 0)
    assert x["E"] < 16 * x["V"] and x["rowmax"] >= 64 and x["V"] <= fc.MAX_V0
    # ties: every coordinate a multiple of 0.5, some points at exact zero
    for name, k in (("ties", 1), ("ties0", 0)):
        f = ms[name][0]["kernels"][k][0]
        assert np.array_equal(f * 2, np.round(f * 2)) and (f == 0).all(1).sum() > 3
    # rows on both sides of the 8-padded lists' units
    assert set(m("rows8", 1)["rows"].tolist()) >= {7, 8, 9, 15, 16, 17} and m("rows8", 1)["E"] < 16 * m("rows8", 1)["V"]
    assert [ms["tiny%d" % n][0]["N"] for n in range(6)] == list(range(6))
    # the guard: the largest |coordinate| of a remainder-0 key just inside 32000 (no phantoms), and beyond it but inside int16
    for name in ("guard_in", "guard_in_neg", "guard_in_u"):
        assert 31900 <= m(name, 1)["rem0"] < fc.GUARD and ms[name][0]["N"] % 4 == 0
    assert m("guard_in", 1)["v"].max() > 31900 and m("guard_in_neg", 1)["v"].min() < -31900
    assert m("guard_in_u", 1)["u"].max() > 21300 and m("guard_in_u", 1)["v"].min() < -31900
    for name in ("guard_out", "guard_out_neg", "guard_out_u"):
        assert fc.GUARD <= m(name, 1)["rem0"] < 32700
    # kernel 0 beyond the chain lanes' vertex limit; kernel 0 within it and without a row of 64 products
    assert m("k0_wide", 0)["V"] > fc.MAX_V0
    assert m("k0_short", 0)["V"] <= fc.MAX_V0 and m("k0_short", 0)["rowmax"] < 64


def test_plan_cases_are_beyond_the_closed_rules(po, wl):
    """No closed rule rejects them; the bound of the LDS plan is above the limit, so the plan itself decides."""
    for name, pb in fc.plan_cases(wl):
        route, why, m = fc.expected_route(pb, po)
        assert route == "plan" and pb["N"] == 2048, (name, route, why)
        assert m[0]["V"] <= fc.MAX_V0 and m[1]["V"] <= fc.MAX_V and max(m[k]["cells"] for k in range(2)) <= fc.MAX_CELLS
        assert fc.plan_bound(2048, m[0]["V"], m[1]["V"]) > fc.LDS
    # a usual SLAM frame of the largest size is within the bound
    assert fc.plan_bound(2048, 124, 1165) <= fc.LDS


@pytest.mark.parametrize("top", fc.TOPS)
def test_oracle_equals_the_reference_on_every_case(po, wl, top):
    if not po.have_ref():
        pytest.skip("the reference's shim is not built here")
    for name, pb in fc.cases(wl, top) + (fc.plan_cases(wl) if top == 2048 else []):
        if pb["N"] == 0:
            continue
        o, r = cc.setup(po.OracleCRF, pb), cc.setup(po.RefCRF, pb)
        for k in range(2):
            assert o.kernel(k)["V"] == r.kernel(k)["V"], (name, k)
            assert cc.same_bits(o.kernel(k)["norm"], r.kernel(k)["norm"]), (name, k)
        for n_iter in (0, 5):
            o.inference_native(n_iter, True)
            r.inference_native(n_iter, True)
            assert cc.same_bits(o.probability(), r.probability()), (name, n_iter)
            assert np.array_equal(o.map(), r.map()), (name, n_iter)
        o.close(); r.close()


def test_the_comparison_rejects_planted_faults(po, wl):
    names = ["slam", "negative", "tiny3", "tiny0", "v_max"]
    pbs = dict(fc.cases(wl, 512))
    refs = [fc.reference(pbs[n], po) for n in names]
    which = [f % len(refs) for f in range(12)]
    got = fc.fake_batch(refs, which, 512)
    fc.compare_batch(got, refs, which)                       # the batch equals its references

    def rejected(change, what):
        bad = [dict(r, Q=r["Q"].copy(), map=r["map"].copy(), V=list(r["V"])) for r in refs]
        change(bad)
        with pytest.raises(AssertionError, match=what):
            fc.compare_batch(got, bad, which)

    def flip_q(bad):
        bad[1]["Q"].view(np.uint32)[311, 1] ^= 1             # the last mantissa bit of one probability
    rejected(flip_q, "Q differs")

    def flip_label(bad):
        bad[0]["map"][511] ^= 1
    rejected(flip_label, "labels differ")

    def v_off(bad):
        bad[4]["V"][1] += 1
    rejected(v_off, "V of kernel 1")

    def v_off_empty(bad):
        bad[3]["V"][0] = 1                                   # an empty frame reports V = 0
    rejected(v_off_empty, "V of kernel 0")

    def bit_beyond(bad):
        b = fc.expected_bits(bad[2], 8).copy()
        b[0] |= np.uint64(1) << np.uint64(3)                 # tiny3 has points 0 .. 2: bit 3 is the first one beyond the frame
        bad[2]["bits"] = b
    rejected(bit_beyond, "label bits differ")

    def bit_far_beyond(bad):
        b = fc.expected_bits(bad[3], 8).copy()
        b[7] |= np.uint64(1) << np.uint64(63)                # the last bit of the row, in an empty frame
        bad[3]["bits"] = b
    rejected(bit_far_beyond, "label bits differ")
    # ... and a batch with a stray bit beyond the frame is rejected by the honest references
    got["bits"][2, 1] = np.uint64(1)
    with pytest.raises(AssertionError, match="frame 2 .*label bits differ"):
        fc.compare_batch(got, refs, which)

"""tests/blur_plan_cases.py without a GPU: the restated rule is sound (its counts add up, in closed form and as a walk over the passes),
the lattice sizes it rests on are the oracle's, and the case table of tests/test_blur_plan.py holds what it claims -- every route is
the expected route of a release-library case, both sides of the vertex bound, odd and even V, and in the compact-table cases a last
odd vertex whose neighbours make k_blur2c's tail branch and both bases of its block count."""
import numpy as np
import pytest

import blur_plan_cases as bp


def test_constants_are_read_from_the_sources():
    c = bp.constants()
    assert c["kPairFuseMaxVertices"] == 700000 and c["kPairFuseMaxFrames"] == 1 and c["kSliceBlurMaxFrames"] == 1
    assert 1 < c["kNbrcMinFrames"] <= c["kNbrcMaxFrames"] < c["kBlurNtMinFrames"]      # (why k_blur2c has no non-temporal form)
    assert c["kNbrcBlock"] == 64 and c["span_limit"] == 0xffff and c["demote_above_D1"] == 3


def walk(D1, j0, F, maxV, table, first, compact, no_pair_fuse):
    """the rule once more, as the walk over the passes that the launcher makes (route_counts is the closed form)"""
    c = bp.constants()
    pairs = not no_pair_fuse and (F <= c["kPairFuseMaxFrames"] or F * maxV <= c["kPairFuseMaxVertices"])
    in_slice = j0 < D1 and (((D1 - j0) % 2 == 1 and D1 >= 3) if pairs else F <= c["kSliceBlurMaxFrames"])
    p = dict.fromkeys(bp.PLAN_FIELDS, 0)
    p["in_splat"], p["in_slice"], p["first_table_pair"] = j0, int(in_slice), -1
    j, end = j0, D1 - int(in_slice)
    while j < end:
        if pairs and j + 1 < end:
            t = table and j - first >= 0 and (j - first) % 2 == 0
            p["paired_table" if t else "paired_plain"] += 2
            if t and p["first_table_pair"] < 0:
                p["first_table_pair"] = (j - first) // 2
            j += 2
        else:
            p["alone_compact" if compact else "alone_32bit"] += 1
            j += 1
    p["nontemporal"] = int(p["alone_32bit"] > 0 and F >= c["kBlurNtMinFrames"])
    return p


def test_closed_form_and_walk_agree_and_the_counts_add_up():
    n = 0
    for D1 in range(2, 10):
        for j0 in range(0, min(D1, 3) + 1):
            for F in (1, 2, 3, 5, 6, 8):
                for maxV in (1000, 700000 // F, 700000 // F + 1):
                    for table in (False, True):
                        for first in (0, 1):
                            for compact in (False, True):
                                for off in (False, True):
                                    a = bp.route_counts(D1, j0, F, maxV, table, first, compact, off)
                                    assert a == walk(D1, j0, F, maxV, table, first, compact, off), (D1, j0, F, maxV, table, first, compact, off)
                                    assert sum(a[r] for r in bp.ROUTES) == D1
                                    assert a["paired_table"] % 2 == 0 and a["paired_plain"] % 2 == 0 and a["in_slice"] <= 1
                                    assert not (a["paired_table"] and a["paired_plain"]) and (a["first_table_pair"] >= 0) == (a["paired_table"] > 0)
                                    n += 1
    assert n == 8928


@pytest.mark.parametrize("case", bp.CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(po, case):
    exp = case.expected()
    assert len(exp) == len(case.terms)
    got_routes = set()
    for k, e in enumerate(exp):
        plan, st = e["plan"], e["state"]
        print(case.name, "term", k, "F", st["F"], "D1", st["D1"], "V", st["V"], "F*maxV", st["product"], "j0", st["j0"], plan)
        assert sum(plan[r] for r in bp.ROUTES) == st["D1"], (case.name, k, plan)
        got_routes |= {r for r in bp.ROUTES if plan[r]}
        # V of every frame is the oracle's
        for f, spec in enumerate(case.frame_specs):
            if spec:
                assert st["V"][f] == bp.oracle_lattice_sizes(po, case, f)[k], (case.name, k, f)
            else:
                assert st["V"][f] == 0
    assert got_routes == case.routes, (case.name, got_routes, case.routes)
    e, st, plan = exp[0], exp[0]["state"], exp[0]["plan"]
    bound = bp.constants()["kPairFuseMaxVertices"]
    checks = {
        "above": st["F"] > 1 and st["product"] > bound and not (plan["paired_table"] or plan["paired_plain"]),
        "below": st["F"] > 1 and bound * 0.98 < st["product"] <= bound and plan["paired_plain"] > 0,
        "ragged": None in case.frames() and any(fr and fr["N"] % 4 for fr in case.frames()) and len({fr["N"] for fr in case.frames() if fr}) > 1,
        "table_not_filled": st["nbr2"] and not st["streaming"] and not st["table"],
        "compact_not_valid": st["nbrc"] and not st["compact"] and not case.env,
        "abandoned": st["nbrc"] and st["sorted_build"] and not st["compact"],
        "nontemporal": plan["nontemporal"] == 1,
        "j0=1": st["j0"] == 1, "j0=2": st["j0"] == 2, "j0=3": st["j0"] == 3,
        "table_from_1": st["first"] == 1 and plan["first_table_pair"] == 0,
        "first_pair_1": st["first"] == 1 and plan["first_table_pair"] == 1,
        "demoted": st["j0"] == 1 and st["D1"] > bp.constants()["demote_above_D1"] and st["F"] == 1
                   and bp.sp.plan_of(e["lattices"], case.max_points, 2)["passes"] == 2,
        "no_launch": plan["in_splat"] + plan["in_slice"] == st["D1"],
        "all_in_splat": plan["in_splat"] == st["D1"],
        "table_never_used": st["table"] and st["first"] == 1 and st["j0"] == 0 and plan["paired_table"] == 0,
        "slice_of_singles": st["F"] == 1 and plan["alone_32bit"] > 0 and plan["in_slice"] == 1,
        "single_in_pair_mode": st["D1"] == 2 and st["j0"] == 1 and plan["alone_32bit"] == 1 and st["product"] <= bound,
    }
    for name in case.classes:
        assert checks[name], (case.name, name, st, plan)
    for e2 in exp:                                      # the side of the vertex bound: above it only where the case says so
        assert (e2["state"]["product"] > bound) == ("above" in case.classes), (case.name, e2["state"]["product"])
    if "above" in case.classes or "below" in case.classes:
        # two distinct frames, repeated: different N, one odd and one even V
        specs = sorted(set(case.frame_specs))
        assert len(specs) == 2 and specs[0][0] != specs[1][0]
        assert {v & 1 for v in st["V"]} == {0, 1}, (case.name, st["V"])
    if plan["alone_compact"]:
        # k_blur2c's tail branch (the last vertex of an odd V) on a pass that runs alone: its SECOND neighbour is present there, and
        # is rebuilt from the block's second base, which differs from the first
        lat = next(l for l in e["lattices"] if l.V & 1)
        v, B = lat.V - 1, bp.constants()["kNbrcBlock"]
        blk = slice(v // B * B, lat.V)
        seen = False
        for j in range(st["j0"], st["D1"]):
            n2 = lat.nbr[j]
            n1 = np.full(lat.V, -1, np.int64)
            n1[n2[n2 >= 0]] = np.nonzero(n2 >= 0)[0]
            b1, b2 = n1[blk][n1[blk] >= 0], n2[blk][n2[blk] >= 0]
            seen |= bool(n2[v] >= 0 and (b1.min() if len(b1) else 0) != b2.min())        # (a block without an n1: base 0)
        assert seen, case.name


def test_table_reaches_every_route_with_the_release_library():
    release = [c for c in bp.CASES if not c.env]
    for route in bp.RELEASE_ROUTES:
        assert any(c.expected()[k]["plan"][route] for c in release for k in range(len(c.terms))), route
    # both instantiations of the pass on 32-bit ids, and the classes the issue names
    assert any(c.plan()["alone_32bit"] and c.plan()["nontemporal"] for c in release) and any(c.plan()["alone_32bit"] and not c.plan()["nontemporal"] for c in release)
    have = set().union(*(c.classes for c in bp.CASES))
    assert have >= {"above", "below", "ragged", "table_not_filled", "compact_not_valid", "abandoned", "nontemporal", "j0=1", "j0=2", "j0=3", "table_from_1",
                    "first_pair_1", "demoted", "no_launch", "all_in_splat", "table_never_used", "slice_of_singles", "single_in_pair_mode"}
    # d + 1 = 2 .. 9 on the two-hop table from pass 0, pairs only and pairs + the slice
    hash1 = {c.expected()[0]["state"]["D1"]: c.plan() for c in release if c.name.startswith("hash1_D")}
    assert sorted(hash1) == list(range(2, 10))
    for D1, p in hash1.items():
        assert p["paired_table"] == D1 - D1 % 2 and p["in_slice"] == D1 % 2 and p["first_table_pair"] == 0, (D1, p)
    # the same batch above the bound with and without the compact table; the same F either side of the bound
    above, below = bp.BY_NAME["big_F3_sorted"], bp.BY_NAME["below_F3_sorted"]
    assert above.F == below.F and above.plan()["alone_compact"] and below.plan()["paired_plain"]
    for name in ("span_F3_sorted", "nocompact_F3_sorted"):
        assert bp.BY_NAME[name].frame_specs == above.frame_specs and bp.BY_NAME[name].plan()["alone_32bit"] == above.plan()["alone_compact"]

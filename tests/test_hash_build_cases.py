"""The cases of tests/test_hash_build.py without a GPU (tests/hash_build_cases.py, notes/hash_build_tests.md): the restated hashes and
capacity rules against the sources, every case against the claim in its name -- from the linear-probing model alone --, and the
planted faults: each changes the lattice of the cases built for it.  On the suite's ordinary frames (wl.slam_problem(2000, seed))
a probe that does not wrap and a reserved key that is "found" change NOTHING: no chain there runs over the end of a table and no
vertex there has the reserved key for a neighbour, so only the constructed cases can tell.  (The other two planted faults -- a
lookup that gives up at the first foreign key, an id read at the home slot -- the ordinary frames do catch: a table 1/7 full
already displaces a few dozen keys by a slot or two.  The model says so, and this file asserts what the model says.)
"""
import numpy as np
import pytest

import hash_build_cases as hb

M32 = 0xffffffff


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_restated_constants_equal_the_sources():
    assert hb.constants() == hb.RESTATED
    assert hb.hcap_steps() == [(340, 344, 1024, 2048), (680, 684, 2048, 4096), (1364, 1368, 4096, 8192)]
    assert [hb.frame_hcap(n) for n in (1, 340, 341, 344, 680, 681, 1364, 1365, 2730, 2731, 4096)] == \
        [1024, 1024, 2048, 2048, 2048, 4096, 4096, 8192, 8192, 8192, 8192]
    assert [hb.small_hcap(n, 2) for n in (1, 224, 225, 228, 452, 456)] == [1024, 1024, 2048, 2048, 2048, 4096]
    assert hb.small_hcap(340, 1) == 1024 and hb.small_hcap(344, 1) == 2048 and hb.small_hcap(168, 3) == 1024 and hb.small_hcap(172, 3) == 2048
    assert hb.stream_cap(600, 5) == 8192 and hb.stream_cap(400, 8) == 8192 and hb.stream_cap(4100, 2) == 32768 and hb.stream_cap(1, 1) == 16
    assert hb.small_supported(4096, 2) and not hb.small_supported(4097, 2) and not hb.small_supported(100, 4)


def _hash32_scalar(x, y):
    h = ((x & 0xffff) | ((y & 0xffff) << 16)) * 2654435761 & M32
    h ^= h >> 15
    h = h * 2246822519 & M32
    return h ^ (h >> 13)


def _hash_key_scalar(key):
    h = 0
    for c in key:
        h = (h + (c & M32)) & M32                        # (unsigned)(int)key[i]: sign-extended
        h = h * 1664525 & M32
    h ^= h >> 15
    h = h * 2246822519 & M32
    return h ^ (h >> 13)


def test_vector_hashes_equal_plain_integer_arithmetic():
    rng = np.random.default_rng(1)
    for d in (1, 2, 3, 5, 8):
        keys = rng.integers(-32768, 32768, (200, d)).astype(np.int16)
        keys[0], keys[1] = -32768, 32767
        assert [int(h) for h in hb.hash_key(keys)] == [_hash_key_scalar([int(c) for c in k]) for k in keys]
    keys = rng.integers(-32768, 32768, (200, 2)).astype(np.int16)
    keys[0] = -32768
    assert int(hb.pack2(keys)[0]) == hb.EMPTY_KEY
    assert [int(h) for h in hb.hash32(hb.pack2(keys))] == [_hash32_scalar(int(x), int(y)) for x, y in keys]
    assert np.array_equal(hb.unpack2(hb.pack2(keys)), keys)


def test_neighbour_keys_wrap_like_the_references_shorts():
    n2 = hb.n2_keys(np.array([[32767, 32767], [0, 0], [-32768, 5]], np.int16))
    assert n2.shape == (3, 3, 2)
    assert n2[:, 0].tolist() == [[32765, -32768], [-32768, 32765], [-32768, -32768]]     # axis 2 of (32767, 32767): the reserved key
    assert n2[:, 1].tolist() == [[-2, 1], [1, -2], [1, 1]]
    assert n2[0, 2].tolist() == [32766, 6]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_on_a_table_small_enough_to_do_by_hand():
    keys = np.array([[0], [2], [4], [6], [8]], np.int16)
    home = np.array([6, 7, 7, 6, 1])
    t = hb.Table(keys, home, 8, hb.hash_key)
    assert t.slot.tolist() == [6, 7, 0, 1, 2] and t.owner.tolist() == [2, 3, 4, -1, -1, -1, 0, 1]
    assert t.past_wrap() == 3 and t.displaced_across_wrap() == 2 and t.longest_chain() == 4
    assert t.to_empty.tolist() == [3, 2, 1, 0, 0, 0, 5, 4]
    nw = hb.Table(keys, home, 8, hb.hash_key, wrap=False)
    assert nw.slot.tolist() == [6, 7, -1, -1, 1] and nw.dropped == 2
    # the occupied slots, and with them the path of every lookup of an absent key, do not depend on the insertion order
    rng = np.random.default_rng(3)
    keys = rng.integers(-99, 99, (300, 3)).astype(np.int16)
    keys = keys[np.unique(keys, axis=0, return_index=True)[1]]
    home = np.minimum(rng.integers(0, 512, keys.shape[0]), rng.integers(300, 520, keys.shape[0])) % 512
    a = hb.Table(keys, home, 512, hb.hash_key)
    p = rng.permutation(keys.shape[0])
    b = hb.Table(keys[p], home[p], 512, hb.hash_key)
    assert np.array_equal(a.occupied, b.occupied) and np.array_equal(a.to_empty, b.to_empty) and a.past_wrap() == b.past_wrap()


# ---- the frame body's cases ---------------------------------------------------------------------------------------------------------------
def _window(name):
    if name.startswith("hcap_step_"):
        return hb.STEP_WINDOW * max(hb.frame_hcap(int(name.rsplit("_", 1)[1])) // 4096, 1)
    return hb.WINDOWS[name][1]


@pytest.mark.parametrize("name", hb.FITTING)
def test_a_windowed_case_is_what_its_name_claims(po, name):
    f, ref, tb = hb.frame_case(po, name)
    N, W = f.shape[0], _window(name)
    s = tb.summary()
    print(name, N, s)
    assert tb.cap == hb.frame_hcap(N) and s["dropped"] == 0 and s["reserved_queries"] == 0
    # every point has a vertex that homes in the window, by the finished frame's own lattice
    inwin = tb.home >= tb.cap - W
    assert inwin[ref["offset"][:N]].any(1).all()
    assert s["past_wrap"] >= W and s["displaced_across_wrap"] >= W and s["longest_lookup"] >= s["past_wrap"]
    assert s["absent_over_wrap"] >= 1 and s["found_over_wrap"] >= W
    rows = np.bincount(ref["offset"][:N].ravel(), minlength=ref["V"])
    if name.startswith("wrap_"):
        assert tb.cap == int(name.rsplit("_", 1)[1])
    if name.startswith("nearly_full_"):
        assert tb.cap == int(name.rsplit("_", 1)[1]) and s["load"] >= 0.99
    if name.startswith("hcap_step_"):
        below, above, cap_below, cap_above = next(st for st in hb.hcap_steps() if N in st[:2])
        assert N % 4 == 0 and tb.cap == (cap_below if N == below else cap_above)
        assert 3 * N <= tb.cap if N == below else 3 * N > tb.cap // 2                # the last count of the smaller table, the first of the larger
    if name == "shared_cells":
        assert N % 4 and rows.min() == 0 and rows.max() == 3 and ref["V"] == 3 * (N // 3) + 3      # three points per cell, a phantom point's cell
    # the kernel keeps the frame, in every launch form the tests use (the loop's plan and the build's scratch beside the table)
    other = [hb.lattice(po, hb.frame_problem(po, name, 0)["kernels"][1][0]), hb.lattice(po, hb.frame_problem(po, name, 1)["kernels"][0][0])]
    row = lambda r: int(np.bincount(r["offset"][:N].ravel(), minlength=r["V"]).max())
    assert hb.frame_plan_fits(N, [ref["V"]], row(ref), tb.cap)
    for dual in (False, True):
        assert hb.frame_plan_fits(N, [ref["V"], other[0]["V"]], row(ref), tb.cap, dual=dual), (name, dual)
        assert hb.frame_plan_fits(N, [other[1]["V"], ref["V"]], row(other[1]), tb.cap, dual=dual), (name, dual)


def test_overfull_has_more_keys_than_the_largest_table_has_slots(po):
    f, ref, tb = hb.frame_case(po, "overfull_8192")
    assert f.shape[0] == 4096 and tb.cap == 8192 == hb.FRAME_HCAP[2] and ref["V"] == 3 * 4096 > tb.cap
    assert tb.dropped == ref["V"] - tb.cap and tb.load == 1.0 and not hb.frame_plan_fits(4096, [ref["V"]], 1, tb.cap)


def test_the_reserved_key_is_a_vertex_of_one_case_and_only_a_query_of_the_other(po):
    reserved = np.array([-32768, -32768], np.int16)
    fv, refv, tbv = hb.frame_case(po, "reserved_vertex")
    fn, refn, tbn = hb.frame_case(po, "reserved_neighbour")
    assert (refv["keys"] == reserved).all(1).sum() == 1 and int((hb.pack2(refv["keys"]) == hb.EMPTY_KEY).sum()) == 1
    assert not (refn["keys"] == reserved).all(1).any()
    lk = tbn.lookups()
    assert lk["reserved"].sum() == 1 and lk["id"][lk["reserved"]].tolist() == [hb.ABSENT] and lk["ends_empty"][lk["reserved"]].all()
    j, v = np.argwhere(lk["reserved"])[0]
    assert j == 2 and refn["keys"][v].tolist() == [32767, 32767]
    # the simplex the issue names, and the reference's own answer for the query: nothing there
    p = refn["offset"][150]
    assert sorted(map(tuple, refn["keys"][p].tolist())) == sorted([(32766, 32766), (32767, 32767), (-32768, 32765)])
    assert refn["nbr"][2, v, 1] == -1
    assert fv.shape == fn.shape == (300, 2) and (fv[:150] == fn[:150]).all() and (fv[151:] == fn[151:]).all()


# ---- the entry-id tables' cases -------------------------------------------------------------------------------------------------------------
def test_small_build_cases_are_what_their_names_claim(po):
    seen = set()
    for name, d, frames in hb.small_cases(po):
        NA = max(f.shape[0] for f in frames)
        assert hb.small_supported(NA, d) and hb.small_hcap(NA, d) == 1024 and hb.small_hcap(hb.SMALL_N[d] + 4, d) == 2048
        tabs = [hb.small_table(hb.lattice(po, f)["keys"], NA) for f in frames]
        s = tabs[0].summary()
        print(name, [f.shape[0] for f in frames], s)
        assert s["past_wrap"] >= 8 and s["displaced_across_wrap"] >= 8 and s["absent_over_wrap"] >= 1 and s["found_over_wrap"] >= 8, name
        if "two_thirds" in name:
            assert NA == hb.SMALL_N[d] and s["load"] >= 0.65, (name, s)
        if "wrap" in name:                               # the second frame: its keys home in the FIRST slots of its own table
            assert (tabs[1].home < 8).sum() >= frames[1].shape[0] // (d + 1) and frames[1].shape[0] % 4
        if "shared" in name:
            ref = hb.lattice(po, frames[0])
            assert np.bincount(ref["offset"].ravel()).max() == 3 and ref["V"] <= frames[0].shape[0] + 6
        seen.add(d)
    assert seen == {1, 2, 3}


def test_streaming_cases_are_what_their_names_claim(po):
    seen = set()
    for name, d, max_points, frames in hb.stream_cases(po):
        assert not hb.small_supported(max_points, d) and max_points < 8192 and max(f.shape[0] for f in frames) == max_points
        cap = hb.stream_cap(max_points, d)
        tabs = [hb.stream_table(hb.lattice(po, f)["keys"], max_points) for f in frames]
        s = [t.summary() for t in tabs]
        print(name, [f.shape[0] for f in frames], s)
        assert all(t.cap == cap for t in tabs)
        # frame 0 runs over the end of its table -- where frame 1's table begins; frame 1's keys home in the first slots of its own
        assert s[0]["past_wrap"] >= 16 and s[0]["absent_over_wrap"] >= 1 and s[0]["found_over_wrap"] >= 16, name
        assert (tabs[1].home < 64).sum() >= 150 and s[1]["longest_lookup"] >= 150 and s[1]["displaced_across_wrap"] == 0, name
        assert frames[2].shape[0] % 4 and frames[2].shape[0] < frames[1].shape[0] < frames[0].shape[0]
        seen.add(d)
    assert seen == {2, 5, 8}


# ---- the planted faults ---------------------------------------------------------------------------------------------------------------------
def _changes(tb, fault):
    """(V changed, neighbour entries changed) by a planted fault"""
    v0, n0 = tb.neighbours()
    v1, n1 = tb.neighbours(fault)
    return v0 != v1, int((n0 != n1).sum())


@pytest.mark.parametrize("name", hb.FITTING)
def test_every_probing_fault_changes_a_windowed_case(po, name):
    tb = hb.frame_case(po, name)[2]
    W = _window(name)
    got = {f: _changes(tb, f) for f in hb.FAULTS}
    print(name, got)
    assert got["no_wrap"][0] and got["no_wrap"][1] >= W                  # vertices are lost off the end of the table, and neighbours with them
    assert got["stop_at_first_foreign_key"][1] >= W and got["id_from_home_slot"][1] >= W
    assert got["reserved_key_found"] == (False, 0)                       # (no query for the reserved key here)


def test_the_reserved_fault_changes_reserved_neighbour_alone(po):
    got = {name: _changes(hb.frame_case(po, name)[2], "reserved_key_found") for name in hb.FRAME_CASES}
    assert {n for n, g in got.items() if g != (False, 0)} == {"reserved_neighbour"} and got["reserved_neighbour"] == (False, 1)
    v, n2 = hb.frame_case(po, "reserved_neighbour")[2].neighbours("reserved_key_found")
    assert (n2 == hb.GARBAGE).sum() == 1


def test_every_probing_fault_changes_the_entry_id_tables_cases(po):
    tabs = [(name, hb.small_table(hb.lattice(po, fr[0])["keys"], max(f.shape[0] for f in fr))) for name, d, fr in hb.small_cases(po)]
    tabs += [(name, hb.stream_table(hb.lattice(po, fr[0])["keys"], mp)) for name, d, mp, fr in hb.stream_cases(po)]
    for name, tb in tabs:
        got = {f: _changes(tb, f) for f in hb.FAULTS}
        print(name, got)
        assert got["no_wrap"][0] and got["stop_at_first_foreign_key"][1] >= 8 and got["id_from_home_slot"][1] >= 8, name
        assert got["reserved_key_found"] == (False, 0), name             # (no key is reserved in a table of entry ids)


def test_what_the_suites_ordinary_frames_can_and_cannot_tell(po, wl):
    """Three frames of the kind every other test of the builds uses.  No key is displaced across the wrap, no lookup crosses it, no
    query is the reserved key: a probe without the mask and a `found` reserved key change NOTHING there -- those faults pass every
    test but the constructed ones.  A table 1 / 7 full still displaces keys (about V^2 / 2 cap of them: 80 at V = 1160 and 8192
    slots), so the two faults that mishandle a displaced key do show on these frames, in the smoothness term's lattice."""
    for seed in (1, 2, 3):
        pb = wl.slam_problem(2000, seed=seed)
        for k in range(2):
            keys = hb.lattice(po, pb["kernels"][k][0])["keys"]
            for tb in (hb.frame_table(keys, 2000), hb.small_table(keys, 2000)):
                s = tb.summary()
                got = {f: _changes(tb, f) for f in hb.FAULTS}
                print(seed, k, s, got)
                assert s["displaced_across_wrap"] == 0 and s["absent_over_wrap"] == 0 and s["found_over_wrap"] == 0 and s["reserved_queries"] == 0
                assert s["longest_lookup"] <= 8 and s["load"] < 0.15
                assert got["no_wrap"] == (False, 0) and got["reserved_key_found"] == (False, 0)
                if k == 1:
                    assert 0 < got["stop_at_first_foreign_key"][1] < tb.V and 0 < got["id_from_home_slot"][1] < tb.V

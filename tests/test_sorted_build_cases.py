"""tests/sorted_build_cases.py without a GPU: every case sits where it claims -- shown with the numpy restatement of the build's rules and
the oracle's own lattice of the finished frames -- and the oracle alone handles every case.  On the device the library's report must
equal the same restatement and satisfy the same claim (tests/test_sorted_build.py); notes/sorted_build_tests.md has the table."""
import numpy as np
import pytest

import sorted_build_cases as sb
import sorted_build_checker as sc

NAMES = [c.name for c in sb.CASES]


def vcap(c):
    return ((sb.features(c)[1] + 3) & ~3) * (c.d + 1)


def ref_of(po, name, frame=0):
    return sb.oracle(po, sb.BY_NAME[name])[frame][0]


@pytest.mark.parametrize("name", NAMES)
def test_case_sits_where_it_claims(po, name):
    c = sb.BY_NAME[name]
    fs, max_points = sb.features(c)
    # the smallest frames the release threshold admits (locality mode is decided by the batch's largest frame), but for the one case
    # whose size the bitmap's 507 904 ids force
    assert sb.PERM_MIN <= max(f.shape[0] for f in fs) <= max_points <= (12000 if name != "wide_id_span" else 57000)
    assert all(sb.int16_guard_holds(f) for f in fs)                      # (and vertex_plan asserts the 62-bit box): no fallback to the hash
    for sorted_build, claim in ((True, c.claim), (False, c.hash_claim)):
        rs = sb.expected(po, c, sorted_build)
        assert claim is None or claim(rs), (name, c.branch, rs)
        for r in rs:
            assert r["long_buckets"] == sum(r[k] for k in sb.FIELDS[3:7]) and (r["sorted_build"] or not any(r[k] for k in sb.FIELDS[:10]))
    for ref, q, m, f, u in sb.oracle(po, c):                              # the oracle alone handles the case
        assert q.shape == (f.shape[0], 2) and np.all(np.isfinite(q)) and m.shape == (f.shape[0],)


def test_neighbouring_cases_differ_by_one_entry_or_point(po):
    top = lambda name: int(sb.bucket_entries(ref_of(po, name), vcap(sb.BY_NAME[name]))[0])
    assert [top(n) for n in ("uniform_512", "uniform_513", "uniform_1023", "uniform_1024")] == [512, 513, 1023, 1024]
    for a, b in (("uniform_512", "uniform_513"), ("uniform_1023", "uniform_1024")):         # ... and every other bucket stays short
        for n in (a, b):
            assert sb.bucket_entries(ref_of(po, n), vcap(sb.BY_NAME[n]))[3] <= sb.LONG_BUCKET
    pb = lambda name, rm: int(np.bincount(sb.point_buckets(sb.features(sb.BY_NAME[name])[0][0], sb.PERM_MIN, rm)[0]).max())
    assert [pb("point_bucket_64", True), pb("point_bucket_65", True)] == [64, 65]
    assert [pb("point_bucket_64", False), pb("point_bucket_65", False)] == [64, 65]
    rows = lambda name: np.sort(np.bincount(ref_of(po, name)["offset"][:ref_of(po, name)["N"]].reshape(-1)))[::-1]
    assert rows("rows_128")[0] == 128 and list(rows("rows_129_and_777")[:7]) == [777] * 3 + [129] * 3 + [rows("rows_129_and_777")[6]]
    assert rows("rows_129_and_777")[6] <= sb.LONG_ROW


def test_bitmap_cases_sit_on_either_side_of_a_word_per_lane(po):
    assert all(w <= 256 for w in sb.bitmap_words(ref_of(po, "uniform_1024"))) and len(sb.bitmap_words(ref_of(po, "uniform_1024"))) == 3
    assert all(256 < w <= sb.BITMAP_WORDS for w in sb.bitmap_words(ref_of(po, "bitmap_over_256_words")))
    wide = sb.bitmap_words(ref_of(po, "wide_id_span"))
    assert any(w > sb.BITMAP_WORDS for w in wide) and any(w <= sb.BITMAP_WORDS for w in wide)
    f = sb.features(sb.BY_NAME["wide_id_span"])[0][0]
    assert np.array_equal(f[0], f[-1]) and int((f == f[0]).all(1).sum()) >= 1024         # the first and the last point among the identical ones


def test_phantom_cases(po):
    assert sb.first_vertex_is_phantoms_alone(ref_of(po, "phantoms_first"))
    assert sb.first_vertex_is_phantoms_alone(ref_of(po, "phantoms_last"), last=True)
    assert not sb.first_vertex_is_phantoms_alone(ref_of(po, "phantoms_mod1_alone"))
    assert not sb.first_vertex_is_phantoms_alone(ref_of(po, "phantoms_mod1_alone"), last=True)
    ref = ref_of(po, "phantoms_in_bitmap")                                 # the giant origin vertex: the phantom points' entries end its runs
    N = ref["N"]
    assert np.array_equal(ref["offset"][N:], np.repeat(ref["offset"][N:N + 1], 3, 0))
    assert all(int((ref["offset"][:N] == v).sum()) >= 1024 for v in ref["offset"][N])
    for m in (1, 2, 3, 0):
        assert ref_of(po, "phantoms_mod%d_alone" % m)["N"] % 4 == m == ref_of(po, "phantoms_mod%d_at_origin" % m)["N"] % 4


def test_box_cases_share_their_size_and_the_mixed_bucket_holds_several_codes(po):
    assert ref_of(po, "box_narrow")["N"] == ref_of(po, "box_wide")["N"]
    c = sb.BY_NAME["mixed_long_bucket"]
    ref = ref_of(po, c.name)
    bucket = sb.vertex_plan(ref, vcap(c))[1]
    big = np.flatnonzero(np.bincount(bucket[ref["offset"].reshape(-1)]) > sb.LONG_BUCKET)
    assert big.size >= 1 and all(int((bucket == b).sum()) > 1 for b in big)


def test_scan_tile_arithmetic():
    """n = Epad + 1 with Epad a multiple of four: of 4096 k and 4096 k +- 1 only 4096 k + 1 can be reached; the other side is 4096 k - 3"""
    assert all((4 * m * (d + 1) + 1) % 4 == 1 for m in range(1, 50) for d in range(1, 9))
    assert (sb.PERM_MIN * 3 + 1) % sb.SCAN_TILE == 1 and (9556 * 3 + 1) % sb.SCAN_TILE == sb.SCAN_TILE - 3 and 9556 % 4 == 0


@pytest.mark.parametrize("name", ["ragged", "phantoms_first", "rows_129_and_777"])
def test_checker_accepts_the_oracles_tables_of_a_case(po, name):
    """the checker and the case table meet: every frame of these cases, an empty one and a one-point one included, in the sorted
    build's numbering and a shuffled point order"""
    rng = np.random.default_rng(3)
    for ref, _, _, _, _ in sb.oracle(po, sb.BY_NAME[name]):
        t = sc.tables_from_reference(ref, sc.row_major_order(ref), rng.permutation(ref["N"]))
        sc.check(ref, t, sorted_build=True)

"""Tracking::BfMatch (src/Tracking.cc:1747-1766): brute-force Hamming 2-NN
with the 0.6 ratio test.  PARITY UNPINNED against OpenCV (absent here): the oracle restates
cv::BFMatcher::knnMatch's published behaviour; the HIP path must equal the oracle exactly."""
import importlib

import numpy as np
import pytest

import next_row_cases as nr

pkg = importlib.import_module("lc-crf-slam_amd")


def descriptors(n_query, n_train, seed, planted=0.4, flips=(0, 40)):
    """Random 256-bit descriptors; a share of the queries gets a noisy copy in the train set (and
    some of those a second, worse copy), so that the ratio test sees accepts, rejects and ties."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (n_query, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (n_train, 32), dtype=np.uint8)
    if n_train and n_query:
        for i in rng.choice(n_query, int(planted * n_query), replace=False):
            j = int(rng.integers(0, n_train))
            bits = rng.choice(256, int(rng.integers(flips[0], flips[1] + 1)), replace=False)
            d = q[i].copy()
            for b in bits:
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            t[j] = d
            if rng.random() < 0.3:                         # an exact duplicate elsewhere: a tie on the best distance
                t[int(rng.integers(0, n_train))] = d
    return q, t


def test_oracle_bf_match_known_answers(po):
    z = np.zeros((1, 32), np.uint8)
    one = z.copy(); one[0, 0] = 0x01                       # distance 1 from z
    far = np.full((1, 32), 0xff, np.uint8)                 # distance 256 from z
    # best 0, second 256: 0 < 256 * 0.6 -> match with the FIRST of the train rows
    out, n = po.oracle_bf_match(z, np.concatenate([far, z, far]))
    assert out.tolist() == [1] and n == 1
    # two exact copies: 0 < 0 * 0.6 is false -> no match (and the tie would keep the lower index)
    out, n = po.oracle_bf_match(z, np.concatenate([z, z, far]))
    assert out.tolist() == [-1] and n == 0
    # ratio boundary: d0 = 3, d1 = 5: 5 * 0.6 rounds to exactly 3.0 in double, and 3 < 3.0 is false
    three = z.copy(); three[0, 0] = 0x07
    five = z.copy(); five[0, 0] = 0x1f
    two = z.copy(); two[0, 0] = 0x03
    out, _ = po.oracle_bf_match(z, np.concatenate([five, three]))
    assert out.tolist() == [-1]
    out, _ = po.oracle_bf_match(z, np.concatenate([five, two]))
    assert out.tolist() == [1]
    out, _ = po.oracle_bf_match(z, np.concatenate([five, two]), ratio=0.4)
    assert out.tolist() == [-1]
    # fewer than two train descriptors: knnMatch returns < 2 neighbours, the reference skips the query
    assert po.oracle_bf_match(z, one)[0].tolist() == [-1]
    assert po.oracle_bf_match(z, np.zeros((0, 32), np.uint8))[0].tolist() == [-1]
    assert po.oracle_bf_match(np.zeros((0, 32), np.uint8), z)[1] == 0


def test_bf_match_argument_checks():
    lib = pkg.lib()
    assert lib.lccrf_bf_match(0, -1, None, 0, None, 0.6, None, None) == -1
    assert lib.lccrf_bf_match(0, 4, None, 4, None, 0.6, None, None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("n_query,n_train,seed", [(2000, 2000, 1), (1, 2, 2), (0, 5, 3), (7, 1, 4), (5, 0, 5),
                                                  (1500, 1023, 6), (333, 1025, 7), (64, 3000, 8), (65, 4096, 9)])
def test_hip_bf_match_equals_oracle(po, n_query, n_train, seed):
    q, t = descriptors(n_query, n_train, seed)
    for ratio in (0.6, 0.95):
        o, no = po.oracle_bf_match(q, t, ratio)
        h, nh = pkg.bf_match(q, t, ratio)
        assert np.array_equal(o, h) and no == nh
    if n_query >= 1500:
        assert 0.2 * n_query < no < 0.6 * n_query           # the planted pairs are found, random pairs are not


@pytest.mark.gpu
def test_hip_bf_match_ties_keep_the_lower_train_index(po):
    q, t = descriptors(400, 900, seed=11, planted=0.0)
    t[500] = t[17]                                         # exact duplicates in the train set
    t[300] = q[5]; t[800] = q[5]                           # and two perfect copies of a query: d0 = d1 = 0 -> rejected
    q[9] = t[17]                                           # query 9: d0 = d1 = 0 as well
    far = q[3].copy(); far[:12] ^= 0xff                    # query 3: a lone near copy at two places, 96 bits away ...
    t[40] = far; t[41] = far                               # ... a tie at the best distance, accepted only at ratio ~1
    o, no = po.oracle_bf_match(q, t, 1.01)
    h, nh = pkg.bf_match(q, t, 1.01)
    assert np.array_equal(o, h) and no == nh
    assert h[3] == 40                                      # a tie at the best distance: the lower train index wins
    assert h[5] == -1 and h[9] == -1                       # d0 = d1 = 0: 0 < 0 * ratio never holds


# ---------------------------------------------------------------------------------------------------------------------------
# sizes, boundaries and ties of tests/next_row_cases.py; the oracle and the numpy reference are held to each other on the CPU
# (test_next_row_cases.py)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_train", nr.BF_TRAIN)
def test_hip_bf_match_small_and_tile_sizes(po, n_train):
    """fewer train rows than the 16 lanes of a query, and the tile of 1024 rows from either side, at query counts around a block's 16"""
    for n_query in nr.BF_QUERY:
        q, t = nr.planted(n_query, n_train, seed=n_train)
        for ratio in (0.6, 1.01):
            h, nh = pkg.bf_match(q, t, ratio)
            o, no = po.oracle_bf_match(q, t, ratio)
            assert np.array_equal(h, o) and nh == no, (n_query, ratio)
            r, nn = nr.bf_match_np(q, t, ratio)
            assert np.array_equal(h, r) and nh == nn, (n_query, ratio)


@pytest.mark.gpu
def test_hip_bf_match_ratio_boundary_pairs(po):
    """every (d0, d1) within 1 of d0 = 0.6 d1, in both row orders, as two-row calls"""
    z = np.zeros((1, 32), np.uint8)
    for d0, d1 in nr.boundary_pairs():
        want = d0 < d1 * 0.6
        for order in ((d0, d1), (d1, d0)):
            t = np.stack([nr.prefix_row(order[0]), nr.prefix_row(order[1])])
            first = 0 if d0 == d1 else order.index(d0)
            h, nh = pkg.bf_match(z, t)
            assert h.tolist() == [first if want else -1] and nh == int(want), (d0, d1, order)
            assert h.tolist() == po.oracle_bf_match(z, t)[0].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", nr.BF_RATIOS)
def test_hip_bf_match_ratios(po, ratio):
    for n_query, n_train in ((33, 17), (17, 1025), (200, 300)):
        q, t = nr.planted(n_query, n_train, seed=3)
        t[n_train // 2] = q[0]; t[n_train // 3] = q[0]             # d0 = d1 = 0: inf * 0 is NaN, never a match
        h, nh = pkg.bf_match(q, t, ratio)
        o, no = po.oracle_bf_match(q, t, ratio)
        r, nn = nr.bf_match_np(q, t, ratio)
        assert np.array_equal(h, o) and np.array_equal(h, r) and nh == no == nn
        assert h[0] == -1
        if ratio == 0:
            assert nh == 0
        if ratio == np.inf:
            assert nh >= 0.9 * n_query                             # all but the queries with two exact copies


@pytest.mark.gpu
def test_hip_bf_match_distance_256(po):
    """the top of the 9-bit distance field: a zero query against rows of 0xff"""
    z = np.zeros((3, 32), np.uint8)
    for n_train in (2, 40, 1030):
        t = np.full((n_train, 32), 0xff, np.uint8)
        h, nh = pkg.bf_match(z, t, 0.6)
        assert h.tolist() == [-1] * 3 and nh == 0                  # 256 < 256 * 0.6 is false
        h, nh = pkg.bf_match(z, t, 1.01)
        assert h.tolist() == [0] * 3 and nh == 3                   # equal distances: the lowest index, accepted above ratio 1
        t[n_train - 1] = 0                                         # one exact copy
        for ratio in (0.6, 1.01):
            h, nh = pkg.bf_match(z, t, ratio)
            assert h.tolist() == [n_train - 1] * 3 and nh == 3
            assert h.tolist() == po.oracle_bf_match(z, t, ratio)[0].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,n_train", [((3, 19), 64), ((7, 23), 2100), ((1023, 1024), 1500), ((5, 2053), 2100), ((1024 + 9, 2048 + 9), 3000)])
def test_hip_bf_match_ties_in_a_lane_and_across_tiles(po, rows, n_train):
    """A tie at the best distance between rows t and t + 16 (one lane of a query), across the tile boundary, and two tiles apart:
    the lower train index wins."""
    q, t = nr.planted(20, n_train, seed=rows[1], share=0.0)
    near = q[4].copy(); near[:6] ^= 0xff                          # 48 bits away: far below any random row
    t[rows[0]] = near; t[rows[1]] = near
    h, nh = pkg.bf_match(q, t, 1.01)
    o, no = po.oracle_bf_match(q, t, 1.01)
    assert np.array_equal(h, o) and nh == no and h[4] == min(rows)
    assert pkg.bf_match(q, t, 0.6)[0][4] == -1                     # d0 = d1


@pytest.mark.gpu
def test_hip_bf_match_all_train_rows_equal(po):
    q, _ = nr.planted(40, 2, seed=5, share=0.0)
    t = np.tile(q[7], (1500, 1))
    h, nh = pkg.bf_match(q, t, 1.01)
    assert h.tolist() == [-1 if i == 7 else 0 for i in range(40)] and nh == 39   # query 7: 0 < 0 * 1.01 is false
    assert np.array_equal(h, po.oracle_bf_match(q, t, 1.01)[0]) and np.array_equal(h, nr.bf_match_np(q, t, 1.01)[0])


@pytest.mark.gpu
def test_hip_bf_match_at_the_train_index_cap(po):
    """n_train = 2^22 - 1, the most the 22-bit index of the key holds: near copies at rows whose indices use the top bits.  Random
    rows sit near distance 128 (never below 60 among 2^24 pairs), so a copy at distance 1 passes 0.6 against any of them."""
    rng = np.random.default_rng(2022)
    t = rng.integers(0, 256, (nr.BF_CAP, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    rows = [(1 << 22) - 2, 1 << 21, (1 << 21) - 1, (1 << 20) + 5]
    for i, r in enumerate(rows):
        t[r] = q[i]
        t[r, i] ^= 1
    try:
        h, nh = pkg.bf_match(q, t)
    finally:
        pkg.lib().lccrf_trim_cache()                               # 200 MB of pinned and of device memory otherwise stay
    assert h.tolist() == rows and nh == 4
    o, no = po.oracle_bf_match(q, t)
    assert o.tolist() == rows and no == 4


@pytest.mark.gpu
def test_hip_bf_match_without_a_count(po):
    """n_matches_out == NULL through the C-ABI: the indices are still right"""
    q, t = nr.planted(33, 1025, seed=9)
    out = np.full(33, -7, np.int32)
    lib = pkg.lib()
    rc = lib.lccrf_bf_match(0, 33, q.ctypes.data, 1025, t.ctypes.data, 0.6, out.ctypes.data_as(lib.lccrf_bf_match.argtypes[6]), None)
    assert rc == 0 and np.array_equal(out, po.oracle_bf_match(q, t)[0]) and (out >= 0).any()

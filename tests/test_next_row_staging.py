"""The staging areas of the unary builder and of BfMatch (csrc/unary_builder.hip, csrc/bf_match.hip): one pinned arena and one device
buffer each, kept between calls behind a mutex, grown when a call needs more, freed by lccrf_trim_cache.  A call after a larger one
must not see the larger one's results, two threads must not see each other's, and a call after a trim starts afresh."""
import importlib
import threading

import numpy as np
import pytest

import crf_cases as cc
import next_row_cases as nr

pkg = importlib.import_module("lc-crf-slam_amd")


def unary_case(po, wl, n_points, n_kf, seed, with_mp):
    s = wl.map_point_scene(n_points, n_kf, seed)
    mp = np.random.default_rng(seed).uniform(0, 1, n_points) if with_mp else None
    args = nr.scene_args(s)
    return args, mp, po.oracle_unary_build(*args, match_prob=mp)


def unary_equal(args, mp, want):
    got = pkg.unary_build(*args, match_prob=mp)
    return all(cc.same_bits(a, b) for a, b in zip(want[:3], got[:3])) and np.array_equal(want[3], got[3])


def bf_case(po, n_query, n_train, seed, ratio=0.6):
    q, t = nr.planted(n_query, n_train, seed)
    return q, t, ratio, po.oracle_bf_match(q, t, ratio)


def bf_equal(q, t, ratio, want):
    h, nh = pkg.bf_match(q, t, ratio)
    return np.array_equal(h, want[0]) and nh == want[1]


@pytest.mark.gpu
def test_hip_unary_build_arena_reuse(po, wl):
    """5000 points, then 3, 0, 700 with match probabilities, 700 without: in one process, in this order"""
    for n_points, n_kf, seed, with_mp in ((5000, 40, 5, False), (3, 2, 6, False), (0, 3, 7, False), (700, 9, 8, True), (700, 9, 8, False)):
        args, mp, want = unary_case(po, wl, n_points, n_kf, seed, with_mp)
        assert unary_equal(args, mp, want), n_points


@pytest.mark.gpu
def test_hip_bf_match_arena_reuse(po):
    """a small call after a large one must not read the large one's results out of the pinned arena"""
    for n_query, n_train in ((2000, 3000), (1, 2), (5, 0), (17, 1025)):
        assert bf_equal(*bf_case(po, n_query, n_train, seed=n_query)), (n_query, n_train)


@pytest.mark.gpu
def test_hip_next_row_after_trim_cache(po, wl):
    """lccrf_trim_cache frees both staging areas; the next call of each tool allocates afresh and is right, before and after growing"""
    u_small, u_large = unary_case(po, wl, 300, 6, 31, True), unary_case(po, wl, 3000, 20, 32, False)
    b_small, b_large = bf_case(po, 20, 40, 33), bf_case(po, 500, 1500, 34)
    lib = pkg.lib()
    assert unary_equal(*u_large) and bf_equal(*b_large)
    assert lib.lccrf_trim_cache() >= 0
    assert unary_equal(*u_small) and bf_equal(*b_small)           # fresh, small
    assert unary_equal(*u_large) and bf_equal(*b_large)           # grown again
    assert lib.lccrf_trim_cache() >= 0 and lib.lccrf_trim_cache() >= 0     # twice in a row: nothing left to free
    assert bf_equal(*b_small) and unary_equal(*u_small)


@pytest.mark.gpu
def test_hip_next_row_from_four_threads(po, wl):
    """Four threads, 20 calls each, both tools and mixed sizes (ctypes releases the GIL during a call): every result equals the
    oracle's, computed beforehand."""
    unary = [unary_case(po, wl, n, k, 40 + i, i % 2 == 0) for i, (n, k) in enumerate(((1200, 12), (3, 2), (257, 8), (0, 2), (600, 9), (40, 5)))]
    bf = [bf_case(po, nq, nt, 50 + i) for i, (nq, nt) in enumerate(((300, 1100), (1, 2), (17, 1025), (5, 0), (64, 33), (33, 2049)))]
    wrong, errors = [], []

    def work(tid):
        try:
            rng = np.random.default_rng(tid)
            for call in range(20):
                j = int(rng.integers(0, 6))
                ok = unary_equal(*unary[j]) if (call + tid) % 2 else bf_equal(*bf[j])
                if not ok:
                    wrong.append((tid, call, j))
        except Exception as e:                                    # a thread's exception would otherwise be lost
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(tid,)) for tid in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and not wrong, (errors, wrong)

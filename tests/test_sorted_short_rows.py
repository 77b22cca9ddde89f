"""Round 7 (csrc/fused_lean.h: sort_short_rows): the two-frames-per-CU inference kernel, run from prepared launch records, numbers
the vertices of every short-row kernel by descending row length, so that the 64 rows a wavefront sums in one round have nearly one
length.  A vertex's number is a label -- the results must not move by a bit: the self-contained kernel (build's numbering), the
inference that writes the records and runs from them, and the one that reuses them agree with each other and with the oracle."""
import numpy as np
import pytest

import crf_cases as cc

pytestmark = pytest.mark.gpu

F = 272                                                       # (at least 256 frames: the lean shape)
SETTINGS = ((5, 1.0), (3, 0.5))                               # (iterations, relax)


def three_inferences(b, n_iter, relax, tag):
    """self-contained, prepare + run, run: the same bits; returns them"""
    b.build()
    b.inference(n_iter, True, relax=relax)
    Q, M = b.probability(), b.map()
    runs0 = b.last_prepare()[1]
    for again in range(2):
        b.inference(n_iter, True, relax=relax)
        assert cc.same_bits(b.probability(), Q) and np.array_equal(b.map(), M), (tag, n_iter, "prepared", again)
    assert b.last_prepare()[1] == runs0 + 1, tag             # (the second inference wrote the records, the third reused them)
    return Q, M


def check_batch(po, base, maxN, tag, lean=True):
    pbs = [base[f % len(base)] for f in range(F)]
    for n_iter, relax in SETTINGS:
        b = cc.batch_of(pbs, maxN=maxN)
        Q, M = three_inferences(b, n_iter, relax, tag)
        assert b.engine() == 2, (tag, b.engine())
        if lean:
            assert b.fused_shape() == (512, 2), (tag, b.fused_shape())
        b.close()
        for i, pb in enumerate(base):
            o = cc.setup(po.OracleCRF, pb)
            o.inference_native(n_iter, True, relax)
            for f in range(i, F, len(base)):
                assert cc.same_bits(Q[f, :pb["N"]], o.probability()), (tag, n_iter, f, pb["N"])
                assert np.array_equal(M[f, :pb["N"]], o.map()), (tag, n_iter, f, pb["N"])
            o.close()


def pick_kernels(pb, pick):
    q = dict(pb)
    q["kernels"] = [pb["kernels"][k] for k in pick]
    return q


def take_points(pb, idx):
    q = dict(pb, N=len(idx), label=pb["label"][idx])
    q["kernels"] = [(np.ascontiguousarray(f[idx]), w) for f, w in pb["kernels"]]
    return q


def lattice(po, feat):
    """(vertex count, row lengths) of the oracle's lattice of one kernel's features"""
    n = feat.shape[0]
    o = po.OracleCRF(n, 2)
    o.set_unary_from_label(np.zeros(n, np.int16), np.float32(0.7))
    o.add_pairwise(feat, 1.0)
    k = o.kernel(0)
    o.close()
    return k["V"], np.bincount(k["offset"].reshape(-1), minlength=k["V"])


def frame_with_vertices(po, wl, target, seed):
    """a SLAM frame whose smoothness (short-row) lattice has exactly `target` vertices: points of a 2048-point frame, spread a little
    wider than the image so that the largest targets are in reach, taken in order; a point that would jump past the target is left out"""
    pb = wl.slam_problem(2048, seed=seed)
    f1 = (pb["kernels"][1][0] * np.float32(1.25)).astype(np.float32)
    pb["kernels"] = [pb["kernels"][0], (f1, pb["kernels"][1][1])]
    idx = np.arange(2048)
    for _ in range(64):
        lo, hi = 1, len(idx)                                  # smallest prefix with at least `target` vertices
        assert lattice(po, f1[idx])[0] >= target, (target, seed)
        while lo < hi:
            mid = (lo + hi) // 2
            if lattice(po, f1[idx[:mid]])[0] >= target:
                hi = mid
            else:
                lo = mid + 1
        if lattice(po, f1[idx[:lo]])[0] == target:
            return take_points(pb, idx[:lo])
        idx = np.delete(idx, lo - 1)
    raise AssertionError("no frame with %d vertices" % target)


@pytest.mark.parametrize("top", [1024, 1536, 2048])
def test_ragged_point_counts_at_every_points_per_lane(po, wl, top):
    """2, 3 and 4 points per lane (the batch's largest frame decides), frames around every boundary, a tiny and an empty one"""
    sizes = [n for n in (513, 1024, 1025, 1536, 1537, 2048) if n <= top] + [3, 0, top]
    base = [wl.slam_problem(n, seed=7100 + i) for i, n in enumerate(sizes)]
    check_batch(po, base, 1024 if top == 1024 else 2048, "top %d" % top)


@pytest.mark.parametrize("pick", [(1,), (0,)])
def test_one_kernel_alone(po, wl, pick):
    """the short-row kernel alone, and the appearance kernel alone (its long rows keep the chain lanes: nothing is renumbered)"""
    sizes = [2000, 1025, 1537, 2048, 700, 3, 0, 1999]
    base = [pick_kernels(wl.slam_problem(n, seed=7200 + i), pick) for i, n in enumerate(sizes)]
    check_batch(po, base, 2048, "pick %r" % (pick,))


def test_rows_of_n_products_in_the_short_row_kernel(po, wl):
    """one_cell: 3 vertices with rows of N products in BOTH kernels (far beyond the sort's last bucket); two_clusters: two very long
    chain rows beside an ordinary smoothness lattice"""
    base = [cc.shaped_problem(wl, 2000, "one_cell", 7301), cc.shaped_problem(wl, 1300, "one_cell", 7302),
            cc.shaped_problem(wl, 2000, "two_clusters", 7303), cc.shaped_problem(wl, 1537, "two_clusters", 7304),
            wl.slam_problem(2048, seed=7305), wl.slam_problem(600, seed=7306)]
    # 22 cells apart with 64, 66, .. 106 points each, the points shuffled: 66 rows, all of them longer than the 63 products the sort
    # tells apart, and the longest of them not the first in vertex order
    rng = np.random.default_rng(7307)
    cell = rng.permutation(np.repeat(np.arange(22), 64 + 2 * np.arange(22)))
    long_rows = wl.slam_problem(len(cell), seed=7307)
    f1 = (np.stack([cell, (cell * 7) % 1013], 1) * np.float32(9.0)).astype(np.float32)
    long_rows["kernels"] = [long_rows["kernels"][0], (f1, long_rows["kernels"][1][1])]
    V, rows = lattice(po, f1)
    assert V == 66 and rows.min() == 64 and rows.max() == 106
    check_batch(po, base + [long_rows], 2048, "one_cell / two_clusters / long rows")


@pytest.mark.parametrize("pick", [(0, 1), (0,)])
def test_rows_of_8(po, wl, pick):
    """rows_of_8: kernel 0 has hundreds of rows of 8 to 9 products -- no chain rows, so kernel 0 is a short-row kernel: alone in frames of
    up to 2048 points, and beside the smoothness kernel -- two renumbered kernels, one row at a time -- in frames of up to 1024
    points, whose two lattices' tables and products fit half a CU's LDS"""
    sizes = [2000, 1025, 1537, 2048, 520] if len(pick) == 1 else [1000, 700, 1024, 520, 900]
    base = [pick_kernels(cc.shaped_problem(wl, n, "rows_of_8", 7400 + i), pick) for i, n in enumerate(sizes)]
    check_batch(po, base, 2048 if len(pick) == 1 else 1024, "rows_of_8 %r" % (pick,))


def test_vertex_counts_around_the_wavefront_rounds(po, wl):
    """Short-row lattices of exactly 64 (one full wavefront), 512 and 513 (one round / one vertex into the second), 1024 and 1025, and
    1344 vertices (the most the plan admits -- in a batch of at most 1536 points per frame: with 2048 the plan for that many vertices
    is past half a CU's LDS), and one whose rows all have the same even length: 4 points per cell, cells apart"""
    nt = 512
    counts = [64, 512, 513, 1024, 1025, 3 * (nt - 64)]
    base = [frame_with_vertices(po, wl, v, 7500 + i) for i, v in enumerate(counts)]
    assert max(pb["N"] for pb in base) <= 1536
    for pb, v in zip(base, counts):
        assert lattice(po, pb["kernels"][1][0])[0] == v
    even = wl.slam_problem(1536, seed=7510)
    cell = np.arange(1536) // 4
    f1 = (np.stack([cell, (cell * 7) % 1013], 1) * np.float32(9.0)).astype(np.float32)
    even["kernels"] = [even["kernels"][0], (f1, even["kernels"][1][1])]
    V, rows = lattice(po, f1)
    assert V == 3 * 384 and (rows == 4).all()
    base += [even, wl.slam_problem(1536, seed=7511)]
    check_batch(po, base, 2048, "vertex counts")


def test_the_records_follow_the_lattices(po, wl):
    """other frames bound to the same handle and built again: the records are written again, for the new lattices"""
    maxN = 2048
    def batch(seed0):
        sizes = [2000, 1300, 2048, 1537, 3, 0, 1025, 1999]
        return [wl.slam_problem(sizes[f % 8], seed=seed0 + f % 8) for f in range(F)]

    def check(b, pbs, tag):
        Q, M = b.probability(), b.map()
        for f in list(range(8)) + [F - 8 + i for i in range(8)]:
            o = cc.setup(po.OracleCRF, pbs[f])
            o.inference_native(5, True)
            assert cc.same_bits(Q[f, :pbs[f]["N"]], o.probability()) and np.array_equal(M[f, :pbs[f]["N"]], o.map()), (tag, f)
            o.close()

    pbs = batch(7600)
    b = cc.batch_of(pbs, maxN=maxN)
    three_inferences(b, 5, 1.0, "first frames")
    assert b.fused_shape() == (512, 2) and b.last_prepare()[1] == 1
    check(b, pbs, "first frames")
    pbs2 = batch(7700)
    feats = [np.stack([np.pad(pb["kernels"][k][0], ((0, maxN - pb["N"]), (0, 0))) for pb in pbs2]) for k in range(2)]
    label = np.stack([np.pad(pb["label"], (0, maxN - pb["N"]), constant_values=-1) for pb in pbs2]).astype(np.int16)
    b.set_inputs_host([pb["N"] for pb in pbs2], feats, label=label, conf=pbs2[0]["conf"])
    three_inferences(b, 5, 1.0, "other frames")
    assert b.last_prepare()[1] == 2
    check(b, pbs2, "other frames")
    b.close()

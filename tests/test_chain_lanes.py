"""Chain lanes of the two-frames-per-CU loop (csrc/fused_lean.h: lean_chain_row, chain_setup_lean, phase S of mean_field_lean): ONE wavefront
per rank range of the appearance kernel's rows sums both labels of a row -- wavefront 0 the 16 longest rows, every further wavefront
32 ranks.  Every (row, label) is still added left to right by one lane through the same ring, so the results must not move by a bit.

One batch per points-per-lane shape of the plan (frames of up to 600, 1100 and 2000 points: 2, 3 and 4 points per lane), 256 frames
each.  The appearance features are built per frame on the CPU -- clusters of identical points (three rows of the cluster's size each)
plus isolated points that step the vertex count -- and the vertex count and the sorted row lengths are read from the CPU checker
before anything runs on the GPU: the frames must cover the vertex counts at which a wavefront fills up, the rings' trip boundaries
and ties between the top wavefront and the next (test_the_frames_cover_the_edges_of_the_mapping, no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

import crf_cases as cc
from chain_cases import descending, lattice, shaped_frame
from kernel_resources import HIPCC, ROOT

F = 256                                                       # (the smallest count that takes the two-frames-per-CU plan)
N_ITER = 3
SIZES = (600, 1100, 2000)
TOP, MAX_V = 16, 208                                          # rows of the top wavefront; the most vertices the chain lanes take
EDGES = [TOP + 32 * j + d for j in range(3) for d in (-1, 0, 1)]
TRIP_ROWS = [4 * q + d for q in (8, 16) for d in (-1, 0, 1)]  # a ring trip is 8 reads of 4 products: 31 .. 33 and 63 .. 65 products


@pytest.fixture(scope="module")
def plan_max_v0(tmp_path_factory):
    """f(points per frame, vertices of the smoothness lattice) -> the most appearance-lattice vertices with which the batch keeps the
    two-frames-per-CU plan: csrc/fused_lean.h's own layout_lean, compiled for the host (tests/cpp/chain_lanes_test.cpp).  Frames of
    2000 points with a smoothness lattice of ~1160 vertices fill half a CU's LDS a little before the chain lanes run out at 208."""
    exe = str(tmp_path_factory.mktemp("chain_plan") / "chain_lanes_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "lc-crf-slam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "chain_lanes_test.cpp"), "-o", exe],
                   check=True, capture_output=True)

    def most(NA, V1):
        out = subprocess.run([exe, str(NA), str(V1)], check=True, capture_output=True, text=True).stdout
        return int([ln for ln in out.splitlines() if ln.startswith("P ")][0].split()[1])
    return most


def batch_frames(po, wl, N, plan_max_v0):
    """the distinct frames of the batch of frames of up to N points: [(problem, V0, rows)]"""
    seed = 8000 + N
    room = N - 80                                             # (points left for the clusters beside up to 80 isolated ones)
    frames = [shaped_frame(po, wl, descending(4, N), 12, seed)]                              # fewer vertices than the top wavefront has rows
    for i, v in enumerate(EDGES):                             # a wavefront full but for one row, full, one row into the next
        frames.append(shaped_frame(po, wl, descending(4 if v < 18 else 5, room), v, seed + 1 + i))
    for i, L in enumerate(TRIP_ROWS):                         # the longest row ends at, before and behind a trip of the rings
        frames.append(shaped_frame(po, wl, [L, L - 1, L - 2, L - 3, L - 5, L - 7], 30, seed + 30 + i))
    frames.append(shaped_frame(po, wl, descending(6, room), 40, seed + 40))                  # ranks 15 .. 17 are one cluster's rows
    for i in range(2):                                        # and the real thing, at full size
        pb = wl.slam_problem(N, seed=seed + 50 + i)
        V, rows = lattice(po, pb["kernels"][0][0])
        frames.append((pb, V, np.sort(rows)[::-1]))
    # the most vertices the generator reaches: what the plan admits beside the batch's largest smoothness lattice, 208 at the most
    V1 = max(lattice(po, pb["kernels"][1][0])[0] for pb, _, _ in frames)
    frames.append(shaped_frame(po, wl, descending(5, room), plan_max_v0(N, V1), seed + 20))
    return frames


@pytest.fixture(scope="module")
def frames(po, wl, plan_max_v0):
    return {N: batch_frames(po, wl, N, plan_max_v0) for N in SIZES}


@pytest.mark.parametrize("N", SIZES)
def test_the_frames_cover_the_edges_of_the_mapping(po, frames, plan_max_v0, N):
    """a condition on the inputs, checked on the CPU"""
    fr = frames[N]
    most = plan_max_v0(N, max(lattice(po, pb["kernels"][1][0])[0] for pb, _, _ in fr))
    assert (most == MAX_V or N == 2000) and EDGES[-1] + 32 < most <= MAX_V
    assert max(pb["N"] for pb, _, _ in fr) == N and all(pb["N"] <= N for pb, _, _ in fr)
    vs = {V for _, V, _ in fr}
    assert min(vs) < TOP and set(EDGES) <= vs and max(vs) == most, sorted(vs)
    longest = {int(rows[0]) for _, _, rows in fr}
    assert set(TRIP_ROWS) <= longest, sorted(longest)
    assert max(longest) >= 64                                 # (the batch's longest row is what asks for the chain lanes)
    assert any(V > TOP and rows[TOP - 1] == rows[TOP] and rows[TOP] >= 64 for _, V, rows in fr)      # the 16th and 17th rows tie
    assert any(V > TOP and rows[TOP - 1] > rows[TOP] for _, V, rows in fr)                           # ... and do not
    assert any(0 < int((rows >= 64).sum()) < TOP for _, _, rows in fr)                               # fewer than 16 long rows
    assert any(int((rows >= 64).sum()) > TOP for _, _, rows in fr)


def run_every_way(b, lean):
    """inference() three times (self-contained, prepare + run, run from the blocks), one run() (the one-launch kernel), and the
    streaming engine on the same batch: every result the same bits as the streaming engine's; returns them"""
    results = []
    b.build()
    b.inference(N_ITER, True)
    assert b.engine() == 2
    assert (b.fused_shape() == (512, 2)) == lean, b.fused_shape()
    results.append(("self-contained", b.probability(), b.map()))
    runs0 = b.last_prepare()[1]
    for tag in ("prepare + run", "from the blocks"):
        b.inference(N_ITER, True)
        results.append((tag, b.probability(), b.map()))
    if lean:
        assert b.last_prepare()[1] == runs0 + 1               # (the second inference wrote the blocks, the third reused them)
    b.run(N_ITER, True)
    assert b.engine() == 3
    results.append(("run", b.probability(), b.map()))
    b.set_engine(1)
    b.inference(N_ITER, True)
    assert b.engine() == 1
    Q, M = b.probability(), b.map()
    for tag, q, m in results:
        assert cc.same_bits(q, Q) and np.array_equal(m, M), tag
    return Q, M


def check_against_the_checker(po, fr, Q, M):
    """every distinct frame, first and last copy: labels identical, Q the same bits (bench.py: check_distinct_frames asks for labels
    and max |dQ|; the same bits are no less)"""
    for i, (pb, _, _) in enumerate(fr):
        o = cc.setup(po.OracleCRF, pb)
        o.inference_native(N_ITER, True)
        for f in (i, i + (F - 1 - i) // len(fr) * len(fr)):
            assert np.array_equal(M[f, :pb["N"]], o.map()), (i, f)
            assert cc.same_bits(Q[f, :pb["N"]], o.probability()), (i, f)
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_both_labels_of_a_row_in_one_wavefront(po, frames, N):
    fr = frames[N]
    b = cc.batch_of([fr[f % len(fr)][0] for f in range(F)], maxN=N)
    Q, M = run_every_way(b, lean=True)
    b.close()
    check_against_the_checker(po, fr, Q, M)


@pytest.mark.gpu
def test_more_vertices_than_the_chain_lanes_take(po, wl, frames):
    """appearance lattices of more than 208 vertices beside ordinary ones: the batch leaves the two-frames-per-CU plan and must still agree"""
    N = SIZES[1]
    fr = [shaped_frame(po, wl, descending(5, N - 100), v, 8900 + v) for v in (MAX_V + 1, MAX_V + 30)] + frames[N][-5:-1]
    assert max(V for _, V, _ in fr) > MAX_V and max(int(rows[0]) for _, _, rows in fr) >= 64
    b = cc.batch_of([fr[f % len(fr)][0] for f in range(F)], maxN=N)
    Q, M = run_every_way(b, lean=False)
    b.close()
    check_against_the_checker(po, fr, Q, M)

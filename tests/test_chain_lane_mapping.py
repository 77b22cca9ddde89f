"""Which chain row a lane of the two-frames-per-CU loop sums (csrc/fused_lean.h: lean_chain_row, lean_chain_waves): one wavefront per
rank range with both labels of a row in it.  Checked on the host (no GPU needed: the functions are __host__ __device__ constexpr)."""
import os
import shutil
import subprocess

import pytest

from kernel_resources import HIPCC, ROOT

NT = 512


@pytest.fixture(scope="module")
def mapping(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_lanes") / "chain_lanes_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "lc-crf-slam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "chain_lanes_test.cpp"), "-o", exe],
                   check=True, capture_output=True)
    lanes, waves, top = {}, {}, None
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "L":
            lanes[int(w[1])] = (int(w[2]), int(w[3]))
        elif w[0] == "W":
            waves[int(w[1])] = int(w[2])
        else:
            top = (int(w[1]), int(w[2]))
    return lanes, waves, top


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_every_row_and_label_has_one_lane_at_every_vertex_count(mapping):
    lanes, waves, (top, max_v) = mapping
    assert sorted(lanes) == list(range(NT)) and (top, max_v) == (16, 208) and sorted(waves) == list(range(max_v + 1))
    for t, (r, l) in lanes.items():
        assert (r == -1 and l == -1) or (r >= 0 and l in (0, 1)), (t, r, l)
    for V0 in range(max_v + 1):
        active = {t: rl for t, rl in lanes.items() if 0 <= rl[0] < V0}       # (chain_setup_lean: a rank >= V0 is no row)
        # every (rank < V0, label) on exactly one lane, and -- by the filter above -- no lane with a rank >= V0
        assert sorted(active.values()) == [(r, l) for r in range(V0) for l in (0, 1)], V0
        # both labels of a row in ONE wavefront, every such wavefront among those phase S lets into the chain
        wave_of = {}
        for t, (r, l) in active.items():
            assert wave_of.setdefault(r, t >> 6) == t >> 6, (V0, r)
            assert t >> 6 < waves[V0] <= NT // 64, (V0, t)
        # the top wavefront holds the `top` longest rows, every further one 32 ranks in rank order
        for r, w in wave_of.items():
            assert w == (0 if r < top else 1 + (r - top) // 32), (V0, r, w)
        assert waves[V0] == 1 + (max(V0 - top, 0) + 31) // 32
        # the top wavefront's lanes per 16-lane group (what one ds_read_b128 is served in): label 1 sits 16 lanes above label 0,
        # so the groups of a label pair always agree; with all `top` rows present, all four groups hold equally many
        groups = [sum(1 for t in active if t < 64 and t // 16 == g) for g in range(4)]
        assert groups[0] == groups[1] and groups[2] == groups[3], (V0, groups)
        if V0 >= top:
            assert groups == [top // 2] * 4, (V0, groups)
    # (the assignment itself, before a vertex count clips it: equally many lanes in each group of the top wavefront)
    assert [sum(1 for t in range(g * 16, g * 16 + 16) if lanes[t][0] >= 0) for g in range(4)] == [top // 2] * 4
    for t, (r, l) in lanes.items():
        if t < 64 and l == 1:
            assert lanes[t - 16] == (r, 0), t

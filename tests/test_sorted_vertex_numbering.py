"""The numbering the prepared launch records give a short-row kernel's vertices (csrc/fused_lean.h: lean_sorted_vertex, rank by
descending row length -> vertex number), checked on the host (no GPU needed: the function is __host__ __device__)."""
import os
import shutil
import subprocess

import pytest

from kernel_resources import HIPCC, ROOT

NT = 512
COUNTS = [1, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1160, 1343, 1344]


@pytest.fixture(scope="module")
def numbering(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sorted_vertex") / "sorted_vertex_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "lc-crf-slam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sorted_vertex_test.cpp"), "-o", exe],
                   check=True, capture_output=True)
    out = subprocess.run([exe] + [str(v) for v in COUNTS], check=True, capture_output=True, text=True).stdout
    maps = {v: {} for v in COUNTS}
    for line in out.splitlines():
        V, q, n = (int(x) for x in line.split())
        maps[V][q] = n
    return maps


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
@pytest.mark.parametrize("V", COUNTS)
def test_ranks_map_onto_the_vertex_numbers_wavefront_by_wavefront(numbering, V):
    m = numbering[V]
    assert sorted(m) == list(range(V)) and sorted(m.values()) == list(range(V))          # a bijection on [0, V)
    rank_of = {n: q for q, n in m.items()}
    for q, n in m.items():
        assert n // NT == q // NT                                                        # round r holds ranks [r NT, (r + 1) NT)
        assert n % 64 == q % 64                                                          # the lane is the rank's place in its chunk
    for c0 in range(0, V, 64):                                                           # a wavefront-round: 64 consecutive ranks, in lane
        ranks = [rank_of[n] for n in range(c0, min(c0 + 64, V))]                         # order: lane 0 has the longest row
        assert ranks == list(range(ranks[0], ranks[0] + len(ranks))) and ranks[0] % 64 == 0
    for r in range((V + NT - 1) // NT):                                                  # full odd rounds are dealt backwards
        first = [rank_of[c0] // 64 for c0 in range(r * NT, min((r + 1) * NT, V), 64)]
        full = (r + 1) * NT <= V
        want = list(range(r * 8, r * 8 + len(first)))
        assert first == (want[::-1] if (r & 1) and full else want), (r, first)

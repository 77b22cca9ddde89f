"""The streaming build of locality mode on the device, branch by branch (csrc/stream_build.hip: launch_sort_points, the sorted build, and
the hash build of the same permuted frames) -- notes/sorted_build_tests.md.

Every case of tests/sorted_build_cases.py is a two-label BatchCRF on the release library, no environment switch.  For every frame:
  * locality_mode() and build_report() -- what the build kernels counted about their own branches -- equal the numpy restatement field
    by field, and satisfy the claim the case was built for: a case that lands in another branch FAILS;
  * the tables as built (built_lattice(): no rebuild, internal order, the build's ids) pass tests/sorted_build_checker.py against the
    oracle's lattice: renumbering a bijection, weights, neighbours, rows in ascending original order, fastn, row-major ids;
  * lattice_sizes, and Q / labels after 3 iterations at relax 0.9, are the oracle's bits.
No tolerance anywhere.  tests/test_sorted_build_cases.py proves the case table and tests/test_sorted_build_checker.py the checker
without a GPU.
"""
import importlib

import numpy as np
import pytest

import sorted_build_cases as sb
import sorted_build_checker as sc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu


def run_case(po, c, sorted_build):
    fs, max_points = sb.features(c)
    refs = sb.oracle(po, c)
    want = sb.expected(po, c, sorted_build)
    F = len(fs)
    feat = np.zeros((F, max_points, c.d), np.float32)
    un = np.zeros((F, max_points, 2), np.float32)
    for i, (_, _, _, f, u) in enumerate(refs):
        feat[i, :f.shape[0]], un[i, :f.shape[0]] = f, u
    b = pkg.BatchCRF(F, max_points, 2, [c.d], [1.0])
    try:
        if not sorted_build:
            b.set_option(pkg.OPT_VERTEX_ORDER, 2)
        b.set_inputs_host([f.shape[0] for f in fs], [feat], unary=un)
        b.build()
        assert b.locality_mode() == (True, sorted_build), (c.name, b.locality_mode())
        got = [b.build_report(0, i) for i in range(F)]
        print(c.name, "sorted" if sorted_build else "hash", [{k: v for k, v in r.items() if v} for r in got])
        assert got == want, (c.name, got, want)
        claim = c.claim if sorted_build else c.hash_claim
        assert claim is None or claim(got), (c.name, c.branch, got)
        sizes = b.lattice_sizes(0)
        for i, (ref, _, _, f, _) in enumerate(refs):
            assert int(sizes[i]) == ref["V"], (c.name, i, int(sizes[i]), ref["V"])
            t = b.built_lattice(0, i)
            assert t["N"] == f.shape[0] and (t["fastn"] is not None) == sorted_build
            sc.check(ref, t, sorted_build)
        b.inference(sb.T, True, relax=sb.RELAX)
        assert b.engine() == 1 and b.locality_mode() == (True, sorted_build)
        q, m = b.probability(), b.map()
        assert [b.build_report(0, i) for i in range(F)] == want                       # (a report of the BUILD: the inference changes nothing)
        for i, (_, qo, mo, f, _) in enumerate(refs):
            n = f.shape[0]
            assert np.array_equal(q[i, :n].view(np.int32), qo.view(np.int32)) and np.array_equal(m[i, :n], mo), (c.name, i)
        return q
    finally:
        b.close()


@pytest.mark.parametrize("name", [c.name for c in sb.CASES])
def test_sorted_build_case(po, name):
    c = sb.BY_NAME[name]
    q = run_case(po, c, True)
    if c.twice:             # a bucket of more than 64 points keeps its arrival order, which differs from run to run: nothing may depend on it
        assert np.array_equal(run_case(po, c, True).view(np.int32), q.view(np.int32))


@pytest.mark.parametrize("name", [c.name for c in sb.CASES])
def test_hash_build_of_permuted_frames_case(po, name):
    """LCCRF_OPT_VERTEX_ORDER = 2: the points stay permuted, the vertices come from the hash table, the rows from k_csr_order /
    k_csr_sort_long -- the same checker applies, less the numbering"""
    c = sb.BY_NAME[name]
    q = run_case(po, c, False)
    if c.twice:
        assert np.array_equal(run_case(po, c, False).view(np.int32), q.view(np.int32))


def test_handle_reports_its_build(po):
    """lccrf_get_build_report on a DenseCRFHIP handle: the sorted build's report behind inference() of a large frame, and an all-zero
    report for a SLAM-size frame, which the one-workgroup build makes"""
    c = sb.BY_NAME["uniform_1024"]
    (ref, qo, mo, f, u), = sb.oracle(po, c)
    h = pkg.DenseCRFHIP(f.shape[0], 2)
    h.set_unary(u)
    h.add_pairwise(f, 1.0)
    h.inference(sb.T, True, sb.RELAX)
    assert h.build_report(0) == sb.expected(po, c, True)[0], h.build_report(0)
    assert np.array_equal(h.probability().view(np.int32), qo.view(np.int32)) and np.array_equal(h.map(), mo)
    h.close()
    h = pkg.DenseCRFHIP(500, 2)
    h.set_unary(u[:500])
    h.add_pairwise(f[:500], 1.0)
    h.inference(2, True)
    assert h.build_report(0) == dict.fromkeys(sb.FIELDS, 0), h.build_report(0)
    h.close()

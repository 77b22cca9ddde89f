"""The window splat (csrc/stream_filter.hip: k_splat2w) on every window, lane shape and halo edge -- notes/splat_window_tests.md.

Every case of tests/splat_plan_cases.py is built on the device; the plan the library reports (lccrf_batch_get_splat_plan: passes, halo,
window, lanes, vertices per lane, long_mode) must equal the CPU restatement's field by field -- which also holds the build's
neighbour-distance count to an independent one and ties the case to the kernel instantiation that ran -- and V per term, Q and the MAP
labels of every non-empty frame must be the oracle's bit for bit, twice.  tests/test_splat_plan_cases.py shows without a GPU that each
case sends values through the halo in its first, an interior and its last window."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import crf_cases as cc
import splat_plan_cases as sp

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

_oracle = {}


def oracle_frame(po, case, f):
    """(V per term, Q, map) of frame f after ITERATIONS at RELAX; computed once per distinct frame and left unchanged"""
    n, seed = case.frame_specs[f]
    key = (tuple(tuple(case.sides(k, f)) for k in range(len(case.terms))), tuple(case.weights), n, seed)
    if key not in _oracle:
        fr = case.frames()[f]
        o = cc.setup(po.OracleCRF, fr)
        o.inference_native(sp.ITERATIONS, True, sp.RELAX)
        _oracle[key] = ([o.kernel(k)["V"] for k in range(len(fr["kernels"]))], o.probability().copy(), o.map().copy())
        o.close()
    return _oracle[key]


def expected_plan(case):
    return np.array([[case.plan(k)[n] for n in sp.PLAN_FIELDS] for k in range(len(case.terms))], np.int64)


def check_batch(po, case, got):
    want = expected_plan(case)
    print(case.name, "plan", dict(zip(sp.PLAN_FIELDS, got["plan"][0].tolist())), "restated", dict(zip(sp.PLAN_FIELDS, want[0].tolist())))
    assert np.array_equal(got["plan"], want), (case.name, got["plan"].tolist(), want.tolist())
    assert np.array_equal(got["plan_after"], want), case.name
    assert int(got["engine"]) == 1 and got["locality"].tolist() == [1, 1], case.name
    for f, spec in enumerate(case.frame_specs):
        if not spec:
            assert not got["V"][:, f].any(), (case.name, f)
            continue
        n = spec[0]
        V, Q, M = oracle_frame(po, case, f)
        assert got["V"][:, f].tolist() == V, (case.name, f)
        for rep in range(2):
            assert cc.same_bits(got["Q%d" % rep][f, :n], Q), (case.name, f, rep, float(np.abs(got["Q%d" % rep][f, :n] - Q).max()))
            assert np.array_equal(got["map%d" % rep][f, :n], M), (case.name, f, rep)


@pytest.mark.parametrize("case", [c for c in sp.CASES if c.api == "batch" and c.passes_cap is None], ids=lambda c: c.name)
def test_window_splat_matches_the_plan_and_the_oracle(po, case):
    check_batch(po, case, sp.run_batch(case))


@pytest.mark.parametrize("case", [c for c in sp.CASES if c.passes_cap is not None], ids=lambda c: c.name)
def test_window_splat_under_the_pass_cap(po, case, tmp_path):
    """LCCRF_SPLAT_PASSES=2 (instrumented library, a child process): two passes in the window where three would fit -- and on a
    single-frame engine with d >= 3 the demotion to one."""
    path = str(tmp_path / "got.npz")
    subprocess.run([sys.executable, os.path.join(sp.ROOT, "tests", "splat_plan_cases.py"), case.name, path], check=True,
                   env=cc.switch_env(case.env()), timeout=300)
    got = dict(np.load(path))
    check_batch(po, case, got)


def test_one_batch_handle_follows_new_inputs(po):
    """wide, narrow, wide on one handle, rebuilt each time: the plan follows (nothing stale in the distance count or the byte-offset
    table), and so do the results"""
    cases = [sp.BY_NAME[n] for n in sp.REBUILD_SEQUENCE]
    _, dims, _, _ = sp.batch_inputs(cases[0])
    b = pkg.BatchCRF(cases[0].F, cases[0].max_points, 2, dims, [float(w) for w in cases[0].weights])
    for case in cases:
        check_batch(po, case, sp.run_batch(case, b))
    b.close()


def test_object_api_handle_runs_the_window_and_leaves_it_for_stepwise_inference(po):
    case = next(c for c in sp.CASES if c.api == "object")
    fr = case.frames()[0]
    h, o = cc.setup(pkg.DenseCRFHIP, fr), cc.setup(po.OracleCRF, fr)
    o.inference_native(sp.ITERATIONS, True, sp.RELAX)
    want = dict(zip(sp.PLAN_FIELDS, expected_plan(case)[0].tolist()))
    for rep in range(2):
        h.inference(sp.ITERATIONS, True, sp.RELAX)
        assert h.splat_plan(0) == want, (rep, h.splat_plan(0), want)
        assert h.engine()[0] == 1
        assert cc.same_bits(h.probability(), o.probability()) and np.array_equal(h.map(), o.map()), rep
    h.step_inference(sp.RELAX)                             # continues on lattices built the plain way: no pass in the splat
    o.step_inference(sp.RELAX)
    assert h.splat_plan(0) == dict.fromkeys(sp.PLAN_FIELDS, 0)
    assert cc.same_bits(h.probability(), o.probability())
    assert h.kernel(0)["V"] == o.kernel(0)["V"] == case.lattices(0)[0].V
    h.close(); o.close()

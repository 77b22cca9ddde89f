"""Every route of the two-label step's blur passes (csrc/engine.h: blur_plan; csrc/stream_filter.hip: k_blur2x2t, k_blur2x2, k_blur2<NT>,
k_blur2c, k_slice2<D1, true>) -- notes/blur_plan_tests.md.

Every case of tests/blur_plan_cases.py is built on the device, on the streaming engine.  The plan the library reports
(lccrf_batch_get_blur_plan) must equal the CPU restatement's field by field for every term -- behind the build, behind two inferences
and behind a rebuild -- which ties the case to the kernels that ran; and V per term, Q and the MAP labels of every frame must be the
oracle's bit for bit after each of the three inferences.  No tolerance anywhere.  tests/test_blur_plan_cases.py shows without a GPU
that the table holds every route and edge it claims."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import blur_plan_cases as bp
import crf_cases as cc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu


def expected_rows(case):
    return np.array([[e["plan"][n] for n in bp.PLAN_FIELDS] for e in case.expected()], np.int64)


def check_batch(po, case, got):
    want = expected_rows(case)
    for k in range(len(case.terms)):
        print(case.name, "term", k, "plan", dict(zip(bp.PLAN_FIELDS, got["plan"][k].tolist())), "restated", dict(zip(bp.PLAN_FIELDS, want[k].tolist())))
    for when in ("plan", "plan_after", "plan_rebuilt"):
        assert np.array_equal(got[when], want), (case.name, when, got[when].tolist(), want.tolist())
    assert got["plan"][:, :6].sum(1).tolist() == [d + 1 for d in case.dims]
    assert got["splat"].tolist() == want[:, 0].tolist(), case.name                  # (in_splat IS the splat plan's passes)
    assert int(got["engine"]) == 1, case.name
    for f, spec in enumerate(case.frame_specs):
        if not spec:
            assert not got["V"][:, f].any(), (case.name, f)
            continue
        n = spec[0]
        V, Q, M = bp.oracle_frame(po, case, f)
        assert got["V"][:, f].tolist() == V, (case.name, f)
        for rep in range(3):
            assert cc.same_bits(got["Q%d" % rep][f, :n], Q), (case.name, f, rep, float(np.abs(got["Q%d" % rep][f, :n] - Q).max()))
            assert np.array_equal(got["map%d" % rep][f, :n], M), (case.name, f, rep)


@pytest.mark.parametrize("case", [c for c in bp.CASES if not c.env], ids=lambda c: c.name)
def test_blur_passes_take_the_planned_routes_and_match_the_oracle(po, case):
    check_batch(po, case, bp.run_batch(case))


@pytest.mark.parametrize("case", [c for c in bp.CASES if c.env], ids=lambda c: c.name)
def test_blur_plan_under_the_instrumented_switches(po, case, tmp_path):
    """The instrumented library in a child process: the compact table abandoned (LCCRF_NBRC_SPAN) or switched off, pass 0 given its own
    launch back while the two-hop table still starts at pass 1 (LCCRF_FAST0_BREAK), passes one per launch on a single frame
    (LCCRF_NO_PAIR_FUSE: the only way to the last pass of SINGLES in the slice), pairs without the table (LCCRF_NO_2HOP_TABLE), and
    d + 1 = 2 with pass 0 in the splat (LCCRF_SPLAT_PASSES=1: the one pass alone in pair mode)."""
    path = str(tmp_path / "got.npz")
    subprocess.run([sys.executable, os.path.join(bp.ROOT, "tests", "blur_plan_cases.py"), case.name, path], check=True,
                   env=cc.switch_env(case.env), timeout=300)
    check_batch(po, case, dict(np.load(path)))


def test_object_api_handle_reports_the_plan(po):
    """lccrf_get_blur_plan on a DenseCRFHIP handle of a large frame: the sorted build's plan behind inference(), and the plain lattices'
    plan (nothing in the splat, the two-hop table from pass 0) once step_inference has rebuilt them the plain way"""
    case = bp.BY_NAME["sorted1_j3_D5"]
    fr = case.frames()[0]
    h, o = cc.setup(pkg.DenseCRFHIP, fr), cc.setup(po.OracleCRF, fr)
    h.inference(bp.ITERATIONS, True, bp.RELAX)
    o.inference_native(bp.ITERATIONS, True, bp.RELAX)
    assert h.blur_plan(0) == case.plan(), (h.blur_plan(0), case.plan())
    assert h.engine()[0] == 1
    assert cc.same_bits(h.probability(), o.probability()) and np.array_equal(h.map(), o.map())
    h.step_inference(bp.RELAX)
    o.step_inference(bp.RELAX)
    st = case.expected()[0]["state"]
    assert h.blur_plan(0) == bp.route_counts(st["D1"], 0, 1, st["maxV"], True, 0, False), h.blur_plan(0)
    assert cc.same_bits(h.probability(), o.probability())
    h.close(); o.close()

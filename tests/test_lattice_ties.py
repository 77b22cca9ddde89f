"""The lattice build's rounding rule (ties to even, quirk Q2) and rank rule (strict '<', Q3) on the device, at inputs where they bind:
the cases of tests/lattice_tie_cases.py (exact rounding ties, axis double ties, exact rank ties; tests/test_lattice_tie_cases.py shows
that a wrong rule moves keys on every one of them) through every text that sits downstream of lattice_simplex (csrc/device_math.h):

  point_record<D>, one-workgroup build   csrc/build_small.hip     handles of d <= 3 and a few hundred points; engines 1 and 2 of a batch
  point_record<D>, streaming hashed      csrc/stream_build.hip    k_points<D>: handles of d >= 4, frames padded beyond the one-workgroup
                                                                  build's range, the SLAM frames under LCCRF_NO_FUSED_BUILD
  point_record<2>, frame kernels         csrc/frame_body.inc      a fresh handle's inference(), batch.run(), run_converged,
                                                                  LCCRF_OPT_FRAME_GENERAL
  point_record2_grid                     csrc/frame_build.h       batch.run() of 256 frames (two frames per CU)
  k_sort_cells + k_points<D, true>       csrc/stream_build.hip    locality mode: frames of 8192 points, the sorted build
  k_corner_to_feature                    csrc/meanfield_backward.hip   tests/test_feature_gradients.py (gradient_settings.TIES)

Which build runs is decided by Engine::build_kernels (csrc/host_engine.hip): locality mode (point order + sorted build) from
perm_min_points() = 8192 points when the caller allows a reorder; else the one-workgroup build where build_small_supported() -- d <= 3,
at most 12 x 1024 lattice entries, the LDS plan -- and LCCRF_NO_FUSED_BUILD is unset; else the streaming hashed build.  The engine is
choose_sized_engine()'s; a fresh two-label, two-term frame takes the one-launch frame kernel before any of that.  Every test asserts
the route it is there for with the library's reports (engine(), fused_shape(), fallback_frames(), locality_mode(), splat_plan()) and,
where the library reports nothing (which hashed build made a handle's lattices), with the rule restated from the sizes.

Every comparison is bit for bit: with tests/golden/ties.npz (written by the reference build itself) where it has the case, else with the
oracle.  Routes and what the device did: notes/lattice_ties.md."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import converge_cases as cv
import crf_cases as cc
import frame_lean_cases as fc
import lattice_tie_cases as tc
import normalization_checker as nc
from joint_checker import dense

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ties.npz")
INTERNALS = ("offset", "bary", "nbr", "norm")
_Z, _REFS = {}, {}


def _z():
    if "z" not in _Z:
        _Z["z"] = np.load(FIXTURE)
    return _Z["z"]


def _fixture(name):
    """(problem, dict(V, offset.., trace, map, T, relax)) of a fixture case: what the reference build gave on the stored inputs"""
    if name not in _REFS:
        z, p = _z(), name.replace(":", "_")
        pb = cc.case_problem(z, p)
        K = len(pb["kernels"])
        ref = dict(V=[int(z["%s_V%d" % (p, k)]) for k in range(K)], trace=z[p + "_trace"], map=z[p + "_map"], T=int(z["iters"]),
                   relax=float(z["relax"]))
        for what in INTERNALS:
            ref[what] = [z["%s_%s%d" % (p, what, k)] for k in range(K)]
        _REFS[name] = (pb, ref)
    return _REFS[name]


def _one_workgroup_build(pb):
    """Engine::build_kernels' rule for a frame below the locality threshold, restated from the sizes (build_small_supported; the LDS plan
    of csrc/build_small.hip holds for every frame it is asked about here: 115 KB of 158 at 2047 points of d = 2)"""
    n4 = (pb["N"] + 3) & ~3
    return pb["N"] < 8192 and all(f.shape[1] <= 3 and n4 * (f.shape[1] + 1) <= 12 * 1024 for f, _ in pb["kernels"])


def _assert_internals(kv, ref, k, tag):
    assert kv["V"] == ref["V"][k], (tag, k, kv["V"], ref["V"][k])
    for what in INTERNALS:
        assert cc.same_bits(kv[what], ref[what][k]), (tag, k, what)


def _oracle_ref(po, pb, T, relax):
    o = cc.setup(po.OracleCRF, pb)
    K = len(pb["kernels"])
    ks = [o.kernel(k) for k in range(K)]
    ref = dict(V=[kv["V"] for kv in ks], trace=o.run_trace(T, relax), T=T, relax=relax)
    for what in INTERNALS:
        ref[what] = [kv[what] for kv in ks]
    o.build_map()
    ref["map"] = o.map()
    o.close()
    return ref


# ---- handle internals: the one-workgroup build (d <= 3) and the streaming hashed build (d >= 4) ----------------------------------------
@pytest.mark.parametrize("name", tc.GENERIC)
def test_handle_internals_and_step_trace_are_the_references(name):
    """h.kernel(0) (V, offset, bary, nbr, norm) and the step path's trace against the reference build's record.  d <= 3: the
    one-workgroup build (build_small.hip); d >= 4: k_points<D> of the streaming hashed build."""
    pb, ref = _fixture(name)
    d = pb["kernels"][0][0].shape[1]
    assert _one_workgroup_build(pb) == (d <= 3)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    _assert_internals(h.kernel(0), ref, 0, name)
    assert cc.same_bits(h.run_trace(ref["T"], ref["relax"]), ref["trace"]), name
    h.build_map()
    assert np.array_equal(h.map(), ref["map"]), name
    assert h.splat_plan(0)["passes"] == 0                        # a hashed build: no blur pass rides in the splat
    h.close()


@pytest.mark.parametrize("d", (1, 2, 3))
def test_streaming_hashed_build_of_small_dimensions(po, d):
    """k_points<1..3>: the case followed by filler points up to a size the one-workgroup build does not take.  Vertices are numbered by
    first occurrence in point order, so the case's own rows of offset and bary are the reference record's; everything else against
    the oracle on the padded frame.  The route: the size rule, and long_mode > 0 -- only the streaming build lists long rows, and the
    filler makes the rows long (N (d + 1) > 4 V on the oracle's V)."""
    name = "ties:d%d" % d
    small, fix = _fixture(name)
    pb = tc.padded(small, tc.padded_size(d))
    assert not _one_workgroup_build(pb) and pb["N"] < 8192
    ref = _oracle_ref(po, pb, 3, 0.75)
    assert pb["N"] * (d + 1) > 4 * ref["V"][0]
    h = cc.setup(pkg.DenseCRFHIP, pb)
    kv = h.kernel(0)
    _assert_internals(kv, ref, 0, name)
    n = small["N"]
    assert np.array_equal(kv["offset"][:n], fix["offset"][0]) and cc.same_bits(kv["bary"][:n], fix["bary"][0])
    assert cc.same_bits(h.run_trace(3, 0.75), ref["trace"])
    plan = h.splat_plan(0)
    assert plan["long_mode"] > 0 and plan["passes"] == 0, plan
    h.close()


_CHILD = r"""
import importlib, sys, numpy as np
sys.path[:0] = [%r, %r]
import crf_cases as cc
pkg = importlib.import_module("lc-crf-slam_amd")
z = np.load(%r)
out = {}
for name in sys.argv[2:]:
    pb = cc.case_problem(z, name)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for k in range(2):
        kv = h.kernel(k)
        out["%%s_V%%d" %% (name, k)] = np.int64(kv["V"])
        for what in ("offset", "bary", "nbr", "norm"):
            out["%%s_%%s%%d" %% (name, what, k)] = kv[what]
    out[name + "_trace"] = h.run_trace(int(z["iters"]), float(z["relax"]))
    h.build_map()
    out[name + "_map"] = h.map()
    h.close()
np.savez(sys.argv[1], **out)
"""


def test_slam_frames_on_the_streaming_hashed_build_in_a_child_process(tmp_path):
    """k_points<2> on the SLAM shape: LCCRF_NO_FUSED_BUILD is a cross-check switch of the instrumented library, so the build runs in a
    child process (cc.switch_env).  Both frames' internals, step trace and labels against the reference record; this process's handle
    on the one-workgroup build gives the same."""
    names = [n.replace(":", "_") for n in tc.SLAM]
    path = str(tmp_path / "ties_streaming_build.npz")
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), FIXTURE)
    env = cc.switch_env({"LCCRF_NO_FUSED_BUILD": "1"})
    assert env["LCCRF_LIB"] == cc.INSTR_LIB and env["LCCRF_NO_FUSED_BUILD"] == "1"
    subprocess.run([sys.executable, "-c", code, path] + names, check=True, env=env, timeout=120)
    got = np.load(path)
    for name, p in zip(tc.SLAM, names):
        pb, ref = _fixture(name)
        assert _one_workgroup_build(pb)                           # (what this process's handle runs, below)
        h = cc.setup(pkg.DenseCRFHIP, pb)
        for k in range(2):
            child = dict(V=int(got["%s_V%d" % (p, k)]), **{w: got["%s_%s%d" % (p, w, k)] for w in INTERNALS})
            _assert_internals(child, ref, k, (name, "streaming"))
            _assert_internals(h.kernel(k), ref, k, (name, "one workgroup"))
        assert cc.same_bits(got[p + "_trace"], ref["trace"]) and np.array_equal(got[p + "_map"], ref["map"]), name
        assert cc.same_bits(h.run_trace(ref["T"], ref["relax"]), ref["trace"]), name
        h.close()


# ---- the SLAM frames on every two-label route -----------------------------------------------------------------------------------------
def _check_handle(h, ref, tag):
    assert h.engine() == (3, 0), (tag, h.engine())
    assert cc.same_bits(h.probability(), ref["trace"][ref["T"]]), tag
    assert np.array_equal(h.map(), ref["map"]), tag


@pytest.mark.parametrize("name", tc.SLAM)
def test_fresh_handle_runs_the_frame_kernel_in_two_workgroups_and_in_one(po, name):
    """point_record<2> of csrc/frame_body.inc: inference() on a fresh handle is one launch of the frame kernel (engine 3), in two
    workgroups by default and in one with LCCRF_OPT_SINGLE_WORKGROUP.  The lattices it leaves in HBM are the reference's too."""
    pb, ref = _fixture(name)
    for single in (0, 1):
        h = pkg.DenseCRFHIP(pb["N"], pb["L"])
        h.set_option(pkg.OPT_SINGLE_WORKGROUP, single)
        h.set_unary_from_label(pb["label"], pb["conf"])
        for f, w in pb["kernels"]:
            h.add_pairwise(f, w)
        h.inference(ref["T"], True, ref["relax"])
        _check_handle(h, ref, (name, single))
        h.inference(5, True)                                      # (and the call of the tracker: five iterations, no damping)
        assert h.engine() == (3, 0)
        q5 = h.probability()
        for k in range(2):
            _assert_internals(h.kernel(k), ref, k, (name, single))
        h.close()
        o5 = _five(po, name, pb)
        assert cc.same_bits(q5, o5), (name, single)


def _five(po, name, pb):
    key = (name, "five")
    if key not in _REFS:
        o = cc.setup(po.OracleCRF, pb)
        o.inference_native(5, True)
        _REFS[key] = o.probability()
        o.close()
    return _REFS[key]


@pytest.mark.parametrize("name", tc.SLAM)
def test_batch_engines_one_two_and_three(name):
    """the one-workgroup build under the streaming engine (1) and the fused engine (2), and batch.run's frame kernel (3)"""
    pb, ref = _fixture(name)
    assert _one_workgroup_build(pb)
    for engine in (1, 2, 3):
        b = cc.batch_of([pb])
        if engine == 3:
            b.run(ref["T"], True, relax=ref["relax"])
            assert b.fallback_frames() == 0
        else:
            b.set_engine(engine)
            b.build()
            b.inference(ref["T"], True, relax=ref["relax"])
            assert b.locality_mode() == (False, False)
        assert b.engine() == engine, (name, engine, b.engine())
        n = pb["N"]
        assert cc.same_bits(b.probability()[0, :n], ref["trace"][ref["T"]]), (name, engine)
        assert np.array_equal(b.map()[0, :n], ref["map"]), (name, engine)
        assert [int(b.lattice_sizes(k)[0]) for k in range(2)] == ref["V"], (name, engine)
        if engine != 3:
            for k in range(2):
                assert cc.same_bits(b.norm(k)[0, :n], ref["norm"][k]), (name, engine, k)
        b.close()


def _frame_refs():
    """the references of fc.compare_batch for both SLAM frames and the empty frame, from the fixture"""
    out = []
    for name in tc.SLAM:
        pb, ref = _fixture(name)
        out.append(dict(N=pb["N"], Q=ref["trace"][ref["T"]], map=ref["map"], V=ref["V"]))
    out.append(dict(N=0, Q=np.zeros((0, 2), np.float32), map=np.zeros(0, np.int16), V=[0, 0]))
    return out


def _download(b):
    b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
    return dict(Q=b.probability(), map=b.map(), bits=b.wait_download()["bits"], V=[b.lattice_sizes(k) for k in range(2)])


def test_half_cu_grid_build_takes_both_frames(po):
    """point_record2_grid: 256 frames (the smallest batch the half-CU kernel takes), the two SLAM frames tiled.  The oracle's lattices
    say both fit the grid build (fc.expected_route), so no frame may leave for the fallback; every frame's Q, labels, label bits and
    lattice sizes are the reference record's."""
    pbs = [_fixture(n)[0] for n in tc.SLAM]
    assert [fc.expected_route(pb, po)[0] for pb in pbs] == ["fit", "fit"]
    which = [f % 2 for f in range(256)]
    T, relax = _fixture(tc.SLAM[0])[1]["T"], _fixture(tc.SLAM[0])[1]["relax"]
    b = cc.batch_of([pbs[w] for w in which], maxN=2048)
    b.run(T, True, relax=relax)
    assert b.engine() == 3 and b.fused_shape() == (512, 2), (b.engine(), b.fused_shape())
    assert b.fallback_frames() == 0
    fc.compare_batch(_download(b), _frame_refs(), which)
    b.close()


def test_ragged_batch_with_an_empty_frame_on_the_default_engine():
    pbs = [_fixture(tc.SLAM[0])[0], dict(_fixture(tc.SLAM[0])[0], N=0, label=np.zeros(0, np.int16),
                                         kernels=[(np.zeros((0, 2), np.float32), w) for _, w in _fixture(tc.SLAM[0])[0]["kernels"]]),
           _fixture(tc.SLAM[1])[0]]
    ref = _fixture(tc.SLAM[0])[1]
    b = cc.batch_of(pbs, maxN=2047)
    b.build()
    b.inference(ref["T"], True, relax=ref["relax"])
    print("ragged batch: engine", b.engine(), "shape", b.fused_shape())
    assert b.engine() in (1, 2) and b.locality_mode() == (False, False)
    fc.compare_batch(_download(b), _frame_refs(), [0, 2, 1])
    b.close()


@pytest.mark.parametrize("name", tc.SLAM)
def test_run_converged_on_a_fresh_handle(po, name):
    """lccrf_run_converged: build, normalisation and iterations until converged in one launch (engine 3), against the oracle's trace"""
    pb, _ = _fixture(name)
    for relax in (1.0, 0.5):
        tr = cv.oracle_trace(po, pb, relax)
        for crit, tol, cap in ((cv.LABELS, 0.0, cv.CAP), (cv.DELTA, 1e-2, cv.CAP), (cv.BOTH, 0.0, 2)):
            want = cv.expect(tr, crit, np.float32(tol), cap)
            h = cc.setup(pkg.DenseCRFHIP, pb)
            h.run_converged(cap, crit, tol, True, relax)
            m = h.map()
            assert h.engine() == (3, 0), (name, relax, h.engine())
            assert cv.same_report(h.convergence(), want), (name, relax, crit, h.convergence(), want)
            assert cc.same_bits(h.probability(), tr[want[0]]) and np.array_equal(m, cv.labels_of(tr[want[0]])), (name, relax, crit)
            h.close()


@pytest.mark.parametrize("name", tc.SLAM)
def test_frame_general_kernel_with_one_dense_matrix(po, name):
    """LCCRF_OPT_FRAME_GENERAL: a fresh frame with a label-compatibility matrix on term 0 in one launch (engine 3), against the float32
    restatement over the ORACLE's lattices (normalization_checker.restate_trace_f32)"""
    pb, _ = _fixture(name)
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    modes, mats = [nc.AFTER, nc.AFTER], [dense(2, 2)[0], None]
    w = nc.weights_f32(pb, nrm, modes)
    tr = nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, 5, 0.75, nrm)
    h = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, x) for (f, _), x in zip(pb["kernels"], w)]))
    h.set_pairwise_compatibility(0, mats[0])
    h.set_option(pkg.OPT_FRAME_GENERAL, 1)
    h.inference(5, True, 0.75)
    m = h.map()
    assert h.engine() == (3, 0), h.engine()
    assert cc.same_bits(h.probability(), tr[5]) and np.array_equal(m, cv.labels_of(tr[5])), name
    h.close()


# ---- locality mode: the sorted build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.BIG)
def test_locality_mode_at_the_threshold(po, name):
    """8192 points, a tenth of them tie points: inference() on a handle runs in locality mode (k_sort_cells orders the points by the
    cell they round to, k_points<D, true> feeds the sorted build), against the oracle.  The handle reports no build; a one-frame batch of
    the same inputs -- the same Engine under the same rule -- must report (internal point order, sorted build) and give the same bits."""
    pb = tc.problem(name)
    T, relax = 3, 0.75
    key = (name, "oracle")
    if key not in _REFS:
        o = cc.setup(po.OracleCRF, pb)
        o.inference_native(T, True, relax)
        _REFS[key] = (o.probability(), o.map(), o.kernel(0)["V"])
        o.close()
    q, m, V = _REFS[key]
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.inference(T, True, relax)
    assert h.engine()[0] == 1, h.engine()
    assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m), name
    h.close()
    f, w = pb["kernels"][0]
    b = pkg.BatchCRF(1, pb["N"], 2, [f.shape[1]], [float(w)])
    b.set_inputs_host([pb["N"]], [f[None]], unary=pb["unary"][None])
    b.build()
    mode = b.locality_mode()
    b.inference(T, True, relax=relax)
    print(name, "locality mode", mode, "->", b.locality_mode(), "splat plan", b.splat_plan(0))
    assert mode == (True, True) and b.locality_mode() == (True, True), (name, mode, b.locality_mode())
    assert b.engine() == 1 and int(b.lattice_sizes(0)[0]) == V
    assert cc.same_bits(b.probability()[0], q) and np.array_equal(b.map()[0], m), name
    b.close()

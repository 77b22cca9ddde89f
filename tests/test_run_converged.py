"""Convergence-driven inference on a fresh frame in ONE launch (include/lccrf.h sections 1i and 2f; notes/convergence.md):
lccrf_run_converged on handles, lccrf_batch_run_converged on batches, the kernel of csrc/frame_converge.hip and the late fallback
for frames it cannot take.

As in tests/test_converge.py every expectation comes from the oracle's trace Q_0 .. Q_cap and the contract restated in numpy float32
(tests/converge_cases.py: the traces are shared with that module, computed once); every comparison is exact -- the bits of Q, the
labels, the label bits, iterations, changed, converged and the bits of delta."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import batch_cases as bc
import converge_cases as cv
import crf_cases as cc
from abi_support import assert_declared_exported_bound, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
E_INVALID = -1
F32 = np.float32
SYMBOLS = ("lccrf_run_converged", "lccrf_batch_run_converged")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, SYMBOLS)
    assert lib.lccrf_abi_version() == 3                          # added without a step: callers probe by symbol
    for cls in (pkg.DenseCRFHIP, pkg.BatchCRF):
        assert hasattr(cls, "run_converged")
    for hdr in ("lccrf_densecrf.hpp", "lccrf_densecrf_gpu.hpp"):
        assert "void runConverged(" in open(os.path.join(ROOT, "include", hdr)).read(), hdr


def test_argument_checks_need_no_device(lib):
    """section 1h's checks come before the handle is looked at: with a NULL handle the error text names the argument"""
    assert_declared_exported_bound(lib, SYMBOLS)

    def err():
        return lib.lccrf_last_error().decode()
    bad = [((5, 0, 0.0, 1, 1.0), "criterion"), ((5, 4, 0.0, 1, 1.0), "criterion"), ((-1, 2, 0.0, 1, 1.0), "max_iterations"),
           ((5, 1, -1.0, 1, 1.0), "tol"), ((5, 1, float("nan"), 1, 1.0), "tol"), ((5, 1, float("inf"), 1, 1.0), "tol"),
           ((5, 2, 0.0, 1, float("nan")), "relax")]
    for args, word in bad:
        assert lib.lccrf_run_converged(None, *args) == E_INVALID and word in err(), (args, err())
        assert lib.lccrf_batch_run_converged(None, *args, None) == E_INVALID and word in err(), (args, err())
    for crit in (1, 2, 3):                                        # good arguments: the NULL handle is what is wrong
        assert lib.lccrf_run_converged(None, 5, crit, 0.0, 1, 1.0) == E_INVALID and "handle" in err()
        assert lib.lccrf_batch_run_converged(None, 0, crit, 1e-3, 0, 0.5, None) == E_INVALID and "handle" in err()


# ---- the cases ---------------------------------------------------------------------------------------------------------------
HANDLE_NAMES = ["N%d" % n for n in cv.SIZES] + ["N%d/appearance" % n for n in cv.SIZES]      # K = 2 and K = 1, every size


def _mid(tr):
    """(t, tol): a tol strictly between d_t and d_{t-1} that makes a mid-run iteration decide; frames of a point or two whose
    deltas never fall strictly keep the plain 1e-3 (the expectation is the oracle's either way)"""
    d = cv.deltas(tr)
    for t in range(3, cv.CAP):
        if d[t - 1] < d[t - 2]:
            return t, cv.mid_tol(tr, t)
    return None, F32(1e-3)


def handle_settings(tr):
    """[(criterion, tol, cap)]: DELTA, LABELS and both at a mid tol; DELTA at tol 0 under a short cap -- never met, the cap ends the
    run; and the mid tol with the cap AT its stop iteration -- met exactly at the cap, converged == 1"""
    _, mid = _mid(tr)
    out = [(cv.DELTA, mid, cv.CAP), (cv.LABELS, F32(0), cv.CAP), (cv.BOTH, mid, cv.CAP), (cv.DELTA, F32(0), 3)]
    stop = cv.expect(tr, cv.DELTA, mid, cv.CAP)
    if stop[3]:
        out.append((cv.DELTA, mid, stop[0]))
    return out


def test_the_handle_cases_decide_mid_run_at_the_cap_and_exactly_at_it(po, wl):
    """on the oracle's numbers alone: among the cases some stop mid-run, some are ended by the cap, some meet the criterion exactly
    at the cap -- in every points-per-lane class"""
    seen = {}
    for name in HANDLE_NAMES:
        ppt = max((cv.CASES[name][0] + cv.LANES - 1) // cv.LANES, 1)
        for relax in cv.RELAX:
            tr = cv.trace(po, wl, name, relax)
            for crit, tol, cap in handle_settings(tr):
                t, _, _, met = cv.expect(tr, crit, tol, cap)
                seen.setdefault(ppt, set()).add("mid" if t < cap else "met at the cap" if met else "cap")
    assert all(seen[p] == {"mid", "met at the cap", "cap"} for p in (1, 2, 3, 4)), seen


BATCH_NS = (0, 1, 64, 65, 700, 1025, 2000, 3000, 4096)
BATCH_SETTING = (cv.BOTH, F32(1e-3), 8, 1.0)                     # criterion, tol, cap, relax
OUTLIER_AT = 4


def _batch_frames(wl):
    """mixed sizes, the empty frame among them, and one frame whose lattices do not fit the one-launch plan (every point its own
    cell: tests/test_frame_engine.py::test_one_outlier_frame_costs_one_frame)"""
    probs = [wl.slam_problem(n, seed=60 + i) if n else cc.empty_problem(2, [2, 2]) for i, n in enumerate(BATCH_NS)]
    probs.insert(OUTLIER_AT, cc.shaped_problem(wl, 1200, "sparse", seed=5))
    return bc.Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]])


def _small_frames(wl, max_points):
    probs = [wl.slam_problem(300, seed=80), cc.empty_problem(2, [2, 2]), wl.slam_problem(64, seed=82)]
    return bc.Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]], max_points)


_BATCH_TRACES = {}


def _frame_traces(po, fr, relax, key):
    """the oracle's trace of every frame on the batch's own inputs (raw unaries, the batch's weights)"""
    if key not in _BATCH_TRACES:
        out = []
        for f, pb in enumerate(fr.probs):
            n = pb["N"]
            if n == 0:
                out.append(np.zeros((cv.CAP + 1, 0, fr.L), F32))
                continue
            one = dict(N=n, L=fr.L, unary=fr.U[f, :n], kernels=[(ft, fr.w[k]) for k, (ft, _) in enumerate(pb["kernels"])])
            out.append(cv.oracle_trace(po, one, relax))
        _BATCH_TRACES[key] = out
    return _BATCH_TRACES[key]


def test_batch_frames_stop_at_three_or_more_different_iterations(po, wl):
    crit, tol, cap, relax = BATCH_SETTING
    fr = _batch_frames(wl)
    assert len(fr.probs) <= 16
    wants = [cv.expect(tr, crit, tol, cap) for tr in _frame_traces(po, fr, relax, "mixed") if tr[0].shape[0]]
    assert len({w[0] for w in wants}) >= 3, wants


# ---- GPU, handles ------------------------------------------------------------------------------------------------------------
def _check(h, tr, crit, tol, cap, relax, want_engine, tag):
    want = cv.expect(tr, crit, tol, cap)
    h.run_converged(cap, crit, tol, True, relax)
    m = h.map()                                                   # right behind the call: the labels are taken as they arrive
    got = h.convergence()
    print(tag, "criterion", crit, "tol", tol, "cap", cap, "relax", relax, "->", got, "want", want, "engine", h.engine())
    assert h.engine() == want_engine, (tag, h.engine(), want_engine)
    assert cv.same_report(got, want), (tag, crit, tol, cap, relax, got, want)
    assert np.array_equal(m, cv.labels_of(tr[want[0]])), (tag, crit, tol, cap, relax)
    assert cc.same_bits(h.probability(), tr[want[0]]), (tag, crit, tol, cap, relax, want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", HANDLE_NAMES)
def test_fresh_handle_stops_where_the_oracle_does_in_one_launch(po, wl, name):
    h = cc.setup(pkg.DenseCRFHIP, cv.problem(wl, name))
    for relax in cv.RELAX:
        tr = cv.trace(po, wl, name, relax)
        for crit, tol, cap in handle_settings(tr):
            _check(h, tr, crit, tol, cap, relax, (3, 0), name)
    # the handle behind the call is as after lccrf_inference(h, t): stepping continues from Q_t ...
    relax = cv.RELAX[-1]
    tr = cv.trace(po, wl, name, relax)
    t = _check(h, tr, cv.LABELS, F32(0), cv.CAP - 1, relax, (3, 0), name)[0]
    h.step_inference(relax)
    assert cc.same_bits(h.probability(), tr[t + 1]), name
    # ... the fixed count t gives the same bits ...
    h.inference(t, True, relax)
    assert cc.same_bits(h.probability(), tr[t]) and np.array_equal(h.map(), cv.labels_of(tr[t])), name
    # ... and with its lattices built and sized (the step put them in HBM) the call goes straight to section 1h's engines
    h.run_converged(cv.CAP - 1, cv.LABELS, 0.0, True, relax)
    assert h.engine()[0] == 2 and cv.same_report(h.convergence(), cv.expect(tr, cv.LABELS, F32(0), cv.CAP - 1)), name
    assert cc.same_bits(h.probability(), tr[t]), name
    h.close()


@pytest.mark.gpu
def test_labels_arrive_behind_the_call_and_the_report_behind_them(po, wl, lib):
    """the C entry points themselves: lccrf_get_map directly behind lccrf_run_converged, then lccrf_get_convergence"""
    name, relax = "N1025", 1.0
    tr = cv.trace(po, wl, name, relax)
    N = cv.CASES[name][0]
    want = cv.expect(tr, cv.LABELS, F32(0), cv.CAP)
    assert want[3] == 1 and 1 < want[0] < cv.CAP
    h = cc.setup(pkg.DenseCRFHIP, cv.problem(wl, name))
    m = np.full(N, -7, np.int16)
    assert lib.lccrf_run_converged(h.h, cv.CAP, cv.LABELS, C.c_float(0.0), 1, C.c_float(relax)) == 0
    assert lib.lccrf_get_map(h.h, m.ctypes.data_as(C.POINTER(C.c_short))) == 0
    assert np.array_equal(m, cv.labels_of(tr[want[0]]))
    it, ch, co, d = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_float(-1)
    assert lib.lccrf_get_convergence(h.h, C.byref(it), C.byref(d), C.byref(ch), C.byref(co)) == 0
    assert cv.same_report(dict(iterations=it.value, delta=F32(d.value), changed=ch.value, converged=co.value), want)
    assert h.engine() == (3, 0)
    # without labels: Q alone, and the label array of the last run is not what the report is read from
    h.run_converged(2, cv.DELTA, 0.0, False, relax)
    assert cv.same_report(h.convergence(), cv.expect(tr, cv.DELTA, F32(0), 2)) and cc.same_bits(h.probability(), tr[2])
    h.close()


@pytest.mark.gpu
def test_trivial_frames_report_zeros(po, wl):
    zero = (0, F32(0), 0, 0)
    name = "N1000"
    tr = cv.trace(po, wl, name, 1.0)
    h = cc.setup(pkg.DenseCRFHIP, cv.problem(wl, name))
    h.run_converged(5, cv.LABELS, 0.0, True, 1.0)                 # something to overwrite
    assert h.convergence()["iterations"] > 0
    h.run_converged(0, cv.BOTH, 1e-3, True, 1.0)                  # max_iterations == 0: Q_0
    assert np.array_equal(h.map(), cv.labels_of(tr[0])) and cv.same_report(h.convergence(), zero) and h.engine() == (3, 0)
    assert cc.same_bits(h.probability(), tr[0])
    h.close()
    e = cc.setup(pkg.DenseCRFHIP, cc.empty_problem(2, [2, 2]))   # a handle of 0 points
    e.run_converged(5, cv.LABELS, 0.0, True, 1.0)
    assert cv.same_report(e.convergence(), zero) and e.map().size == 0
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,seed", [(1200, 5), (900, 6)])
def test_handle_whose_lattices_do_not_fit_is_re_run_like_its_twin(po, wl, N, seed):
    """every point its own lattice cell (tests/test_frame_engine.py::test_object_api_frame_that_does_not_fit_is_seen_through_the_
    label_array): the one-launch kernel flags the frame, the next synchronisation point re-runs it with section 1h's engines"""
    pb = cc.shaped_problem(wl, N, "sparse", seed=seed)
    tr = cv.oracle_trace(po, pb, 1.0)
    twin = cc.setup(pkg.DenseCRFHIP, pb)
    for crit, tol, cap in handle_settings(tr):
        want = cv.expect(tr, crit, tol, cap)
        ref = twin.inference_converged(cap, crit, tol, True, 1.0)
        h = cc.setup(pkg.DenseCRFHIP, pb)                         # fresh: nothing built, the call takes the one launch
        h.run_converged(cap, crit, tol, True, 1.0)
        m = h.map()
        got = h.convergence()
        print(N, crit, tol, cap, "->", got, "twin", ref, "want", want, "engines", h.engine(), twin.engine())
        assert got == ref and cv.same_report(got, want), (got, ref, want)
        assert np.array_equal(m, twin.map()) and np.array_equal(m, cv.labels_of(tr[want[0]]))
        assert cc.same_bits(h.probability(), twin.probability()) and cc.same_bits(h.probability(), tr[want[0]])
        assert h.engine() == twin.engine() and h.engine()[0] in (1, 2)       # what it was re-run on
        h.close()
    twin.close()


# ---- GPU, batches ------------------------------------------------------------------------------------------------------------
def _device_i32(addr, n):
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(n, np.int32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), C.c_size_t(4 * n), 2) == 0
    return out


def _outputs(b, F):
    """every output array of a settled batch"""
    b.synchronize()
    dev = b.device_convergence()                                  # complete behind lccrf_batch_synchronize
    out = dict(q=b.probability(), m=b.map(), rep=b.convergence(),
               dev={k: _device_i32(dev[k], F) for k in ("iterations", "delta", "changed", "converged")})
    b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
    out["bits"] = b.wait_download()["bits"].copy()
    return out


def _check_batch(out, fr, traces, crit, tol, cap, tag):
    wants = [cv.expect(tr, crit, tol, cap) for tr in traces]
    rep = out["rep"]
    print(tag, "iterations", rep["iterations"], "want", [w[0] for w in wants])
    assert all(len(v) == len(traces) for v in rep.values())
    for f, (tr, w) in enumerate(zip(traces, wants)):
        n = int(fr.N[f])
        got = {k: v[f] for k, v in rep.items()}
        assert cv.same_report(got, w), (tag, f, got, w)
        assert cc.same_bits(out["q"][f, :n], tr[w[0]]), (tag, f, w)
        assert np.array_equal(out["m"][f, :n], cv.labels_of(tr[w[0]])), (tag, f)
        # the label bits of a frame are those of ITS Q_t, and 0 beyond its points
        assert np.array_equal(out["bits"][f], cv.label_bits_of(tr[w[0]], out["bits"].shape[1])), (tag, f, w)
    assert np.array_equal(out["dev"]["iterations"], rep["iterations"]) and np.array_equal(out["dev"]["changed"], rep["changed"])
    assert np.array_equal(out["dev"]["delta"], rep["delta"].view(np.int32)) and np.array_equal(out["dev"]["converged"], rep["converged"])
    return wants


@pytest.mark.gpu
def test_batch_every_frame_stops_on_its_own_and_the_outlier_alone_is_re_run(po, wl):
    crit, tol, cap, relax = BATCH_SETTING
    fr = _batch_frames(wl)
    traces = _frame_traces(po, fr, relax, "mixed")
    b = fr.batch(build=False)                                     # inputs only
    b.run_converged(cap, crit, tol, True, relax)
    out = _outputs(b, len(traces))
    assert b.engine() == 3 and b.fallback_frames() == 1
    wants = _check_batch(out, fr, traces, crit, tol, cap, "mixed frames")
    assert wants[0] == (0, F32(0), 0, 0)                          # the empty frame
    assert len({w[0] for w in wants[1:]}) >= 3
    # the twin: lccrf_batch_build + lccrf_batch_inference_converged on a second batch with the same inputs
    b2 = fr.batch()
    b2.inference_converged(cap, crit, tol, True, relax)
    out2 = _outputs(b2, len(traces))
    for f, n in enumerate(fr.N):
        assert out["q"][f, :n].tobytes() == out2["q"][f, :n].tobytes() and out["m"][f, :n].tobytes() == out2["m"][f, :n].tobytes(), f
    assert out["bits"].tobytes() == out2["bits"].tobytes()
    for k in ("iterations", "delta", "changed", "converged"):
        assert out["rep"][k].tobytes() == out2["rep"][k].tobytes() and out["dev"][k].tobytes() == out2["dev"][k].tobytes(), k
    b2.close()
    # the same batch again with fewer and smaller frames: no stale bits, no stale reports
    small = _small_frames(wl, fr.maxN)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.run_converged(cap, cv.LABELS, 0.0, True, relax)
    out3 = _outputs(b, len(small.probs))
    assert b.engine() == 3 and b.fallback_frames() == 0
    _check_batch(out3, small, _frame_traces(po, small, relax, "small"), cv.LABELS, F32(0), cap, "three smaller frames")
    # ... and the fixed-count one-launch run on the same batch afterwards
    b.run(5, True, relax)
    b.synchronize()
    q = b.probability()
    for f, tr in enumerate(_frame_traces(po, small, relax, "small")):
        assert cc.same_bits(q[f, :small.N[f]], tr[5]), f
    assert b.engine() == 3
    b.close()


# ---- C++ ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_converged_exe(tmp_path_factory, po):
    """tests/cpp/run_converged_call_site_test.cpp: the tracker's sequence with DenseCRFHIP::runConverged, built as
    tests/test_cpp_adapter.py builds its programs"""
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    out = str(tmp_path_factory.mktemp("cpp_run_converged") / "run_converged_call_site_test")
    subprocess.run(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "run_converged_call_site_test.cpp"), "-o", out, pkg.LIB_PATH, po.ORACLE_SO,
                    "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-Wl,-rpath," + os.path.dirname(po.ORACLE_SO),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _write_inputs(path, wl, N, seed):
    fr = wl.slam_frame(N, seed)
    with open(path, "wb") as f:
        f.write(np.int32(N).tobytes())
        for a in (fr["obs"], fr["err"], fr["uv"], fr["init_label"]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_cpp_method_compiles_and_fails_loudly_without_gpu(run_converged_exe, wl, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = str(tmp_path / "in.bin")
    _write_inputs(p, wl, 64, 1)
    r = subprocess.run([run_converged_exe, p], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout     # throws; no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2000, 77])
def test_cpp_run_converged_call_site_matches_the_oracle(run_converged_exe, wl, tmp_path, N):
    p = str(tmp_path / "in.bin")
    _write_inputs(p, wl, N, 9)
    r = subprocess.run([run_converged_exe, p], capture_output=True, text=True)
    assert r.returncode == 0 and "RUN CONVERGED OK" in r.stdout, r.stdout + r.stderr

"""Convergence-driven inference (include/lccrf.h sections 1h and 2e; notes/convergence.md): lccrf_inference_converged on handles,
lccrf_batch_inference_converged on batches, the one-launch kernel of csrc/fused_converge.hip and the streaming fallback of
csrc/converge_track.hip.

Every expectation comes from the oracle's trace Q_0 .. Q_cap (OracleCRF.run_trace, confirmed against the reference's own code where
it is built) and the contract restated in numpy float32 (tests/converge_cases.py); every comparison is exact -- the bits of Q, the
labels, the label bits, iterations, changed, converged and the bits of delta.  The terms with a matrix or a normalisation mode take
their trace from tests/normalization_checker.py's float32 restatement, which the fused general kernel's tests hold to the bit.

CPU: the argument checks (no device needed), and that the cases are worth running -- per points-per-lane class and criterion one
case stops before its cap and one at it, the stop iterations spread, single points decide where the reach tests want them."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import converge_cases as cv
import crf_cases as cc
import normalization_checker as nc
from abi_support import assert_declared_exported_bound, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
E_INVALID, E_STATE = -1, -5
F32 = np.float32
NAMES = list(cv.CASES)
SYMBOLS = ("lccrf_inference_converged", "lccrf_get_convergence", "lccrf_batch_inference_converged",
           "lccrf_batch_get_convergence_host", "lccrf_batch_device_convergence")


@pytest.fixture(autouse=True)
def _entry_points(lib):
    """everything below is about these entry points: without them in the header, the library and the binding, every test fails"""
    assert_declared_exported_bound(lib, SYMBOLS)


def _shape(word):
    return word & 0xffff, (word >> 16) & 15, (word >> 20) & 1


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    src = assert_declared_exported_bound(lib, SYMBOLS)
    assert "LCCRF_STOP_DELTA" in src and "LCCRF_STOP_LABELS" in src
    assert lib.lccrf_abi_version() == 3                          # added without a step: callers probe by symbol
    assert (pkg.STOP_DELTA, pkg.STOP_LABELS) == (1, 2)
    for cls in (pkg.DenseCRFHIP, pkg.BatchCRF):
        assert hasattr(cls, "inference_converged") and hasattr(cls, "convergence")


def test_argument_checks_need_no_device(lib):
    """the checks of section 1h come before the handle is looked at: with a NULL handle the error text names the argument"""
    def err():
        return lib.lccrf_last_error().decode()
    bad = [((5, 0, 0.0, 1, 1.0), "criterion"), ((5, 4, 0.0, 1, 1.0), "criterion"), ((5, -1, 0.0, 1, 1.0), "criterion"),
           ((-1, 2, 0.0, 1, 1.0), "max_iterations"), ((5, 1, -1e-3, 1, 1.0), "tol"), ((5, 1, float("inf"), 1, 1.0), "tol"),
           ((5, 1, float("nan"), 1, 1.0), "tol"), ((5, 2, 0.0, 1, float("nan")), "relax"), ((5, 2, 0.0, 1, float("inf")), "relax")]
    for args, word in bad:
        assert lib.lccrf_inference_converged(None, *args) == E_INVALID and word in err(), (args, err())
        assert lib.lccrf_batch_inference_converged(None, *args, None) == E_INVALID and word in err(), (args, err())
    for crit in (1, 2, 3):                                        # good arguments: the NULL handle is what is wrong
        assert lib.lccrf_inference_converged(None, 5, crit, 0.0, 1, 1.0) == E_INVALID and "handle" in err()
        assert lib.lccrf_batch_inference_converged(None, 0, crit, 1e-3, 0, 0.5, None) == E_INVALID and "handle" in err()
    it = C.c_int(7)
    assert lib.lccrf_get_convergence(None, C.byref(it), None, None, None) == E_INVALID and it.value == 7
    assert lib.lccrf_batch_get_convergence_host(None, None, None, None, None) == E_INVALID
    assert lib.lccrf_batch_device_convergence(None, None, None, None, None) == E_INVALID


def test_the_restated_contract_on_a_hand_made_trace():
    q = lambda a, b: np.array([[a, 1 - a], [b, 1 - b]], F32)
    tr = [q(.5, .5), q(.75, .25), q(.875, .25), q(.875, .25), q(.875, .25)]
    assert cv.expect(tr, cv.DELTA, 0.0, 4) == (3, F32(0), 0, 1)
    assert cv.expect(tr, cv.DELTA, 0.125, 4) == (2, F32(.125), 0, 1)
    assert cv.expect(tr, cv.LABELS, 0.0, 4) == (2, F32(.125), 0, 1)           # t = 1: point 1 flips from the tie's label 0 to 1
    assert cv.expect(tr, cv.BOTH, 0.0, 2) == (2, F32(.125), 0, 0)             # the cap ended it
    assert cv.expect(tr, cv.DELTA, 0.25, 1) == (1, F32(.25), 1, 1)            # met exactly at the cap: converged
    assert cv.expect(tr, cv.DELTA, 0.0, 0) == (0, F32(0), 0, 0)
    assert cv.expect(tr, cv.DELTA, 0.1, 4, skip=0)[0] == 2 and cv.expect(tr, cv.DELTA, 0.1, 4)[0] == 3


def test_cases_stop_before_and_at_their_caps_in_every_class(po, wl):
    """on the oracle's numbers alone: a test that only ever hits the cap shows nothing"""
    early, at_cap, stops, shapes = set(), set(), set(), set()
    for name in NAMES:
        N = cv.CASES[name][0]
        ppt, ch = cv.want_shape(po, wl, name)
        shapes.add((len(cv.CASES[name][2]), ppt, ch))
        for relax in cv.RELAX:
            tr = cv.trace(po, wl, name, relax)
            for crit, tol, cap in cv.settings(tr, N):
                t, _, _, met = cv.expect(tr, crit, tol, cap)
                stops.add(t)
                if cap:
                    (early if t < cap else at_cap).add((ppt, crit))
    want = {(p, c) for p in (1, 2, 3, 4) for c in (cv.DELTA, cv.LABELS, cv.BOTH)}
    assert early >= want and at_cap >= want, (want - early, want - at_cap)
    assert len(stops) >= 4, stops
    assert shapes == {(k, p, ch) for k in (1, 2) for p in (1, 2, 3, 4) for ch in (0, 1)}, shapes    # k_converge's 16 instantiations


def test_the_oracle_traces_are_the_references(po, wl):
    if not po.have_ref():
        pytest.skip("the reference's shim is not built here")
    for name in ("N65", "N1025", "N2049/smooth_first"):
        for relax in cv.RELAX:
            assert cc.same_bits(cv.trace(po, wl, name, relax), cv.oracle_trace(po, cv.problem(wl, name), relax, cls=po.RefCRF)), name


_REACH = {}


def _reach(po, wl, N):
    """per target the seeds whose deciding point lands where intended: [(rolled problem, trace, t, point, tol)], and the seeds tried"""
    if N not in _REACH:
        out, seeds = {}, (0, 1)
        for seed in seeds:
            pb = wl.slam_problem(N, seed=seed)
            dec = cv.deciding(cv.oracle_trace(po, pb, 1.0))
            for tname, tgt in cv.targets(N).items():
                got = out.setdefault(tname, [])
                if dec is None:
                    continue
                pb2 = cv.rolled(pb, tgt - dec[1])
                tr2 = cv.oracle_trace(po, pb2, 1.0)               # rolling changes the bits: the expectation is the rolled input's
                d2 = cv.deciding(tr2)
                if d2 is not None and d2[1] == tgt:                # the precondition: the deciding point is where intended
                    got.append((pb2, tr2) + d2)
        _REACH[N] = (out, len(seeds))
    return _REACH[N]


@pytest.mark.parametrize("N", (700, 2500))
def test_single_points_decide_where_the_reach_tests_want_them(po, wl, N):
    cases, tried = _reach(po, wl, N)
    assert set(cases) == set(cv.targets(N))
    tg = cv.targets(N)
    ppt = (N + cv.LANES - 1) // cv.LANES
    assert tg["first wavefront"] < 64 and tg["index N-1"] == N - 1 and tg["last slot"] // cv.LANES == ppt - 1
    assert (tg["last wavefront with a point"] % cv.LANES) // 64 == (min(N, cv.LANES) - 1) // 64
    for tname, ok in cases.items():
        assert 2 * (tried - len(ok)) <= tried, (tname, len(ok), tried)       # at most half of the seeds tried may be skipped
        for pb2, tr2, t, point, tol in ok:
            assert point == tg[tname]
            assert cv.expect(tr2, cv.DELTA, tol, cv.CAP, skip=point)[0] == t < cv.expect(tr2, cv.DELTA, tol, cv.CAP)[0]


# ---- GPU, the kernel path ----------------------------------------------------------------------------------------------------
def _check(h, tr, crit, tol, cap, relax, want_engine, tag):
    want = cv.expect(tr, crit, tol, cap)
    got = h.inference_converged(cap, crit, tol, True, relax)
    print(tag, "criterion", crit, "tol", tol, "cap", cap, "relax", relax, "->", got, "want", want)
    assert h.engine() == want_engine, (tag, h.engine(), want_engine)
    assert cv.same_report(got, want), (tag, crit, tol, cap, relax, got, want)
    q = h.probability()
    assert cc.same_bits(q, tr[want[0]]), (tag, crit, tol, cap, relax, want)
    assert np.array_equal(h.map(), cv.labels_of(tr[want[0]])), (tag, crit, tol, cap, relax)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_handle_stops_where_the_oracle_does(po, wl, name):
    N = cv.CASES[name][0]
    ppt, ch = cv.want_shape(po, wl, name)
    word = 1024 | ppt << 16 | ch << 20
    h = cc.setup(pkg.DenseCRFHIP, cv.problem(wl, name))
    for relax in cv.RELAX:
        tr = cv.trace(po, wl, name, relax)
        for crit, tol, cap in cv.settings(tr, N):
            _check(h, tr, crit, tol, cap, relax, (2, word), name)
    assert _shape(h.engine()[1]) == (1024, ppt, ch)              # the chain bit as the launcher reports it, asserted not assumed
    h.close()


# The self-contained prologue (csrc/fused_prologue.inc: one text, included by k_converge as by k_fused and k_general) keeps a lattice's tables in registers between its loads and its LDS stores: the neighbour table
# of up to 4096 / 3 = 1365 vertices, the row pointers of up to 2047; what lies beyond is copied by two plain loops.  The SLAM frames
# above stay below both (the smooth term's lattice stops growing near 1180 vertices: the image has no more cells), so one frame with
# every point of its first term in a cell of its own (V = 3 N) is there for the loops: 683 points, the smallest with V > 2047.
LARGE_N, LARGE_V = 683, (1365, 2047)


def _vertices(po, pb):
    o = cc.setup(po.OracleCRF, pb)
    out = [o.kernel(k)["V"] for k in range(len(pb["kernels"]))]
    o.close()
    return out


def test_lattices_lie_on_both_sides_of_the_prologues_register_rounds(po, wl):
    assert all(max(_vertices(po, cv.problem(wl, name))) <= LARGE_V[0] for name in NAMES)
    V = _vertices(po, cc.shaped_problem(wl, LARGE_N, "sparse", 5))
    assert V[0] == 3 * LARGE_N > LARGE_V[1] >= 3 * (LARGE_N - 1) and V[1] <= LARGE_V[0], V


@pytest.mark.gpu
def test_handle_on_a_lattice_beyond_the_prologues_register_rounds(po, wl):
    pb = cc.shaped_problem(wl, LARGE_N, "sparse", 5)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for relax in cv.RELAX:
        tr = cv.oracle_trace(po, pb, relax, 2)
        for crit in (cv.DELTA, cv.LABELS):
            _check(h, tr, crit, F32(0), 2, relax, (2, 1024 | 1 << 16), "sparse:N%d" % LARGE_N)
    h.close()


def test_edge_frames_fill_the_plan_to_the_byte_and_96_bytes_short_of_it(po):
    for sites, want in ((cv.EDGE_FULL, cv.LDS_LIMIT), (cv.EDGE_ROOM, cv.LDS_LIMIT - 96)):
        pb = cv.edge_problem(sites)
        o = cc.setup(po.OracleCRF, pb)
        ks = [o.kernel(k) for k in range(2)]
        o.close()
        assert [k["V"] for k in ks] == [3 * m for m in sites]
        assert max(int(np.bincount(k["offset"].reshape(-1)).max()) for k in ks) == 2          # short rows: no chain path
        assert cv.edge_plan_bytes(cv.EDGE_N, [k["V"] for k in ks]) == want
    assert want + 16 <= cv.LDS_LIMIT < cv.edge_plan_bytes(cv.EDGE_N, [3 * m for m in cv.EDGE_FULL]) + 16


@pytest.mark.gpu
@pytest.mark.parametrize("sites,engine", [(cv.EDGE_FULL, 1), (cv.EDGE_ROOM, 2)], ids=["full", "room"])
def test_a_plan_without_room_for_the_reductions_words_streams(po, sites, engine):
    """the fused engine takes the frame (lccrf_inference: engine 2); k_converge takes it only with 16 bytes to spare -- without them
    its launcher returns 0 and the converged call runs on the streaming step (engine 1, shape word 0), with the same results"""
    pb = cv.edge_problem(sites)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for relax in cv.RELAX:
        tr = cv.oracle_trace(po, pb, relax)
        for crit, tol, cap in ((cv.LABELS, F32(0), cv.CAP), (cv.DELTA, F32(1e-3), cv.CAP), (cv.DELTA, F32(0), 2), (cv.LABELS, F32(0), 0)):
            _check(h, tr, crit, tol, cap, relax, (1, 0) if engine == 1 else (2, 1024 | 2 << 16), sites)
    h.inference(2, True, 1.0)                                     # the fixed count on the same lattices: the fused engine takes both
    assert h.engine() == (2, 1024 | 2 << 16) and cc.same_bits(h.probability(), cv.oracle_trace(po, pb, 1.0, 2)[2])
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", (700, 2500))
def test_one_point_decides_wherever_it_sits(po, wl, N):
    """tol lies between the largest and the second-largest per-point change at iteration t: a reduction that dropped the point --
    in the first wavefront, the last wavefront with a point, the last slot, at index N - 1 -- would stop at t, one too early"""
    cases, _ = _reach(po, wl, N)
    for tname, ok in cases.items():
        for pb2, tr2, t, point, tol in ok:
            h = cc.setup(pkg.DenseCRFHIP, pb2)
            want = _check(h, tr2, cv.DELTA, tol, cv.CAP, 1.0, (2, h_word(N, po, pb2)), "%s @%d" % (tname, point))
            assert want[0] > t
            h.close()


def h_word(N, po, pb):
    o = cc.setup(po.OracleCRF, pb)
    k0 = o.kernel(0)
    o.close()
    row0 = int(np.bincount(k0["offset"].reshape(-1), minlength=k0["V"]).max())
    return 1024 | ((N + 1023) // 1024) << 16 | int(row0 >= 64 and k0["V"] <= 464) << 20


@pytest.mark.gpu
def test_state_repeats_and_the_fixed_path_behind_a_converged_call(po, wl, lib):
    name, relax = "N1025", 1.0
    tr = cv.trace(po, wl, name, relax)
    h = cc.setup(pkg.DenseCRFHIP, cv.problem(wl, name))
    it = C.c_int(0)
    assert lib.lccrf_get_convergence(h.h, C.byref(it), None, None, None) == E_STATE       # nothing has run yet
    t, _, _, met = cv.expect(tr, cv.LABELS, 0.0, cv.CAP)
    assert met and 1 < t < cv.CAP - 1
    first = h.inference_converged(cv.CAP, cv.LABELS, 0.0, True, relax)
    assert first["iterations"] == t
    h.step_inference(relax)                                       # continues from Q_t as after lccrf_inference(h, t)
    assert cc.same_bits(h.probability(), tr[t + 1])
    # a second call, and one with another criterion in between: nothing stale in the per-frame arrays
    assert h.inference_converged(cv.CAP, cv.LABELS, 0.0, True, relax) == first
    other = h.inference_converged(cv.CAP, cv.DELTA, 0.0, False, relax)
    assert cv.same_report(other, cv.expect(tr, cv.DELTA, 0.0, cv.CAP)) and other != first
    assert h.inference_converged(cv.CAP, cv.LABELS, 0.0, True, relax) == first
    assert cc.same_bits(h.probability(), tr[t]) and np.array_equal(h.map(), cv.labels_of(tr[t]))
    # NULL outputs are fine, one at a time
    d = C.c_float(0)
    assert lib.lccrf_get_convergence(h.h, None, C.byref(d), None, None) == 0 and F32(d.value) == first["delta"]
    # the fixed path afterwards: the reference's bits, and its own engines
    h.inference(5, True, 1.0)
    assert cc.same_bits(h.probability(), tr[5]) and np.array_equal(h.map(), cv.labels_of(tr[5]))
    assert h.engine()[0] == 2 and _shape(h.engine()[1])[0] in (512, 1024)
    h.close()


# ---- GPU, batches ------------------------------------------------------------------------------------------------------------
BATCH_NS = (0, 1, 64, 700, 1025, 2000, 2049, 3000)
BATCH_SETTING = (cv.BOTH, F32(1e-3), 8, 1.0)                     # criterion, tol, cap, relax


def _frames(wl, Ns, first_seed, max_points=None):
    probs = [wl.slam_problem(n, seed=first_seed + i) if n else cc.empty_problem(2, [2, 2]) for i, n in enumerate(Ns)]
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


def _device_i32(addr, n):
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(n, np.int32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), C.c_size_t(4 * n), 2) == 0
    return out


def _check_batch(b, fr, traces, crit, tol, cap, want_engine, tag):
    wants = [cv.expect(tr, crit, tol, cap) for tr in traces]
    rep = b.convergence()
    print(tag, "iterations", rep["iterations"], "want", [w[0] for w in wants])
    assert b.engine() == want_engine, (tag, b.engine())
    q, m = b.probability(), b.map()
    for f, (tr, w) in enumerate(zip(traces, wants)):
        n = int(fr.N[f])
        got = {k: v[f] for k, v in rep.items()}
        assert cv.same_report(got, w), (tag, f, got, w)
        assert cc.same_bits(q[f, :n], tr[w[0]]), (tag, f, w)
        assert np.array_equal(m[f, :n], cv.labels_of(tr[w[0]])), (tag, f)
    dev = b.device_convergence()                                  # the same arrays where a caller on the device reads them
    F = len(traces)
    assert np.array_equal(_device_i32(dev["iterations"], F), rep["iterations"])
    assert np.array_equal(_device_i32(dev["delta"], F), rep["delta"].view(np.int32))
    assert np.array_equal(_device_i32(dev["changed"], F), rep["changed"])
    assert np.array_equal(_device_i32(dev["converged"], F), rep["converged"])
    if fr.L == 2:
        b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
        bits = b.wait_download()["bits"]
        for f, (tr, w) in enumerate(zip(traces, wants)):          # the label bits of a frame that stopped early are those of ITS Q_t
            assert np.array_equal(bits[f], cv.label_bits_of(tr[w[0]], bits.shape[1])), (tag, f, w)
    return wants


def test_batch_frames_stop_at_different_iterations_and_one_hits_the_cap(po, wl):
    crit, tol, cap, relax = BATCH_SETTING
    fr = _frames(wl, BATCH_NS, 20)
    wants = [cv.expect(tr, crit, tol, cap) for tr in _frame_traces(po, fr, relax, "eight")][1:]     # (frame 0 is empty)
    assert len({w[0] for w in wants}) >= 3 and any(w[3] == 0 and w[0] == cap for w in wants), wants
    assert any(w[3] == 1 and w[0] < cap for w in wants)


@pytest.mark.gpu
def test_batch_every_frame_stops_on_its_own(po, wl):
    import torch
    crit, tol, cap, relax = BATCH_SETTING
    fr = _frames(wl, BATCH_NS, 20)
    traces = _frame_traces(po, fr, relax, "eight")
    b = fr.batch()
    b.inference_converged(cap, crit, tol, True, relax)
    wants = _check_batch(b, fr, traces, crit, tol, cap, 2, "eight frames")
    assert wants[0] == (0, F32(0), 0, 0)                          # the empty frame
    # a caller's stream in place of the batch's
    s = torch.cuda.Stream()
    b.inference_converged(cap, cv.LABELS, 0.0, True, relax, stream=s.cuda_stream)
    _check_batch(b, fr, traces, cv.LABELS, 0.0, cap, 2, "caller's stream")
    # the same handle with fewer and smaller frames: nothing of the last batch shows
    small = _frames(wl, (300, 0, 64), 40, max_points=fr.maxN)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    assert pkg.lib().lccrf_batch_get_convergence_host(b.h, None, None, None, None) == E_STATE    # new inputs: nothing reported yet
    b.inference_converged(cap, crit, tol, True, relax)
    _check_batch(b, small, _frame_traces(po, small, relax, "three"), crit, tol, cap, 2, "three smaller frames")
    # ... and the fixed-count path on the same handle afterwards
    b.inference(5, True, relax)
    q = b.probability()
    for f, tr in enumerate(_frame_traces(po, small, relax, "three")):
        assert cc.same_bits(q[f, :small.N[f]], tr[5]), f
    assert b.engine() == 2
    b.close()


@pytest.mark.gpu
def test_batch_on_the_streaming_engine_gives_the_same_reports(po, wl):
    """lccrf_batch_set_engine(1): the fallback on frames the kernel path takes -- the restore of frames that finished early"""
    crit, tol, cap, relax = BATCH_SETTING
    fr = _frames(wl, BATCH_NS, 20)
    b = fr.batch(build=False)
    b.set_engine(1)
    b.build()
    b.inference_converged(cap, crit, tol, True, relax)
    _check_batch(b, fr, _frame_traces(po, fr, relax, "eight"), crit, tol, cap, 1, "eight frames, streaming")
    b.close()


# ---- GPU, the fallback -------------------------------------------------------------------------------------------------------
def _fallback_settings(tr):
    d = cv.deltas(tr)
    t = next(t for t in range(3, cv.CAP) if d[t - 1] < d[t - 2])
    return [(cv.DELTA, cv.mid_tol(tr, t), cv.CAP), (cv.LABELS, F32(0), cv.CAP), (cv.BOTH, cv.mid_tol(tr, t), cv.CAP),
            (cv.DELTA, F32(0), 2), (cv.LABELS, F32(0), 0)]


FALLBACK = {
    "L3:d2_d3:N200": lambda wl: wl.generic_problem(200, [2, 3], 3, seed=5),
    "slam:N5000": lambda wl: wl.slam_problem(5000, seed=1),
    "slam:N8192": lambda wl: wl.slam_problem(8192, seed=2),      # a handle of this size runs inference in locality mode
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FALLBACK))
def test_fallback_stops_where_the_oracle_does(po, wl, name):
    pb = FALLBACK[name](wl)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for relax in cv.RELAX:
        tr = cv.oracle_trace(po, pb, relax)
        stops = set()
        for crit, tol, cap in _fallback_settings(tr):
            stops.add(_check(h, tr, crit, tol, cap, relax, (1, 0), name)[0])
        assert len(stops) >= 3, stops
    h.step_inference(1.0)                                         # (cap 0 left Q_0) continues as after lccrf_inference(h, 0)
    assert cc.same_bits(h.probability(), cv.oracle_trace(po, pb, 1.0, 1)[1])
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ("matrix", "before"))
def test_fallback_with_a_matrix_or_a_normalisation_mode(po, wl, setting):
    """a two-label handle the fixed-count path runs on the fused general kernel: the converged call streams (engine 1).  The trace
    is the float32 restatement's, which steps exactly (tests/test_fused_general.py holds lccrf_inference to it bit for bit)."""
    pb = wl.slam_problem(700, seed=3)
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    rng = np.random.default_rng(77)
    mats = [(np.eye(2) + 0.3 * rng.standard_normal((2, 2))).astype(F32), None] if setting == "matrix" else [None, None]
    modes = [nc.AFTER, nc.AFTER] if setting == "matrix" else [nc.BEFORE, nc.AFTER]
    w = nc.weights_f32(pb, nrm, modes)
    h = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, x) for (f, _), x in zip(pb["kernels"], w)]))
    for k in range(2):
        h.set_normalization(k, modes[k])
        if mats[k] is not None:
            h.set_pairwise_compatibility(k, mats[k])
    for relax in cv.RELAX:
        tr = nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, cv.CAP, relax, nrm)
        for crit, tol, cap in _fallback_settings(tr):
            _check(h, tr, crit, tol, cap, relax, (1, 0), setting)
    h.inference(3, True, 1.0)                                     # the fixed-count path keeps its own kernel
    assert h.engine()[0] == 4
    h.close()


def test_three_label_batch_stops_at_different_iterations(po, wl):
    fr = bc.generic_frames(wl, Ns=(300, 77, 150, 250))
    wants = [cv.expect(tr, cv.LABELS, 0.0, cv.CAP) for tr in _frame_traces(po, fr, 1.0, "L3")]
    assert len({w[0] for w in wants}) >= 2, wants


@pytest.mark.gpu
def test_three_label_batch_on_the_fallback(po, wl):
    fr = bc.generic_frames(wl, Ns=(300, 77, 150, 250))
    b = fr.batch()
    for crit, tol in ((cv.LABELS, 0.0), (cv.DELTA, 1e-2)):
        b.inference_converged(cv.CAP, crit, tol, True, 1.0)
        _check_batch(b, fr, _frame_traces(po, fr, 1.0, "L3"), crit, F32(tol), cv.CAP, 1, "three labels")
    b.close()


# ---- C++ ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def converged_exe(tmp_path_factory, po):
    """tests/cpp/converged_call_site_test.cpp: the tracker's call site with DenseCRFHIP::inferenceConverged, built as
    tests/test_cpp_adapter.py builds its programs"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    out = str(tmp_path_factory.mktemp("cpp_converge") / "converged_call_site_test")
    subprocess.run(["g++", "-std=c++14", "-O2", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "converged_call_site_test.cpp"), "-o", out, pkg.LIB_PATH, po.ORACLE_SO,
                    "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-Wl,-rpath," + os.path.dirname(po.ORACLE_SO),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _write_inputs(path, wl, N, seed):
    fr = wl.slam_frame(N, seed)
    with open(path, "wb") as f:
        f.write(np.int32(N).tobytes())
        for a in (fr["obs"], fr["err"], fr["uv"], fr["init_label"]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_cpp_method_compiles_and_fails_loudly_without_gpu(converged_exe, wl, tmp_path):
    import subprocess
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = str(tmp_path / "in.bin")
    _write_inputs(p, wl, 64, 1)
    r = subprocess.run([converged_exe, p], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout     # throws; no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2000, 77])
def test_cpp_converged_call_site_matches_the_oracle(converged_exe, wl, tmp_path, N):
    import subprocess
    p = str(tmp_path / "in.bin")
    _write_inputs(p, wl, N, 9)
    r = subprocess.run([converged_exe, p], capture_output=True, text=True)
    assert r.returncode == 0 and "CONVERGED OK" in r.stdout, r.stdout + r.stderr

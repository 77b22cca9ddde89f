"""LCCRF_OPT_FRAME_GENERAL (include/lccrf.h): a fresh frame whose terms carry a label-compatibility matrix or a normalisation mode
runs lattice build, normalisation and inference in ONE launch (csrc/frame_general.hip: k_frame_general, k_frame_general_converge) on
lccrf_inference, lccrf_run_converged, lccrf_batch_run and lccrf_batch_run_converged.  notes/frame_general.md.

The reference of every frame is its restated float32 trace (normalization_checker.restate_trace_f32); the second witness is the same
batch or handle with the option off (engine 4 or 1).  Every comparison is exact: the bits of Q, the labels, the label bits, V and the
convergence reports.  The frames, settings, traces and checkers are those of tests/batch_general_cases.py, tests/converge_cases.py
and tests/test_batch_general.py (imported, not copied).  Before the option existed lccrf_set_option(5) was LCCRF_E_INVALID: every
GPU test here that sets it fails without the feature.

CPU: the frames reach both row routes, both points-per-lane classes and both term counts frame by frame; the sparse frame's model
shows in its trace.  GPU: the rest."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import batch_general_cases as bg
import compat_checker as ck
import converge_cases as cv
import crf_cases as cc
import normalization_checker as nc
import test_batch_general as tbg
import test_fused_general as fg
from abi_support import dev, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
F32 = np.float32
E_INVALID = -1
OPT = 5                                                           # LCCRF_OPT_FRAME_GENERAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERAL = tbg.GENERAL                                             # every setting but the Potts / AFTER one
SPARSE_SETTING = "mixed"                                          # a matrix and SYMMETRIC on term 0, BEFORE on term 1


def _make(bt, sname, on, **kw):
    """the batch with the setting applied, inputs only (nothing built), the option set or left at its default"""
    modes, mats, w = bg.setting(bt, sname)
    b = bg.make(bt, modes, mats, w, build=False, **kw)
    if on:
        b.set_option(OPT, 1)
    return b


def _same_outputs(b, twin, bt, tag, with_map=True):
    """bit for bit what the option-off twin holds: Q, labels, label bits, V"""
    q, q2 = b.probability(), twin.probability()
    for f, n in enumerate(bt.N):
        assert cc.same_bits(q[f, :n], q2[f, :n]), (tag, f)
    if with_map:
        m, m2 = b.map(), twin.map()
        for f, n in enumerate(bt.N):
            assert np.array_equal(m[f, :n], m2[f, :n]), (tag, f)
        bits = []
        for x in (b, twin):
            x.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
            bits.append(x.wait_download()["bits"].copy())
        assert np.array_equal(bits[0], bits[1]), tag
    for k in range(bt.K):
        assert np.array_equal(b.lattice_sizes(k)[:len(bt.N)], twin.lattice_sizes(k)[:len(bt.N)]), (tag, k)


def _check_q(b, bt, want_q, tag):
    q = b.probability()
    for f, want in enumerate(want_q):
        n = int(bt.N[f])
        assert cc.same_bits(q[f, :n], want), (tag, f, n)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_option_is_declared_next_to_the_others():
    hdr = open(os.path.join(ROOT, "include", "lccrf.h")).read()
    assert "LCCRF_OPT_FRAME_GENERAL    = 5" in hdr and "#define LCCRF_ABI_VERSION 3 " in hdr
    assert pkg.OPT_FRAME_GENERAL == pkg.BatchCRF.OPT_FRAME_GENERAL == OPT


def test_option_on_a_bad_handle_is_rejected_as_the_others_are(lib):
    for opt in (pkg.OPT_SINGLE_WORKGROUP, OPT):
        assert lib.lccrf_set_option(None, opt, 1) == E_INVALID and b"NULL" in lib.lccrf_last_error()
        assert lib.lccrf_batch_set_option(None, opt, 1) == E_INVALID and b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_set_default_option(6, 1) == E_INVALID


def test_frames_reach_both_row_routes_frame_by_frame(po, wl, golden):
    """The frame kernel decides kernel 0's route per frame (csrc/fused_loop.h: chain_wanted -- the longest row of ITS kernel 0 has at
    least 64 products and that lattice at most 464 vertices), and the launch its points per lane from the batch's largest frame: over
    the batches every (terms, points per lane, chain rows) occurs, short-row and chain-row frames inside one launch among them."""
    seen, mixed = set(), 0
    for name, (frames, order) in bg.BATCHES.items():
        bt = bg.batch(name, golden, po, wl)
        ppt = bt.shape()[1]
        routes = set()
        for fn in frames:
            if fn == bg.EMPTY:
                continue
            _, _, _, v, r = bg.base(fn, golden, po, wl)
            k0 = bg.ORDERS[order][0]
            routes.add(int(r[k0] >= 64 and v[k0] <= 464))
        seen |= {(bt.K, ppt, ch) for ch in routes}
        mixed += routes == {0, 1}
    assert seen == {(k, p, ch) for k in (1, 2) for p in (1, 2) for ch in (0, 1)}, seen
    assert mixed >= 2, mixed
    assert {int(n) for n in bg.batch("two/", golden, po, wl).N} == {5, 7, 1001, 1024, 0, 1025, 2000, 2048}


def test_the_sparse_frames_model_shows_in_its_trace(po, wl, golden):
    """a re-run that forgot the matrix or the modes cannot match: the sparse frame's restated Q differs between the model and Potts"""
    for name in bg.SPARSE:
        bt = bg.batch(name, golden, po, wl)
        modes, mats, w = bg.setting(bt, SPARSE_SETTING)
        assert any(m is not None and not np.array_equal(m, np.eye(2)) for m in mats) and any(m != nc.AFTER for m in modes)
        with_model = bg.traces(bt, SPARSE_SETTING, 1.0, 5)[0][5]
        potts = bg.traces(bt, "after", 1.0, 5, weights=w)[0][5]
        assert with_model.shape == potts.shape and not cc.same_bits(with_model, potts), name
        assert not np.array_equal(ck.map_of(with_model), ck.map_of(potts)) or np.abs(with_model - potts).max() > 1e-3, name


# ---- GPU: batches --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sname", GENERAL)
@pytest.mark.parametrize("bname", list(bg.BATCHES))
def test_batch_run_is_one_launch_and_every_frames_restatement(po, wl, golden, bname, sname):
    bt = bg.batch(bname, golden, po, wl)
    b, twin = _make(bt, sname, True), _make(bt, sname, False)
    for relax in (1.0, 0.7):
        trs = bg.traces(bt, sname, relax, 5)
        for T, with_map in ((0, True), (5, True), (5, False), (1, True)):
            tag = (bname, sname, T, relax, with_map)
            b.run(T, with_map, relax)
            twin.run(T, with_map, relax)
            if with_map:
                bg.check_frames(b, bt, [tr[T] for tr in trs], tag)
            else:
                _check_q(b, bt, [tr[T] for tr in trs], tag)
            assert b.engine() == 3 and b.fallback_frames() == 0 and b.fused_shape() == (1024, 1), (tag, b.engine(), b.fused_shape())
            assert twin.engine() == 4 and twin.fallback_frames() == 0, (tag, twin.engine())     # the route does not leak
            _same_outputs(b, twin, bt, tag, with_map)
    b.close(), twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bname,sname,relax", bg.CONVERGED)
def test_batch_run_converged_is_one_launch_and_stops_frame_by_frame(po, wl, golden, bname, sname, relax):
    bt = bg.batch(bname, golden, po, wl)
    trs = bg.traces(bt, sname, relax)
    b, twin = _make(bt, sname, True), _make(bt, sname, False)
    settings = bg.converged_settings(trs, bg.DESIGNATED[bname.split("/")[0]]) + [(cv.DELTA, F32(0), 2)]    # tol 0: the cap ends it
    for crit, tol, cap in settings:
        tag = (bname, sname, relax, crit, float(tol), cap)
        b.run_converged(cap, crit, tol, True, relax)
        tbg._check_converged(b, bt, trs, crit, tol, cap, 3, tag)
        assert b.fallback_frames() == 0 and b.fused_shape() == (1024, 1), tag
        twin.run_converged(cap, crit, tol, True, relax)
        assert twin.engine() == 4, (tag, twin.engine())
        r1, r2 = b.convergence(), twin.convergence()
        assert all(np.array_equal(r1[k].view(np.int32), r2[k].view(np.int32)) for k in r1), tag
        _same_outputs(b, twin, bt, tag)
    crit, tol, cap = settings[0]                                  # without labels: Q and the report alone
    b.run_converged(cap, crit, tol, False, relax)
    wants = [cv.expect(tr, crit, tol, cap) for tr in trs]
    _check_q(b, bt, [tr[w[0]] for tr, w in zip(trs, wants)], (bname, sname, "no map"))
    rep = b.convergence()
    assert all(cv.same_report({k: v[f] for k, v in rep.items()}, w) for f, w in enumerate(wants)) and b.engine() == 3
    b.run(3, True, relax)                                         # the fixed count behind a converged run
    bg.check_frames(b, bt, [tr[3] for tr in trs], (bname, sname, "fixed behind converged"))
    assert b.engine() == 3
    b.close(), twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bname", list(bg.SPARSE))
def test_a_frame_beyond_the_kernels_lds_is_re_run_with_the_model(po, wl, golden, bname):
    """the sparse frame (every point a lattice cell of its own: 3300 vertices) does not fit the frame kernel's build; it alone is
    re-run in the sub-engine, with the matrices and modes of the run -- and with the next run's when they have changed since"""
    bt = bg.batch(bname, golden, po, wl)
    b = _make(bt, SPARSE_SETTING, True)
    for sname, relax in ((SPARSE_SETTING, 1.0), ("matrices", 0.7), ("symmetric", 1.0), (SPARSE_SETTING, 0.7)):
        modes, mats, w = bg.setting(bt, sname)
        bg.apply(b, modes, mats)
        for k, x in enumerate(w):
            b.set_pairwise_weight(k, float(x))
        trs = bg.traces(bt, sname, relax, 5)
        b.run(5, True, relax)
        bg.check_frames(b, bt, [tr[5] for tr in trs], (bname, sname, relax))
        assert b.engine() == 3 and b.fallback_frames() == 1, (sname, b.engine(), b.fallback_frames())
    modes, mats, w = bg.setting(bt, SPARSE_SETTING)
    trs = bg.traces(bt, SPARSE_SETTING, 0.5)
    for crit, tol, cap in ((cv.LABELS, F32(0), bg.CAP), (cv.DELTA, F32(1e-2), 4)):
        b.run_converged(cap, crit, tol, True, 0.5)
        tbg._check_converged(b, bt, trs, crit, tol, cap, 3, (bname, "converged", crit))
        assert b.fallback_frames() == 1
    b.close()


# ---- GPU: handles ----------------------------------------------------------------------------------------------------------------
HANDLES = [n for n, want in fg.CASES.items() if want is not None] + ["N1024"]
_HANDLE_TRACES = {}


def _handle_case(name, sname, relax, golden, po, wl):
    """(problem, raw unary, weights, modes, matrices, restated trace Q_0 .. Q_CAP): computed once, never changed"""
    key = (name, sname, relax)
    if key not in _HANDLE_TRACES:
        pb, U, nrm, _ = fg._prepared(name, golden, po, wl)
        modes, mats = fg._settings(len(pb["kernels"]))[sname]
        w = nc.weights_f32(pb, nrm, modes)
        tr = nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, bg.CAP, relax, nrm)
        for q in tr:
            q.setflags(write=False)
        _HANDLE_TRACES[key] = (pb, U, w, modes, mats, tr)
    return _HANDLE_TRACES[key]


def _walk_handle(h, tr, relax, tag):
    """inference and run_converged on the fresh handle in one launch, the labels read right behind each call; then, with the
    lattices in HBM behind a step, the same calls on the option-off engines with the same bits"""
    h.inference(5, True, relax)
    m = h.map()                                                   # label by label, as they arrive
    assert h.engine() == (3, 0), (tag, h.engine())
    assert np.array_equal(m, ck.map_of(tr[5])) and cc.same_bits(h.probability(), tr[5]), tag
    h.inference(0, False, relax)
    assert h.engine() == (3, 0) and cc.same_bits(h.probability(), tr[0]), tag
    for crit, tol, cap in ((cv.LABELS, F32(0), bg.CAP), (cv.DELTA, F32(1e-2), bg.CAP), (cv.BOTH, F32(0), 2), (cv.LABELS, F32(0), 0)):
        want = cv.expect(tr, crit, tol, cap)
        h.run_converged(cap, crit, tol, True, relax)
        m = h.map()
        got = h.convergence()
        assert h.engine() == (3, 0), (tag, h.engine())
        assert cv.same_report(got, want), (tag, crit, cap, got, want)
        assert np.array_equal(m, cv.labels_of(tr[want[0]])) and cc.same_bits(h.probability(), tr[want[0]]), (tag, crit, cap)
    t = cv.expect(tr, cv.LABELS, F32(0), bg.CAP - 1)[0]
    h.run_converged(bg.CAP - 1, cv.LABELS, 0.0, True, relax)
    h.step_inference(relax)                                       # the lattices go to HBM: stepping continues from Q_t
    assert cc.same_bits(h.probability(), tr[t + 1]), tag
    h.inference(5, True, relax)
    assert h.engine()[0] == 4 and cc.same_bits(h.probability(), tr[5]) and np.array_equal(h.map(), ck.map_of(tr[5])), (tag, h.engine())
    h.run_converged(bg.CAP, cv.LABELS, 0.0, True, relax)
    want = cv.expect(tr, cv.LABELS, F32(0), bg.CAP)
    assert h.engine()[0] in (1, 4) and cv.same_report(h.convergence(), want) and cc.same_bits(h.probability(), tr[want[0]]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", HANDLES)
def test_fresh_handle_runs_its_model_in_one_launch(po, wl, golden, name):
    """unaries from labels (the tracker's call) and the same frame from raw unaries"""
    cases = [("mixed", 1.0), ("matrices", 0.7)] if name != "c2" else [(s, 1.0) for s in GENERAL] + [("mixed", 0.7)]
    for i, (sname, relax) in enumerate(cases):
        pb, U, w, modes, mats, tr = _handle_case(name, sname, relax, golden, po, wl)
        for raw in (False, True) if i == 0 else (False,):
            one = dict(pb, unary=U) if raw else pb
            if raw:
                one = {k: v for k, v in one.items() if k not in ("label", "conf")}
            h = fg._handle(one, w, modes, mats)
            h.set_option(OPT, 1)
            _walk_handle(h, tr, relax, (name, sname, relax, raw))
            h.close()
            if "unary" in pb:                                     # (a case that comes with raw unaries has no labels to derive them from)
                break


@pytest.mark.gpu
@pytest.mark.parametrize("N", (7, 1001, 1025, 2000))
def test_fresh_handle_with_unknown_labels(po, wl, N):
    """the label -1 takes the uniform energy (densecrf3d.h:116-129): derived in the kernel as the oracle derives it"""
    pb = wl.slam_problem(N, seed=31)
    label = np.array(pb["label"], np.int16).copy()
    label[::5], label[3::7] = -1, -1
    pb = dict(pb, label=label)
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    modes, mats = fg._settings(2)["mixed"]
    w = nc.weights_f32(pb, nrm, modes)
    tr = nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, bg.CAP, 1.0, nrm)
    h = fg._handle(pb, w, modes, mats)
    h.set_option(OPT, 1)
    _walk_handle(h, tr, 1.0, ("unknown labels", N))
    h.close()


@pytest.mark.gpu
def test_handle_whose_lattices_do_not_fit_is_re_run_with_its_model(po, wl, golden):
    pb, U, w, modes, mats, tr = _handle_case("sparse:N1100", "mixed", 1.0, golden, po, wl)
    h = fg._handle(pb, w, modes, mats)
    h.set_option(OPT, 1)
    h.inference(5, True, 1.0)
    m = h.map()
    assert np.array_equal(m, ck.map_of(tr[5])) and cc.same_bits(h.probability(), tr[5])
    assert h.engine()[0] in (1, 4), h.engine()                    # what it was re-run on
    h.close()
    h = fg._handle(pb, w, modes, mats)
    h.set_option(OPT, 1)
    want = cv.expect(tr, cv.LABELS, F32(0), bg.CAP)
    h.run_converged(bg.CAP, cv.LABELS, 0.0, True, 1.0)
    m = h.map()
    assert cv.same_report(h.convergence(), want) and np.array_equal(m, cv.labels_of(tr[want[0]]))
    assert cc.same_bits(h.probability(), tr[want[0]]) and h.engine()[0] in (1, 4), h.engine()
    h.close()


# ---- GPU: routing edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F,names", [(256, ("c2", "N2048", "N1025", "N1024")), (256, ("N7", "slam:N1001", "N1024")), (3, ("c2", "N7")),
                                     (1, ("c2",))])
def test_a_potts_batch_keeps_its_route_and_shape(po, wl, golden, F, names):
    """the lean shape (256 full-size frames), the small shape (256 frames of up to 1024 points), the two-workgroup form (a few
    frames) and a single frame: with the option on a Potts / AFTER batch launches what it launches with the option off"""
    bt = bg.Batch("potts route " + "+".join(names), names, "", golden, po, wl)
    n, feats, unary = bt.inputs()
    idx = np.arange(F) % len(names)
    seen = []
    for on in (False, True):
        b = pkg.BatchCRF(F, bt.maxN, 2, [2, 2], [float(x) for x in bt.w0])
        if on:
            b.set_option(OPT, 1)
        b.set_inputs_host(n[idx], [f[idx] for f in feats], unary=unary[idx])
        b.run(5, True, 1.0)
        q = b.probability()
        seen.append((b.engine(), b.fused_shape(), b.fallback_frames(), q.tobytes()))
        for f in range(min(F, len(names))):
            assert cc.same_bits(q[f, :n[idx][f]], bg.traces(bt, "after", 1.0, 5)[f][5]), (on, f)
        b.run_converged(4, cv.LABELS, 0.0, True, 1.0)
        seen[-1] += (b.engine(), b.fused_shape(), b.probability().tobytes())
        b.close()
    assert seen[0] == seen[1] and seen[0][0] == 3, (seen[0][:3], seen[1][:3])


@pytest.mark.gpu
def test_a_2049_point_frame_with_a_matrix_is_not_taken(po, wl, golden):
    bt = bg.Batch("big", ("N7", bg.EMPTY, "N2049"), "", golden, po, wl)
    out = []
    for on in (False, True):
        b = _make(bt, "mixed", on)
        b.run(5, True, 1.0)
        bg.check_frames(b, bt, [tr[5] for tr in bg.traces(bt, "mixed", 1.0, 5)], ("2049", on))
        out.append((b.engine(), b.fallback_frames(), b.probability().tobytes()))
        b.close()
    assert out[0] == out[1] and out[0][0] in (1, 4), (out[0][:2], out[1][:2])


@pytest.mark.gpu
def test_a_three_label_handle_with_a_matrix_is_not_taken(po, wl, golden):
    pb = cc.golden_problem(golden, "generic:d1_L3")
    K, L = len(pb["kernels"]), pb["L"]
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(K)]
    o.close()
    mats, modes = fg._dense(K, L), [nc.AFTER] * K
    w = nc.weights_f32(pb, nrm, modes)
    ref = nc.restate_f32(U, nc.feats(pb), w, mats, modes, 5, 1.0, nrm)
    h = fg._handle(pb, w, modes, mats)
    h.set_option(OPT, 1)
    h.inference(5, True, 1.0)
    assert h.engine()[0] == 1 and cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref)), h.engine()
    h.close()


@pytest.mark.gpu
def test_the_model_changes_between_runs_on_the_same_inputs(po, wl, golden):
    bt = bg.batch("two/", golden, po, wl)
    w = [F32(x) for x in bt.w0]
    b = bg.make(bt, [nc.AFTER] * 2, [None] * 2, w, build=False)
    b.set_option(OPT, 1)
    mats = fg._dense(2, 2)
    models = [([nc.AFTER, nc.AFTER], [mats[0], None]), ([nc.AFTER, nc.SYMMETRIC], [mats[0], None]),
              ([nc.BEFORE, nc.SYMMETRIC], [mats[1], mats[0]]), ([nc.AFTER, nc.AFTER], [None, None])]
    b.run(5, True, 0.7)
    potts_q, potts_shape = b.probability(), b.fused_shape()
    assert b.engine() == 3
    for modes, ms in models:
        bg.apply(b, modes, ms)
        b.run(5, True, 0.7)
        want = [nc.restate_f32(fr[1], fr[2], w, ms, modes, 5, 0.7, fr[3]) if fr else np.zeros((0, 2), F32) for fr in bt.frames]
        bg.check_frames(b, bt, want, ("model", modes))
        assert b.engine() == 3 and b.fallback_frames() == 0
    assert cc.same_bits(b.probability(), potts_q) and b.fused_shape() == potts_shape      # cleared: the Potts one-launch run again
    b.close()


# ---- GPU: the option's plumbing ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_default_option_reaches_new_handles_and_batches_and_a_recycled_handle_starts_from_it(po, wl, golden, lib):
    pb, U, w, modes, mats, tr = _handle_case("c2", "mixed", 1.0, golden, po, wl)
    bt = bg.batch("one/", golden, po, wl)

    def engines():
        h = fg._handle(pb, w, modes, mats)
        h.inference(5, True, 1.0)
        assert cc.same_bits(h.probability(), tr[5])
        e = h.engine()[0]
        h.close()
        b = _make(bt, "mixed", False)
        b.run(5, True, 1.0)
        bg.check_frames(b, bt, [t[5] for t in bg.traces(bt, "mixed", 1.0, 5)], "default option")
        eb = b.engine()
        b.close()
        return e, eb

    assert engines() == (4, 4)
    for bad in (0, 6, 99):
        assert lib.lccrf_set_default_option(bad, 1) == E_INVALID
    try:
        pkg.set_default_option(OPT, 1)
        assert engines() == (3, 3)
    finally:
        pkg.set_default_option(OPT, 0)
    assert engines() == (4, 4)
    # a handle that set the option itself, destroyed and handed out again from the cache: the default (off) again
    h = fg._handle(pb, w, modes, mats)
    h.set_option(OPT, 1)
    h.inference(5, True, 1.0)
    assert h.engine()[0] == 3
    h.close()
    assert engines() == (4, 4)


# ---- GPU: gradients behind a one-launch run ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gradients_after_a_one_launch_run_are_those_after_the_two_kernel_run(po, wl, golden):
    import torch
    bt = bg.Batch("two frames", ("N7", "N1025"), "", golden, po, wl)
    F, K, T = len(bt.frames), bt.K, 3
    G = dev(np.random.default_rng(9).standard_normal((F, bt.maxN, 2)).astype(F32))
    outs = []
    for on in (True, False):
        b = _make(bt, "mixed", on)
        b.run(T, True, 0.7)
        assert b.engine() == (3 if on else 4)
        gu, gw = dev(np.full((F, bt.maxN, 2), np.nan, F32)), dev(np.full((F, K), np.nan, F32))
        gc, gm = dev(np.full((F, K, 2, 2), np.nan, F32)), dev(np.full(K + K * 4, np.nan, F32))
        b.inference_backward_all_device(T, 0.7, G.data_ptr(), gu.data_ptr(), gw.data_ptr(), None, gc.data_ptr(), gm.data_ptr())
        b.synchronize()
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy().copy() for x in (gu, gw, gc, gm)])
        b.close()
    for a, c in zip(*outs):
        assert np.isfinite(a).any() and a.tobytes() == c.tobytes()
    assert np.isfinite(outs[0][1]).all() and np.isfinite(outs[0][3]).all() and np.abs(outs[0][3]).max() > 0


# ---- C++ -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/frame_general_call_site_test.cpp, built as tests/test_run_converged.py builds its program"""
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    out = str(tmp_path_factory.mktemp("cpp_frame_general") / "frame_general_call_site_test")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "frame_general_call_site_test.cpp"), "-o", out, pkg.LIB_PATH,
                    "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _inputs(path, wl, N, seed):
    pb = wl.slam_problem(N, seed=seed)
    fr, mu = pb["frame"], fg._dense(2, 2)[0]
    with open(path, "wb") as f:
        f.write(np.int32(N).tobytes())
        for a in (fr["obs"], fr["err"], fr["uv"], fr["init_label"], mu):
            f.write(np.ascontiguousarray(a).tobytes())
    return pb, mu


def test_cpp_program_compiles_and_fails_loudly_without_a_gpu(exe, wl, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _inputs(src, wl, 64, 1)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout, r.stdout + r.stderr      # throws; no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2000, 77])
def test_cpp_call_site_runs_the_learnt_model_in_one_launch(exe, po, wl, tmp_path, N):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    pb, mu = _inputs(src, wl, N, 9)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and "FRAME GENERAL CALL-SITE DONE" in r.stdout, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    q = np.frombuffer(raw, np.float32, 2 * N, 0).reshape(N, 2)
    labels = np.frombuffer(raw, np.int16, N, 8 * N)
    engine, iterations, changed, converged = np.frombuffer(raw, np.int32, 4, 10 * N)
    delta = np.frombuffer(raw, np.float32, 1, 10 * N + 16)[0]
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    modes = [nc.AFTER, nc.SYMMETRIC]
    tr = nc.restate_trace_f32(U, nc.feats(pb), nc.weights_f32(pb, nrm, modes), [mu, None], modes, bg.CAP, 1.0, nrm)
    want = cv.expect(tr, cv.LABELS, F32(0), bg.CAP)
    assert engine == 3, (engine, r.stdout)
    assert cv.same_report(dict(iterations=iterations, delta=delta, changed=changed, converged=converged), want), (r.stdout, want)
    assert cc.same_bits(q, tr[want[0]]) and np.array_equal(labels, cv.labels_of(tr[want[0]]))

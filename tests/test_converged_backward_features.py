"""Feature gradients of a batch's converged inference, each frame at its own iteration count (include/lccrf.h section 2l:
lccrf_batch_inference_backward_modes_converged; notes/convergence.md section 8), on the streaming sweep and on the one-launch kernel
(LCCRF_OPT_FUSED_BACKWARD_FEATURES).  Every comparison is bit for bit (cc.same_bits): per frame against a handle holding that frame --
lccrf_inference_backward_modes at t_f --, against section 2i's fixed-count call where the counts are equal, against section 2k's and
2j's calls without a feature array, and d_grad_model against the restated ordered sum.  Then the frames whose count is 0 behind a call
that left its accumulators in the area, a real converged run whose device report goes straight into the call, the float64 checkers
under the existing bars, the refusals and the torch layers."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import batch_learned_cases as bl
import converge_cases as cv
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import joint_checker as jc
import mode_feature_checker as mc
import normalization_checker as nc
import test_converged_backward_learnt as tl
from abi_support import dev, hip_malloc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT = pkg.OPT_FUSED_BACKWARD_FEATURES
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
E_INVALID, E_STATE = -1, -5
NS, CAP, COUNTS = tl.NS, tl.CAP, tl.COUNTS                        # (0, 5, 7, 64, 257, 1000, 1025, 2048) at (3, 0, 1, 5, 2, 5, 9, -1), cap 5
RELAX_SET = [1.0, 0.7]
MODELS = list(bl.SETTINGS) + ["one_term", "one_term_after"]       # after (Potts), before, symmetric, none, matrices, mixed; K = 1 twice
ONE_LAUNCH = ("after", "one_term_after")                          # Potts terms normalised AFTER: what section 1l's kernel takes
FULL = dict(compat=True, model=True)                              # every output: the compat form, which always streams
PLAIN = dict(compat=False, model=False)                           # neither dL/dmu nor the sums: section 1l's form


def _frames(golden, wl, model, Ns=NS):
    return tl._frames(golden, wl, "one_term" if model.startswith("one_term") else model, Ns)


def _model(fr, model, po):
    return bl.setting(fr, "after", po) if model == "one_term_after" else tl._model(fr, model, po)


def _call(b, fr, on, cap, relax, counts, G, unary=True, weights=True, features=True, skip=(), compat=True, model=True, stream=None,
          it_ptr=None):
    """one call with the option on / off, every output pre-filled with NaN: dict(gu, gw, gf, gm, model, q, route); an output that is not
    asked for (a NULL pointer; features: None for a NULL array, `skip` for NULL entries) comes back as filled"""
    import torch
    F, K, L = len(fr.N), fr.K, fr.L
    b.set_option(OPT, 1 if on else 0)
    it = dev(np.asarray(counts, np.int32))
    g = dev(np.ascontiguousarray(G, np.float32))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, max(K, 1)), nan(F, max(K, 1), L, L), nan(max(K, 1) * (1 + L * L))
    gf = [nan(F, fr.maxN, d) for d in fr.dims]
    torch.cuda.synchronize()
    b.inference_backward_modes_converged_device(cap, relax, it.data_ptr() if it_ptr is None else it_ptr, g.data_ptr(),
                                                gu.data_ptr() if unary else None, gw.data_ptr() if weights and K else None,
                                                [None if k in skip else t.data_ptr() for k, t in enumerate(gf)] if features else None,
                                                gm.data_ptr() if compat and K else None, md.data_ptr() if model and K else None,
                                                stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return dict(gu=gu.cpu().numpy(), gw=gw[:, :K].cpu().numpy(), gm=gm[:, :K].cpu().numpy(), gf=[t.cpu().numpy() for t in gf],
                model=md[:K * (1 + L * L)].cpu().numpy(), q=b.probability(), route=b.backward_route())


def _handle_results(fr, handles, tfs, relax, G, compat=True):
    """per frame of more than 0 points: (dL/dU, dL/dw, dL/dmu, [dL/df_k]) of lccrf_inference_backward_modes at t_f, then Q of
    inference(t_f)"""
    want = {}
    for f, h in handles.items():
        n = int(fr.N[f])
        hu, hw, hm, hf = mc.backward(h, fr.dims, fr.L, tfs[f], relax, G[f, :n], compat=compat)
        h.inference(tfs[f], False, relax)
        want[f] = (hu, hw, hm, hf, h.probability())
    return want


def _plus_zero(a):
    return np.all(a == 0) and not np.signbit(a).any()


def _assert_frames_have_handle_bits(fr, want, got, tfs, what, compat=True):
    """per frame: the handle's dL/dU, dL/dw, every dL/df_k, dL/dmu and Q_{t_f}; +0 rows beyond n_points; zeros for an empty frame; +0 in
    every row of dL/df and 0 in dL/dw and dL/dmu for a frame with t_f = 0"""
    for f, n in enumerate(fr.N):
        tag = "%s frame %d (N=%d, t_f=%d)" % (what, f, n, tfs[f])
        assert _plus_zero(got["gu"][f, n:]), tag + ": rows of dL/dU beyond n_points not +0"
        assert all(_plus_zero(a[f, n:]) for a in got["gf"]), tag + ": rows of dL/df beyond n_points not +0"
        if n == 0:
            assert np.all(got["gw"][f] == 0) and (not compat or np.all(got["gm"][f] == 0)), tag + ": an empty frame's gradients not 0"
            continue
        hu, hw, hm, hf, hq = want[f]
        assert cc.same_bits(got["gu"][f, :n], hu), tag + ": dL/dU differs"
        assert cc.same_bits(got["gw"][f], hw), tag + ": dL/dw differs: %s, handle %s" % (got["gw"][f], hw)
        for k, a in enumerate(got["gf"]):
            assert cc.same_bits(a[f, :n], hf[k]), tag + ": dL/df%d differs by up to %g" % (k, np.abs(a[f, :n] - hf[k]).max())
        if compat:
            assert cc.same_bits(got["gm"][f], hm), tag + ": dL/dmu differs by up to %g" % np.abs(got["gm"][f] - hm).max()
        assert cc.same_bits(got["q"][f, :n], hq), tag + ": Q differs"
        if tfs[f] == 0:
            assert all(_plus_zero(a[f]) for a in got["gf"]), tag + ": dL/df of a frame with t_f = 0 not +0 in every bit"
            assert np.all(got["gw"][f] == 0) and (not compat or _plus_zero(got["gm"][f])), tag
    assert all(np.abs(a).max() > 0 for a in got["gf"]) or max(tfs) == 0, what + ": no frame has a feature gradient"
    if compat:
        assert cc.same_bits(got["model"], bl.model_of(got["gw"], got["gm"])), what + ": d_grad_model is not the ordered sum"
    else:
        assert np.isnan(got["gm"]).all() and np.isnan(got["model"]).all(), what + ": an output that was not asked for was written"


# ---- 1. per-frame bits against handles, on both routes ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_every_frame_has_the_bits_of_its_handle_on_both_routes(po, wl, golden, model):
    fr = _frames(golden, wl, model)
    setting = _model(fr, model, po)
    b, handles = tl._learnt_batch(fr, setting), tl._handles(fr, setting)
    b.inference(CAP, True, 1.0)
    b.synchronize()
    labels = b.map()
    tfs = tl.clamped(COUNTS, CAP)
    assert tfs == [3, 0, 1, 5, 2, 5, 5, 0]
    for relax in RELAX_SET:
        G = fr.grad_prob(41 + int(10 * relax))
        for form, compat in ((FULL, True), (PLAIN, False)):
            want = _handle_results(fr, handles, tfs, relax, G, compat)
            for on in (False, True):
                what = "%s relax=%g %s option %d" % (model, relax, "full" if compat else "plain", on)
                got = _call(b, fr, on, CAP, relax, COUNTS, G, **form)
                one_launch = on and not compat and model in ONE_LAUNCH
                assert got["route"] == (FUSED if one_launch else STREAM), what
                _assert_frames_have_handle_bits(fr, want, got, tfs, what, compat)
                assert np.array_equal(b.map(), labels), what + ": the labels changed"
    tl._close(b, handles)


# ---- 2. the stale-area case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["after", "mixed"])
def test_frames_with_count_zero_ignore_what_an_earlier_call_left_in_the_area(po, wl, golden, model):
    """a fixed-count feature call leaves every frame's dL/d(corner weight) and norm accumulators in the area; the counted call behind it
    must give the 5-point and the 2048-point frame, both at t_f = 0, +0 in every bit of dL/df -- on both routes"""
    fr = _frames(golden, wl, model)
    b = tl._learnt_batch(fr, _model(fr, model, po))
    tfs = tl.clamped(COUNTS, CAP)
    zero = [f for f, t in enumerate(tfs) if t == 0 and fr.N[f]]
    assert [int(fr.N[f]) for f in zero] == [5, 2048]
    G = fr.grad_prob(4)
    form = PLAIN if model == "after" else FULL
    for on in (False, True):
        b.set_option(OPT, 0)
        left = mc.batch_backward(b, fr, CAP, 0.7, G, **form)     # (streams: the accumulators of every frame are in the area)
        assert b.backward_route() == STREAM and all(np.abs(a[f, :fr.N[f]]).max() > 0 for a in left["gf"] for f in zero)
        got = _call(b, fr, on, CAP, 0.7, COUNTS, G, **form)
        assert got["route"] == (FUSED if on and model == "after" else STREAM)
        for f in zero:
            for k, a in enumerate(got["gf"]):
                assert _plus_zero(a[f]), (on, f, k, a[f][np.flatnonzero(a[f].any(axis=1) | np.signbit(a[f]).any(axis=1))[:4]])
            assert np.all(got["gw"][f] == 0), (on, f, got["gw"][f])
        assert all(np.isfinite(a).all() for a in got["gf"]) and np.isfinite(got["gw"]).all()
    b.close()


# ---- 3. degenerate counts ---------------------------------------------------------------------------------------------------------
def _fixed(b, fr, on, T, relax, G, form):
    b.set_option(OPT, 1 if on else 0)
    out = mc.batch_backward(b, fr, T, relax, G, **form)
    return dict(out, q=b.probability(), route=b.backward_route())


def _assert_same_call(a, ref, N, what, compat=True, route=True):
    for k in ("gu", "gw") + (("gm", "model") if compat else ()):
        assert cc.same_bits(a[k], ref[k]), "%s: %s differs" % (what, k)
    for k, (x, y) in enumerate(zip(a["gf"], ref["gf"])):
        assert cc.same_bits(x, y), "%s: dL/df%d differs" % (what, k)
    for f, n in enumerate(N):
        assert cc.same_bits(a["q"][f, :n], ref["q"][f, :n]), "%s: Q of frame %d differs" % (what, f)
    assert not route or a["route"] == ref["route"], what


@pytest.mark.parametrize("model,on", [("mixed", False), ("after", False), ("after", True)], ids=["mixed", "after-stream", "after-fused"])
def test_degenerate_counts_are_the_fixed_count_call(po, wl, golden, model, on):
    fr = _frames(golden, wl, model)
    b = tl._learnt_batch(fr, _model(fr, model, po))
    F, relax = len(fr.N), 0.7
    G = fr.grad_prob(5)
    form, compat = (FULL, True) if model == "mixed" else (PLAIN, False)
    at_cap, at_zero = _fixed(b, fr, on, CAP, relax, G, form), _fixed(b, fr, on, 0, relax, G, form)
    assert at_cap["route"] == (FUSED if on else STREAM) and at_zero["route"] == STREAM     # (section 1l: T = 0 streams)
    _assert_same_call(_call(b, fr, on, CAP, relax, [CAP] * F, G, **form), at_cap, fr.N, "every count at the cap", compat)
    _assert_same_call(_call(b, fr, on, CAP, relax, [CAP + 7] * F, G, **form), at_cap, fr.N, "every count beyond the cap", compat)
    # (every count 0 under a cap >= 1: the one-launch kernel takes the request, the fixed-count call at T = 0 streams -- the same bits)
    _assert_same_call(_call(b, fr, on, CAP, relax, [0] * F, G, **form), at_zero, fr.N, "every count 0", compat, route=False)
    _assert_same_call(_call(b, fr, on, 0, relax, COUNTS, G, **form), at_zero, fr.N, "max_iterations = 0", compat)
    assert np.all(at_zero["gw"] == 0) and all(_plus_zero(a) for a in at_zero["gf"])
    b.close()


# ---- 4. no feature arrays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_without_a_feature_array_the_call_is_section_2k_and_on_a_plain_batch_section_2j(po, wl, golden, on):
    import torch
    fr = _frames(golden, wl, "mixed")
    b = tl._learnt_batch(fr, _model(fr, "mixed", po))
    G = fr.grad_prob(6)
    ref = tl._call(b, fr, on, CAP, 0.7, COUNTS, G)               # section 2k's call, options 6 and 7 as `on` says
    assert ref["route"] == (FUSED if on else STREAM)
    for features, skip in ((False, ()), (True, (0, 1))):          # a NULL array; an array of NULL entries
        got = _call(b, fr, on, CAP, 0.7, COUNTS, G, features=features, skip=skip)
        assert all(np.isnan(a).all() for a in got["gf"])
        _assert_same_call(dict(got, gf=[]), dict(ref, gf=[]), fr.N, "no feature array (%s)" % (features,))
    b.close()
    fr = _frames(golden, wl, "after")
    b = fr.batch()
    tl._route(b, on)
    got = _call(b, fr, on, CAP, 0.7, COUNTS, G, features=False, **PLAIN)
    it, g = dev(np.asarray(COUNTS, np.int32)), dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((len(fr.N), fr.K), float("nan"), device="cuda")
    torch.cuda.synchronize()
    b.inference_backward_converged_device(CAP, 0.7, it.data_ptr(), g.data_ptr(), gu.data_ptr(), gw.data_ptr())
    b.synchronize()
    torch.cuda.synchronize()
    assert b.backward_route() == got["route"] == (FUSED if on else STREAM)
    assert cc.same_bits(got["gu"], gu.cpu().numpy()) and cc.same_bits(got["gw"], gw.cpu().numpy())
    assert np.isnan(got["gm"]).all() and np.isnan(got["model"]).all()
    q = b.probability()
    assert all(cc.same_bits(got["q"][f, :n], q[f, :n]) for f, n in enumerate(fr.N))
    b.close()


# ---- 5. entries and outputs left out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,on", [("mixed", False), ("after", True)], ids=["mixed-stream", "after-fused"])
def test_every_entry_and_every_output_left_null_in_turn(po, wl, golden, model, on):
    fr = _frames(golden, wl, model)
    b = tl._learnt_batch(fr, _model(fr, model, po))
    G = fr.grad_prob(8)
    form = FULL if model == "mixed" else PLAIN
    full = _call(b, fr, on, CAP, 0.7, COUNTS, G, **form)
    assert full["route"] == (FUSED if on else STREAM)
    keys = {"unary": "gu", "weights": "gw"}
    keys.update({"compat": "gm", "model": "model"} if model == "mixed" else {})
    cases = [dict(skip=(k,)) for k in range(fr.K)] + [{name: False} for name in keys] + [dict(unary=False, weights=False, skip=(1,))]
    for left_out in cases:
        out = _call(b, fr, on, CAP, 0.7, COUNTS, G, **dict(form, **left_out))
        assert out["route"] == full["route"], left_out
        for name, k in keys.items():
            assert np.isnan(out[k]).all() if left_out.get(name) is False else cc.same_bits(out[k], full[k]), (left_out, name)
        for k, (x, y) in enumerate(zip(out["gf"], full["gf"])):
            assert np.isnan(x).all() if k in left_out.get("skip", ()) else cc.same_bits(x, y), (left_out, k)
        assert all(cc.same_bits(out["q"][f, :n], full["q"][f, :n]) for f, n in enumerate(fr.N)), left_out
    b.close()


# ---- 6. a shape only the streaming route takes ----------------------------------------------------------------------------------
def test_a_streaming_only_shape(wl):
    """three labels, one 3-D term with a matrix, normalised SYMMETRIC: four corners per point, rows of one lane"""
    probs = [wl.generic_problem(n, [3], 3, seed=60 + i) for i, n in enumerate((5, 64, 257))]
    fr = bc.Frames(probs, [float(w) for _, w in probs[0]["kernels"]])
    assert (fr.L, fr.K, fr.dims) == (3, 1, [3])
    for setting in (([nc.SYMMETRIC], jc.dense(1, 3), None), ([nc.AFTER], [None], None)):
        b, handles = tl._learnt_batch(fr, setting), tl._handles(fr, setting)
        counts, cap, relax = (2, 0, 3), 3, 0.7
        G = fr.grad_prob(9)
        for form, compat in ((FULL, True), (PLAIN, False)):
            want = _handle_results(fr, handles, list(counts), relax, G, compat)
            for on in (False, True):
                got = _call(b, fr, on, cap, relax, counts, G, **form)
                assert got["route"] == STREAM, on
                _assert_frames_have_handle_bits(fr, want, got, list(counts), "L=3 d=3 option %d" % on, compat)
        tl._close(b, handles)


# ---- 7. from a real converged run, with no host synchronisation in between ----------------------------------------------------------
@pytest.mark.parametrize("model,on", [("mixed", False), ("after", False), ("after", True)], ids=["mixed", "after-stream", "after-fused"])
def test_the_device_report_of_a_converged_run_goes_straight_in(po, wl, model, on):
    import torch
    fr = bc.Frames([cv.problem(wl, name) for name in tl.CONVERGED_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    setting = bl.setting(fr, model, po)
    b, handles = tl._learnt_batch(fr, setting), tl._handles(fr, setting)
    b.set_option(OPT, 1 if on else 0)
    compat = model == "mixed"
    F, K, L = len(fr.N), fr.K, fr.L
    G = fr.grad_prob(17)
    g = dev(G)
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, K), nan(F, K, L, L), nan(K * (1 + L * L))
    gf = [nan(F, fr.maxN, d) for d in fr.dims]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.inference_converged(cv.CAP, cv.LABELS, 0.0, True, 1.0, stream=s.cuda_stream)
    q_conv = tl._device_q(b, fr, s)                               # (a copy queued on the same stream: no host wait in between)
    b.inference_backward_modes_converged_device(cv.CAP, 1.0, b.device_convergence()["iterations"], g.data_ptr(), gu.data_ptr(),
                                                gw.data_ptr(), [t.data_ptr() for t in gf], gm.data_ptr() if compat else None,
                                                md.data_ptr() if compat else None, stream=s.cuda_stream)
    b.synchronize()
    torch.cuda.synchronize()
    assert b.backward_route() == (FUSED if on else STREAM)
    rep = b.convergence()
    stops = [int(t) for t in rep["iterations"]]
    print("iterations", stops)
    assert all(0 <= t <= cv.CAP for t in stops) and min(stops) < cv.CAP, stops
    got = dict(gu=gu.cpu().numpy(), gw=gw.cpu().numpy(), gm=gm.cpu().numpy(), model=md.cpu().numpy(), gf=[t.cpu().numpy() for t in gf],
               q=b.probability())
    q_conv = q_conv.cpu().numpy()
    for f, n in enumerate(fr.N):
        assert cc.same_bits(got["q"][f, :n], q_conv[f, :n]), "frame %d: Q is not what the converged call left" % f
    _assert_frames_have_handle_bits(fr, _handle_results(fr, handles, stops, 1.0, G, compat), got, stops, "converged run", compat)
    again = b.convergence()
    assert all(np.array_equal(rep[k].view(np.int32), again[k].view(np.int32)) for k in rep), (rep, again)
    tl._close(b, handles)


# ---- 8. the float64 checkers, under the existing bars -------------------------------------------------------------------------------
CHECKED_COUNTS = (5, 1, 0)                                        # (gradient_settings.T_SHORT: counts the existing lists hold the case at)


def _three_copies(pb, w, U, G):
    n = pb["N"]
    fr = bc.Frames([pb] * 3, [float(x) for x in w], max_points=n + bl.SLACK)
    fr.U[:, :n] = U                                               # (the unary the references were computed for)
    Gb = np.full((3, fr.maxN, pb["L"]), np.nan, np.float32)
    Gb[:, :n] = G
    return fr, Gb


@pytest.mark.parametrize("mode", mc.ONE_MODE, ids=[nc.MODE_NAMES[m] for m in mc.ONE_MODE])
def test_frames_match_the_mode_checker_at_their_own_counts(po, wl, golden, mode):
    """every term in `mode` with dense matrices: the case, the references and the bars of tests/test_mode_feature_gradients.py
    (mode_feature_checker.SETTINGS: slam1001:s38, relax 0.7, dense), the 1001-point frame three times in one batch, each copy held to
    the reference at its own count"""
    relax = 0.7
    refs = [mc.reference_for(po, wl, golden, "slam1001:s38", (mode,), t, relax, "dense") for t in CHECKED_COUNTS]
    assert all(("slam1001:s38", (mode,), t, relax, "dense") in mc.SETTINGS for t in CHECKED_COUNTS)
    s = refs[0]
    n = s["pb"]["N"]
    fr, G = _three_copies(s["pb"], s["w"], s["U"], s["G"])
    b = tl._learnt_batch(fr, (s["modes"], s["mats"], None))
    got = _call(b, fr, True, max(CHECKED_COUNTS), relax, CHECKED_COUNTS, G)
    assert got["route"] == STREAM
    for f, ref in enumerate(refs):
        assert all(np.isfinite(a[f, :n]).all() for a in got["gf"])
        ref["ref"].check(gs._named((got["gu"][f, :n], got["gw"][f], got["gm"][f]), [a[f, :n] for a in got["gf"]]))
    assert all(_plus_zero(a[2]) for a in got["gf"])
    assert cc.same_bits(got["model"], bl.model_of(got["gw"], got["gm"]))
    b.close()


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_frames_match_the_feature_checker_at_their_own_counts(po, wl, golden, on):
    """Potts terms normalised AFTER: the case, the references and the bars of tests/test_feature_gradients.py (gradient_settings'
    feature list: slam:N1001, relax 0.7), three times in one batch, each copy held to the references at its own count"""
    relax, name = 0.7, "slam:N1001"
    assert all((name, t, relax) in gset.FEATURE_SETTINGS for t in CHECKED_COUNTS)
    refs = [gset.features(po, wl, golden, name, t, relax) for t in CHECKED_COUNTS]
    pb = refs[0]["pb"]
    n = pb["N"]
    o = cc.setup(po.OracleCRF, pb)
    U = o.unary().astype(np.float32)
    o.close()
    fr, G = _three_copies(pb, gs.weights(pb), U, refs[0]["G"])
    b = fr.batch()
    got = _call(b, fr, on, max(CHECKED_COUNTS), relax, CHECKED_COUNTS, G, **PLAIN)
    assert got["route"] == (FUSED if on else STREAM)
    for f, s in enumerate(refs):
        assert all(np.isfinite(a[f, :n]).all() for a in got["gf"])
        s["ref"].check({"dL/df%d" % k: a[f, :n] for k, a in enumerate(got["gf"])})
        s["ref_1c"].check({"dL/dU": got["gu"][f, :n], "dL/dw": got["gw"][f]})
    assert all(_plus_zero(a[2]) for a in got["gf"]) and np.all(got["gw"][2] == 0)
    b.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_as_it_was(po, wl, golden):
    import torch
    lib, vp = pkg.lib(), C.c_void_p
    fn = lib.lccrf_batch_inference_backward_modes_converged
    fr = _frames(golden, wl, "mixed", Ns=(5, 257, 1000))
    setting = _model(fr, "mixed", po)
    F, K, L = 3, fr.K, fr.L
    G = np.nan_to_num(fr.grad_prob(2))
    it, g = dev(np.array([1, 2, 3], np.int32)), dev(G)
    gu, gw = torch.zeros(G.shape, device="cuda"), torch.zeros((F, K), device="cuda")
    gm, md = torch.zeros((F, K, L, L), device="cuda"), torch.zeros(K * (1 + L * L), device="cuda")
    gf = [torch.zeros((F, fr.maxN, d), device="cuda") for d in fr.dims]
    ptrs = (vp * K)(*[vp(t.data_ptr()) for t in gf])
    torch.cuda.synchronize()
    call = lambda h, cap, relax, itp, fp=ptrs: fn(h, cap, C.c_float(relax), itp, vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()), fp,
                                                  vp(gm.data_ptr()), vp(md.data_ptr()), None)
    itp = vp(it.data_ptr())
    # answered before the batch is looked at: on a NULL batch and on one that is not built
    nb = fr.batch(build=False)
    bl.apply(nb, *setting)
    for h in (None, nb.h):
        assert call(h, -1, 1.0, itp) == E_INVALID and b"max_iterations" in lib.lccrf_last_error()
        assert call(h, 3, float("nan"), itp) == E_INVALID and b"relax" in lib.lccrf_last_error()
        assert call(h, 3, 1.0, None) == E_INVALID and b"d_iterations" in lib.lccrf_last_error()
    assert call(None, 3, 1.0, itp) == E_INVALID
    assert call(nb.h, 3, 1.0, itp) == E_STATE
    nb.close()
    b = tl._learnt_batch(fr, setting)
    b.inference(3, True, 1.0)
    b.synchronize()
    q, labels = b.probability(), b.map()
    host = np.array([1, 2, 3], np.int32)                          # pageable host memory: section 1b refuses it
    hl, short = hip_malloc(8)                                    # [n_frames - 1] counts, and far too small for a feature array
    assert call(b.h, 3, 1.0, vp(host.ctypes.data)) == E_INVALID
    assert call(b.h, 3, 1.0, short) == E_INVALID
    assert call(b.h, 3, 1.0, itp, (vp * K)(vp(gf[0].data_ptr()), short)) == E_INVALID
    hl.hipFree(short)
    assert call(b.h, -1, 1.0, itp) == E_INVALID and call(b.h, 3, float("inf"), itp) == E_INVALID
    assert call(b.h, 3, 1.0, None) == E_INVALID
    assert b.backward_route() == pkg.BACKWARD_NONE
    # the fixed-count and counted calls without section 1m's part keep refusing feature arrays on this batch
    assert lib.lccrf_batch_inference_backward_all(b.h, 1, C.c_float(1.0), vp(g.data_ptr()), None, None, ptrs, None, None, None) == E_STATE
    assert lib.lccrf_batch_inference_backward_converged(b.h, 3, C.c_float(1.0), itp, vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()),
                                                        None) == E_STATE
    torch.cuda.synchronize()
    for t in [gu, gw, gm, md] + gf:                               # nothing was written
        assert float(t.abs().max()) == 0.0
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), labels)
    b.inference(3, True, 1.0)                                    # ... and the batch gives its earlier bits
    b.synchronize()
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), labels)
    handles = tl._handles(fr, setting)
    G2 = fr.grad_prob(3)
    got = _call(b, fr, False, 3, 1.0, [1, 2, 3], G2)
    _assert_frames_have_handle_bits(fr, _handle_results(fr, handles, [1, 2, 3], 1.0, G2), got, [1, 2, 3], "after the refusals")
    tl._close(b, handles)
    # K = 0 is legal
    b0 = pkg.BatchCRF(1, 5, 2, [], [])
    b0.set_inputs_host([5], [], unary=np.random.default_rng(1).standard_normal((1, 5, 2)).astype(np.float32))
    b0.build()
    g0, gu0 = dev(np.ones((1, 5, 2), np.float32)), torch.full((1, 5, 2), float("nan"), device="cuda")
    torch.cuda.synchronize()
    b0.inference_backward_modes_converged_device(2, 1.0, dev(np.array([1], np.int32)).data_ptr(), g0.data_ptr(), gu0.data_ptr())
    b0.synchronize()
    assert np.isfinite(gu0.cpu().numpy()).all()
    b0.close()


# ---- 10. the torch layers -----------------------------------------------------------------------------------------------------------
TORCH_CASES = ("N63", "N1000", "N1025")


def _torch_inputs(fr, seed=0):
    import torch
    scale = 1.0 + 0.01 * seed                                     # (another forward's inputs: other features, so other lattices)
    u = (torch.from_numpy(fr.U).cuda() * scale).requires_grad_(True)
    fs = [(torch.from_numpy(f).cuda() * scale).requires_grad_(True) for f in fr.feats]
    w = torch.tensor(fr.w, requires_grad=True)
    return u, fs, w


def _layer_grads(u, fs, w, m=None):
    out = [u.grad.cpu().numpy()] + [f.grad.cpu().numpy() for f in fs] + [w.grad.numpy().copy()]
    return out + ([m.grad.numpy().copy()] if m is not None else [])


@pytest.mark.parametrize("converged", [False, True], ids=["fixed", "converged"])
@pytest.mark.parametrize("compat,on", [(False, False), (False, True), (True, False)], ids=["potts-stream", "potts-fused", "matrices"])
def test_the_torch_functions_hand_over_the_direct_calls_gradients(wl, converged, compat, on):
    """unary.grad and every features[k].grad are the direct call's bits, weights.grad / compat.grad its d_grad_model (with matrices) or
    torch's sum of its per-frame dL/dw (without); a backward behind another forward on the same batch gives the same bits"""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.Frames([cv.problem(wl, name) for name in TORCH_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    F, K = len(fr.N), fr.K
    b = pkg.BatchCRF(F, fr.maxN, fr.L, fr.dims, fr.w)
    bl.apply(b, [nc.SYMMETRIC, nc.AFTER] if compat else [], [])
    b.set_option(OPT, 1 if on else 0)
    Gn = np.nan_to_num(fr.grad_prob(5))
    G = torch.from_numpy(Gn).cuda()
    cap, relax = (cv.CAP, 1.0) if converged else (5, 0.7)
    mu = np.stack(jc.dense(2, 2))

    def forward(seed):
        u, fs, w = _torch_inputs(fr, seed)
        m = torch.tensor(mu, requires_grad=True) if compat else None
        if converged:
            q, it = ag.mean_field_batch_features_converged(b, fr.N, u, fs, w, cap, relax=relax, compat=m)
            assert not it.requires_grad and it.dtype == torch.int32 and tuple(it.shape) == (F,)
        else:
            q, it = ag.mean_field_batch_features(b, fr.N, u, fs, w, cap, relax, compat=m), None
        return q, it, (u, fs, w, m)

    q, it, leaves = forward(0)
    q.backward(G)
    torch.cuda.synchronize()
    assert b.backward_route() == (FUSED if on else STREAM)
    counts = it.cpu().numpy() if converged else np.full(F, cap, np.int32)
    if converged:
        assert np.array_equal(counts, b.convergence()["iterations"]) and counts.min() < cap, counts
    # the direct call on the batch as the forward left it: its tensors bound, its weights and matrices set
    direct = _call(b, fr, on, cap, relax, counts, Gn, **(FULL if compat else PLAIN))
    assert direct["route"] == (FUSED if on else STREAM)
    got = _layer_grads(*leaves)
    assert cc.same_bits(got[0], direct["gu"])
    for k in range(K):
        assert cc.same_bits(got[1 + k], direct["gf"][k]) and np.linalg.norm(got[1 + k]) > 0, k
    if compat:
        assert cc.same_bits(got[1 + K], direct["model"][:K]) and cc.same_bits(got[2 + K].reshape(-1), direct["model"][K:])
    else:
        assert cc.same_bits(got[1 + K], torch.from_numpy(direct["gw"]).cuda()[:, :K].sum(0).cpu().numpy())
    for f, n in enumerate(fr.N):
        assert cc.same_bits(q.detach().cpu().numpy()[f, :n], direct["q"][f, :n]), f
    # the same forward, another forward on the same batch in between, then its backward
    q, it, leaves = forward(0)
    q2, _, _ = forward(1)
    assert not cc.same_bits(q.detach().cpu().numpy(), q2.detach().cpu().numpy())
    q.backward(G)
    torch.cuda.synchronize()
    for x, y in zip(_layer_grads(*leaves), got):
        assert cc.same_bits(x, y)
    b.close()


@pytest.mark.parametrize("converged", [False, True], ids=["fixed", "converged"])
def test_the_module_gives_the_chain_rule_on_both_routes_and_a_step_moves_log_sd(wl, converged):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.Frames([cv.problem(wl, name) for name in TORCH_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    U = torch.from_numpy(fr.U).cuda()
    Gn = np.nan_to_num(fr.grad_prob(5))
    G = torch.from_numpy(Gn).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.BatchLearnedKernelCRF(fr.N, fr.feats, [1.0, 1.0], fr.w, groups=[[[0, 1]], [[0, 1]]],
                                         max_iterations=cv.CAP if converged else None, n_iterations=5, fused_backward=fused)
        assert [tuple(p.shape) for p in layer.log_sd] == [(1,), (1,)] and all(float(p.detach()) == 0.0 for p in layer.log_sd)
        u = U.clone().requires_grad_(True)
        res = layer(u)
        q, it = res if converged else (res, None)
        q.backward(G)
        torch.cuda.synchronize()
        route = layer.batch.backward_route()
        counts = it.cpu().numpy() if converged else np.full(len(fr.N), 5, np.int32)
        direct = _call(layer.batch, fr, fused, cv.CAP if converged else 5, 1.0, counts, Gn, **PLAIN)
        sd_grads = [float(p.grad) for p in layer.log_sd]
        for k, gk in enumerate(sd_grads):                         # d f / d log_sd = -f: the chain rule on the direct call's dL/df
            want = -float((direct["gf"][k].astype(np.float64) * fr.feats[k]).sum())
            assert np.isfinite(gk) and gk != 0.0 and abs(gk - want) <= 1e-4 * abs(want) + 1e-7, (k, gk, want)
        assert cc.same_bits(u.grad.cpu().numpy(), direct["gu"])
        before = [float(p.detach()) for p in layer.log_sd]
        opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
        opt.step()
        assert all(float(p.detach()) != x for p, x in zip(layer.log_sd, before)), "one optimiser step left log_sd where it was"
        out[fused] = (u.grad.cpu().numpy(), np.array(sd_grads, np.float32), layer.weights.grad.numpy().copy(), q.detach().cpu().numpy(),
                      counts, route)
        layer.close()
    assert out[False][5] == STREAM and out[True][5] == FUSED
    for x, y in zip(out[True][:5], out[False][:5]):
        assert cc.same_bits(x, y)
    assert not converged or out[True][4].min() < cv.CAP

"""Gradients of a batch's converged inference under a learnt model, each frame at its own iteration count (include/lccrf.h section
2k: lccrf_batch_inference_backward_all_converged; notes/convergence.md section 7), on the streaming sweep and on the one-launch
kernel (LCCRF_OPT_FUSED_BACKWARD_LEARNT).  Every comparison is bit for bit (cc.same_bits): per frame against a handle holding that
frame -- lccrf_inference_backward_all at t_f -- against the fixed-count batch call where the counts are equal, against section 2j's
call on a plain batch, and d_grad_model against the restated ordered sum.  Then the frames whose count is 0 behind a call that left
its partials in the area, a real converged run whose device report goes straight into the call, the float64 checker under the
existing bars, the refusals and the torch layers."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import batch_learned_cases as bl
import converge_cases as cv
import crf_cases as cc
import gradient_settings as gset
import joint_checker as jc
import normalization_checker as nc
from abi_support import dev, hip_malloc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT_POTTS, OPT_LEARNT = pkg.OPT_FUSED_BACKWARD, pkg.OPT_FUSED_BACKWARD_LEARNT
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
E_INVALID, E_STATE = -1, -5
# phantom points at each N % 4, a wavefront edge, the 256 / 257 chunk edge of k_compat_bwd, one and two points per lane, and 1, 2, 5
# and 8 chunks of dL/dmu
NS = (0, 5, 7, 64, 257, 1000, 1025, 2048)
CAP, COUNTS = 5, (3, 0, 1, 5, 2, 5, 9, -1)                       # the last two clamp to 5 and 0
RELAX_SET = [1.0, 0.7]
MODELS = list(bl.SETTINGS) + ["one_term"]                        # after (Potts), before, symmetric, none, matrices, mixed; K = 1


def clamped(counts, cap):
    return [min(max(int(c), 0), cap) for c in counts]


def _frames(golden, wl, model, Ns=NS):
    fr = bc.slam_frames(golden, wl, Ns=Ns)
    if model != "one_term":
        return fr
    return bc.Frames([dict(pb, kernels=pb["kernels"][:1]) for pb in fr.probs], fr.w[:1])


def _model(fr, model, po):
    """(modes, matrices, weights) of the model's setting; the one-term variant takes the mixed setting's first term"""
    return bl.setting(fr, "mixed" if model == "one_term" else model, po)


def _learnt_batch(fr, setting):
    b = fr.batch()
    bl.apply(b, *setting)
    return b


def _handles(fr, setting):
    return {f: bl.handle(fr, f, *setting) for f, n in enumerate(fr.N) if n}


def _route(b, on):
    """both one-launch options on or off: the learnt requests answer to option 7, a plain one (section 2j's) to option 6"""
    b.set_option(OPT_POTTS, 1 if on else 0)
    b.set_option(OPT_LEARNT, 1 if on else 0)


def _call(b, fr, on, cap, relax, counts, G, unary=True, weights=True, compat=True, model=True, stream=None):
    """one call with the options on / off, every output pre-filled with NaN: dict(gu, gw, gm, model, q, route); an output that is not
    asked for (a NULL pointer) comes back as filled"""
    import torch
    F, K, L = len(fr.N), fr.K, fr.L
    _route(b, on)
    it = dev(np.asarray(counts, np.int32))
    g = dev(np.ascontiguousarray(G, np.float32))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, max(K, 1)), nan(F, max(K, 1), L, L), nan(max(K, 1) * (1 + L * L))
    torch.cuda.synchronize()
    b.inference_backward_all_converged_device(cap, relax, it.data_ptr(), g.data_ptr(),
                                              gu.data_ptr() if unary else None, gw.data_ptr() if weights and K else None,
                                              gm.data_ptr() if compat and K else None, md.data_ptr() if model and K else None, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return dict(gu=gu.cpu().numpy(), gw=gw[:, :K].cpu().numpy(), gm=gm[:, :K].cpu().numpy(), model=md[:K * (1 + L * L)].cpu().numpy(),
                q=b.probability(), route=b.backward_route())


def _handle_results(fr, handles, tfs, relax, G):
    """per frame of more than 0 points: (dL/dU, dL/dw, dL/dmu) of lccrf_inference_backward_all at t_f, then Q of inference(t_f)"""
    want = {}
    for f, h in handles.items():
        n = int(fr.N[f])
        hu, hw, hm, _ = jc.backward_all(h, fr.dims, fr.L, tfs[f], relax, G[f, :n], features=False)
        h.inference(tfs[f], False, relax)
        want[f] = (hu, hw, hm, h.probability())
    return want


def _assert_frames_have_handle_bits(fr, want, got, tfs, what):
    """per frame: the handle's dL/dU, dL/dw, dL/dmu and Q_{t_f}; +0 rows beyond n_points; zeros for an empty frame and, in dL/dw and
    dL/dmu, for a frame with t_f = 0"""
    for f, n in enumerate(fr.N):
        tag = "%s frame %d (N=%d, t_f=%d)" % (what, f, n, tfs[f])
        assert np.all(got["gu"][f, n:] == 0) and not np.signbit(got["gu"][f, n:]).any(), tag + ": rows beyond n_points not +0"
        if n == 0:
            assert np.all(got["gw"][f] == 0) and np.all(got["gm"][f] == 0), tag + ": an empty frame's gradients not 0"
            continue
        hu, hw, hm, hq = want[f]
        assert cc.same_bits(got["gu"][f, :n], hu), tag + ": dL/dU differs"
        assert cc.same_bits(got["gw"][f], hw), tag + ": dL/dw differs: %s, handle %s" % (got["gw"][f], hw)
        assert cc.same_bits(got["gm"][f], hm), tag + ": dL/dmu differs by up to %g" % np.abs(got["gm"][f] - hm).max()
        assert cc.same_bits(got["q"][f, :n], hq), tag + ": Q differs"
        if tfs[f] == 0:
            assert np.all(got["gw"][f] == 0) and np.all(got["gm"][f] == 0) and not np.signbit(got["gm"][f]).any(), tag
    assert cc.same_bits(got["model"], bl.model_of(got["gw"], got["gm"])), what + ": d_grad_model is not the ordered sum"


def _close(b, handles=None):
    for h in (handles or {}).values():
        h.close()
    b.close()


# ---- 1. per-frame bits against handles, on both routes; 2. the stale-area case ---------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_every_frame_has_the_bits_of_its_handle_on_both_routes(po, wl, golden, model):
    fr = _frames(golden, wl, model)
    setting = _model(fr, model, po)
    b, handles = _learnt_batch(fr, setting), _handles(fr, setting)
    b.inference(CAP, True, 1.0)
    b.synchronize()
    labels = b.map()
    tfs = clamped(COUNTS, CAP)
    assert tfs == [3, 0, 1, 5, 2, 5, 5, 0]
    for relax in RELAX_SET:
        what = "%s relax=%g" % (model, relax)
        G = fr.grad_prob(31 + int(10 * relax))
        want = _handle_results(fr, handles, tfs, relax, G)
        off = _call(b, fr, False, CAP, relax, COUNTS, G)
        assert off["route"] == STREAM, what
        _assert_frames_have_handle_bits(fr, want, off, tfs, what + " streaming")
        on = _call(b, fr, True, CAP, relax, COUNTS, G)
        assert on["route"] == FUSED, what
        _assert_frames_have_handle_bits(fr, want, on, tfs, what + " one launch")
        assert np.array_equal(b.map(), labels), what + ": the labels changed"
    _close(b, handles)


@pytest.mark.parametrize("model", ["matrices", "after"])
def test_frames_with_count_zero_ignore_what_an_earlier_call_left_in_the_area(po, wl, golden, model):
    """the fixed-count streaming call leaves every frame's partials of dL/dmu in the area; no iteration of the counted call writes
    those of a frame with t_f = 0, and its dL/dmu must still be exactly +0 -- on both routes"""
    fr = _frames(golden, wl, model)
    setting = _model(fr, model, po)
    b = _learnt_batch(fr, setting)
    tfs = clamped(COUNTS, CAP)
    zero = [f for f, t in enumerate(tfs) if t == 0 and fr.N[f]]
    assert [int(fr.N[f]) for f in zero] == [5, 2048]
    G = fr.grad_prob(4)
    _route(b, False)
    left = bl.backward_all(b, fr, CAP, 0.7, G)
    assert b.backward_route() == STREAM and all(np.abs(left["gm"][f]).min() > 0 and np.abs(left["gw"][f]).min() > 0 for f in zero)
    for on in (False, True):
        got = _call(b, fr, on, CAP, 0.7, COUNTS, G)
        assert got["route"] == (FUSED if on else STREAM)
        for f in zero:
            assert np.all(got["gm"][f] == 0) and not np.signbit(got["gm"][f]).any(), (on, f, got["gm"][f])
            assert np.all(got["gw"][f] == 0), (on, f, got["gw"][f])
        assert np.isfinite(got["gm"]).all() and np.isfinite(got["gw"]).all() and np.isfinite(got["model"]).all()
        assert cc.same_bits(got["model"], bl.model_of(got["gw"], got["gm"]))
        if not on:
            bl.backward_all(b, fr, CAP, 0.7, G)                  # (the partials again, in front of the one-launch call)
    b.close()


# ---- 3. degenerate counts ---------------------------------------------------------------------------------------------------------
def _fixed(b, fr, on, T, relax, G):
    _route(b, on)
    out = bl.backward_all(b, fr, T, relax, G)
    return dict(out, q=b.probability(), route=b.backward_route())


def _assert_same_call(a, ref, N, what):
    for k in ("gu", "gw", "gm", "model"):
        assert cc.same_bits(a[k], ref[k]), "%s: %s differs" % (what, k)
    for f, n in enumerate(N):
        assert cc.same_bits(a["q"][f, :n], ref["q"][f, :n]), "%s: Q of frame %d differs" % (what, f)
    assert a["route"] == ref["route"], what


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_degenerate_counts_are_the_fixed_count_call(po, wl, golden, on):
    fr = _frames(golden, wl, "mixed")
    b = _learnt_batch(fr, _model(fr, "mixed", po))
    F, relax = len(fr.N), 0.7
    G = fr.grad_prob(5)
    at_cap, at_zero = _fixed(b, fr, on, CAP, relax, G), _fixed(b, fr, on, 0, relax, G)
    assert at_cap["route"] == (FUSED if on else STREAM)
    _assert_same_call(_call(b, fr, on, CAP, relax, [CAP] * F, G), at_cap, fr.N, "every count at the cap")
    _assert_same_call(_call(b, fr, on, CAP, relax, [CAP + 7] * F, G), at_cap, fr.N, "every count beyond the cap")
    _assert_same_call(_call(b, fr, on, CAP, relax, [0] * F, G), at_zero, fr.N, "every count 0")
    _assert_same_call(_call(b, fr, on, 0, relax, COUNTS, G), at_zero, fr.N, "max_iterations = 0")
    assert np.all(at_zero["gw"] == 0) and np.all(at_zero["gm"] == 0)
    b.close()


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_a_plain_batch_without_model_outputs_is_section_2j(wl, golden, on):
    import torch
    fr = _frames(golden, wl, "after")
    b = fr.batch()
    G = fr.grad_prob(6)
    got = _call(b, fr, on, CAP, 0.7, COUNTS, G, compat=False, model=False)
    assert np.isnan(got["gm"]).all() and np.isnan(got["model"]).all()
    it, g = dev(np.asarray(COUNTS, np.int32)), dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((len(fr.N), fr.K), float("nan"), device="cuda")
    torch.cuda.synchronize()
    b.inference_backward_converged_device(CAP, 0.7, it.data_ptr(), g.data_ptr(), gu.data_ptr(), gw.data_ptr())
    b.synchronize()
    torch.cuda.synchronize()
    assert b.backward_route() == got["route"] == (FUSED if on else STREAM)
    assert cc.same_bits(got["gu"], gu.cpu().numpy()) and cc.same_bits(got["gw"], gw.cpu().numpy())
    q = b.probability()
    assert all(cc.same_bits(got["q"][f, :n], q[f, :n]) for f, n in enumerate(fr.N))
    b.close()


# ---- 4. d_grad_model; 5. every output left NULL in turn ---------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_the_model_gradient_and_every_output_left_null_in_turn(po, wl, golden, on):
    fr = _frames(golden, wl, "mixed")
    b = _learnt_batch(fr, _model(fr, "mixed", po))
    G = fr.grad_prob(8)
    full = _call(b, fr, on, CAP, 0.7, COUNTS, G)
    want = bl.model_of(full["gw"], full["gm"])
    assert np.isfinite(want).all() and np.abs(want).min() > 0
    assert cc.same_bits(full["model"], want), (full["model"], want)
    keys = {"unary": "gu", "weights": "gw", "compat": "gm", "model": "model"}
    for left_out in (("unary",), ("weights",), ("compat",), ("model",), ("weights", "compat"), ("unary", "weights", "compat")):
        out = _call(b, fr, on, CAP, 0.7, COUNTS, G, **{k: False for k in left_out})
        assert out["route"] == full["route"], left_out
        for name, k in keys.items():
            assert np.isnan(out[k]).all() if name in left_out else cc.same_bits(out[k], full[k]), (left_out, name)
        assert all(cc.same_bits(out["q"][f, :n], full["q"][f, :n]) for f, n in enumerate(fr.N)), left_out
    b.close()


# ---- 6. a shape only the streaming route takes ----------------------------------------------------------------------------------
def test_a_streaming_only_shape(wl):
    """three labels, one 3-D term with a matrix: the rows of k_compat_bwd are tiles of 85 points, lane p owns entry p of the 3 x 3"""
    probs = [wl.generic_problem(n, [3], 3, seed=60 + i) for i, n in enumerate((5, 64, 257))]
    fr = bc.Frames(probs, [float(w) for _, w in probs[0]["kernels"]])
    assert (fr.L, fr.K, fr.dims) == (3, 1, [3])
    setting = ([nc.AFTER], jc.dense(1, 3), None)
    b, handles = _learnt_batch(fr, setting), _handles(fr, setting)
    counts, cap, relax = (2, 0, 3), 3, 0.7
    G = fr.grad_prob(9)
    want = _handle_results(fr, handles, list(counts), relax, G)
    for on in (False, True):
        got = _call(b, fr, on, cap, relax, counts, G)
        assert got["route"] == STREAM, on
        _assert_frames_have_handle_bits(fr, want, got, list(counts), "L=3 d=3 options %d" % on)
    _close(b, handles)


# ---- 7. from a real converged run, with no host synchronisation in between ----------------------------------------------------------
CONVERGED_CASES = ("N63", "N64", "N65", "N1000", "N1025")


def _device_q(b, fr, stream):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    with torch.cuda.stream(stream):
        return ag._device_view(b.device_buffers()[1], (len(fr.N), fr.maxN, fr.L), torch.device("cuda", 0)).clone()


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_the_device_report_of_a_converged_run_goes_straight_in(po, wl, on):
    import torch
    fr = bc.Frames([cv.problem(wl, name) for name in CONVERGED_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    setting = bl.setting(fr, "mixed", po)
    b, handles = _learnt_batch(fr, setting), _handles(fr, setting)
    _route(b, on)
    F, K, L = len(fr.N), fr.K, fr.L
    G = fr.grad_prob(17)
    g = dev(G)
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, K), nan(F, K, L, L), nan(K * (1 + L * L))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.inference_converged(cv.CAP, cv.LABELS, 0.0, True, 1.0, stream=s.cuda_stream)
    q_conv = _device_q(b, fr, s)                                  # (a copy queued on the same stream: no host wait in between)
    b.inference_backward_all_converged_device(cv.CAP, 1.0, b.device_convergence()["iterations"], g.data_ptr(), gu.data_ptr(),
                                              gw.data_ptr(), gm.data_ptr(), md.data_ptr(), stream=s.cuda_stream)
    b.synchronize()
    torch.cuda.synchronize()
    assert b.backward_route() == (FUSED if on else STREAM)
    rep = b.convergence()
    stops = [int(t) for t in rep["iterations"]]
    print("iterations", stops)
    assert all(0 <= t <= cv.CAP for t in stops) and min(stops) < cv.CAP, stops
    got = dict(gu=gu.cpu().numpy(), gw=gw.cpu().numpy(), gm=gm.cpu().numpy(), model=md.cpu().numpy(), q=b.probability())
    q_conv = q_conv.cpu().numpy()
    for f, n in enumerate(fr.N):
        assert cc.same_bits(got["q"][f, :n], q_conv[f, :n]), "frame %d: Q is not what the converged call left" % f
    _assert_frames_have_handle_bits(fr, _handle_results(fr, handles, stops, 1.0, G), got, stops, "converged run")
    again = b.convergence()
    assert all(np.array_equal(rep[k].view(np.int32), again[k].view(np.int32)) for k in rep), (rep, again)
    _close(b, handles)


# ---- 8. the float64 checker, under the existing bars --------------------------------------------------------------------------------
CHECKED_COUNTS = (5, 1, 0)                                        # (gradient_settings.T_SHORT: the counts the existing bars were found at)


@pytest.mark.parametrize("mode", nc.MODES, ids=[nc.MODE_NAMES[m] for m in nc.MODES])
def test_frames_match_the_float64_checker_at_their_own_counts(po, wl, golden, mode):
    """every term in `mode` with dense matrices: the case, the references and the bars of tests/test_normalization.py
    (gradient_settings.normalization: 10 x the float32 checker's error, capped), the 1001-point frame three times in one batch, each
    copy held to the reference at its own count"""
    relax = 0.7
    refs = [gset.normalization(po, wl, golden, "slam1001:s38", mode, t, relax) for t in CHECKED_COUNTS]
    s = refs[0]
    pb, n = s["pb"], s["pb"]["N"]
    fr = bc.Frames([pb] * 3, [float(x) for x in s["w"]], max_points=n + bl.SLACK)
    fr.U[:, :n] = s["U"]                                          # (the unary the references were computed for)
    b = _learnt_batch(fr, (s["modes"], s["mats"], None))
    G = np.full((3, fr.maxN, 2), np.nan, np.float32)
    G[:, :n] = s["G"]
    got = _call(b, fr, True, max(CHECKED_COUNTS), relax, CHECKED_COUNTS, G)
    print("route", got["route"])
    for f, ref in enumerate(refs):
        ref["ref"].check({"dL/dU": got["gu"][f, :n], "dL/dw": got["gw"][f], "dL/dmu": got["gm"][f]})
    assert cc.same_bits(got["model"], bl.model_of(got["gw"], got["gm"]))
    b.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_as_it_was(po, wl, golden):
    import torch
    lib, vp = pkg.lib(), C.c_void_p
    fn = lib.lccrf_batch_inference_backward_all_converged
    fr = _frames(golden, wl, "mixed", Ns=(5, 257, 1000))
    setting = _model(fr, "mixed", po)
    F, K, L = 3, fr.K, fr.L
    G = np.nan_to_num(fr.grad_prob(2))
    it, g = dev(np.array([1, 2, 3], np.int32)), dev(G)
    gu, gw = torch.zeros(G.shape, device="cuda"), torch.zeros((F, K), device="cuda")
    gm, md = torch.zeros((F, K, L, L), device="cuda"), torch.zeros(K * (1 + L * L), device="cuda")
    torch.cuda.synchronize()
    call = lambda h, cap, relax, itp: fn(h, cap, C.c_float(relax), itp, vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()),
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
    b = _learnt_batch(fr, setting)
    b.inference(3, True, 1.0)
    b.synchronize()
    q, labels = b.probability(), b.map()
    host = np.array([1, 2, 3], np.int32)                          # pageable host memory: section 1b refuses it
    hl, short = hip_malloc(8)                                    # [n_frames - 1] counts
    assert call(b.h, 3, 1.0, vp(host.ctypes.data)) == E_INVALID
    assert call(b.h, 3, 1.0, short) == E_INVALID
    hl.hipFree(short)
    assert call(b.h, -1, 1.0, itp) == E_INVALID and call(b.h, 3, float("inf"), itp) == E_INVALID
    assert call(b.h, 3, 1.0, None) == E_INVALID
    assert b.backward_route() == pkg.BACKWARD_NONE
    # section 2j's call keeps refusing a learnt batch
    assert lib.lccrf_batch_inference_backward_converged(b.h, 3, C.c_float(1.0), itp, vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()),
                                                        None) == E_STATE
    torch.cuda.synchronize()
    for t in (gu, gw, gm, md):                                    # nothing was written
        assert float(t.abs().max()) == 0.0
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), labels)
    b.inference(3, True, 1.0)                                    # ... and the batch gives its earlier bits
    b.synchronize()
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), labels)
    handles = _handles(fr, setting)
    G2 = fr.grad_prob(3)
    got = _call(b, fr, False, 3, 1.0, [1, 2, 3], G2)
    _assert_frames_have_handle_bits(fr, _handle_results(fr, handles, [1, 2, 3], 1.0, G2), got, [1, 2, 3], "after the refusals")
    _close(b, handles)


# ---- 10. the torch layers -----------------------------------------------------------------------------------------------------------
def test_the_torch_function_hands_over_the_direct_calls_gradients(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.Frames([cv.problem(wl, name) for name in ("N63", "N1000", "N1025")], [wl.TUM3["w1"], wl.TUM3["w2"]])
    modes = [nc.SYMMETRIC, nc.AFTER]
    mu = np.stack(jc.dense(2, 2))
    b = fr.batch()
    bl.apply(b, modes, [None, None])
    U = torch.from_numpy(fr.U).cuda()
    Gn = np.nan_to_num(fr.grad_prob(5))
    u = U.clone().requires_grad_(True)
    w = torch.tensor(fr.w, requires_grad=True)
    m = torch.tensor(mu, requires_grad=True)
    q, it = ag.mean_field_batch_compat_converged(b, u, w, m, cv.CAP)
    assert not it.requires_grad and it.dtype == torch.int32 and tuple(it.shape) == (3,)
    q.backward(torch.from_numpy(Gn).cuda())
    torch.cuda.synchronize()
    counts = it.cpu().numpy()
    assert np.array_equal(counts, b.convergence()["iterations"]) and counts.min() < cv.CAP, counts
    direct = _call(b, fr, False, cv.CAP, 1.0, counts, Gn)         # (the batch still carries the forward's weights and matrices)
    assert cc.same_bits(u.grad.cpu().numpy(), direct["gu"])
    assert cc.same_bits(w.grad.numpy(), direct["model"][:2]) and cc.same_bits(m.grad.numpy().reshape(-1), direct["model"][2:])
    for f, n in enumerate(fr.N):
        assert cc.same_bits(q.detach().cpu().numpy()[f, :n], direct["q"][f, :n]), f
    b.close()


def test_the_module_gives_identical_gradients_with_and_without_the_one_launch_backward(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.Frames([cv.problem(wl, name) for name in ("N63", "N1000", "N1025")], [wl.TUM3["w1"], wl.TUM3["w2"]])
    U = torch.from_numpy(fr.U).cuda()
    G = torch.from_numpy(np.nan_to_num(fr.grad_prob(5))).cuda()
    mu = torch.tensor(np.stack(jc.dense(2, 2)))
    out = {}
    for fused in (False, True):
        layer = ag.BatchCompatConvergedMeanFieldCRF(fr.N, fr.feats, fr.w, max_iterations=cv.CAP, normalization=[nc.SYMMETRIC, nc.AFTER],
                                                    fused_backward=fused)
        assert torch.equal(layer.compat.detach(), torch.eye(2).repeat(2, 1, 1))
        layer.compat.data.copy_(mu)
        u = U.clone().requires_grad_(True)
        q, it = layer(u)
        q.backward(G)
        torch.cuda.synchronize()
        out[fused] = (u.grad.cpu().numpy(), layer.weights.grad.numpy().copy(), layer.compat.grad.numpy().copy(), q.detach().cpu().numpy(),
                      it.cpu().numpy(), layer.batch.backward_route())
        layer.close()
    assert out[False][5] == STREAM and out[True][5] == FUSED
    for x, y in zip(out[True][:5], out[False][:5]):
        assert cc.same_bits(x, y)
    assert np.abs(out[True][2]).min() > 0 and out[True][4].min() < cv.CAP

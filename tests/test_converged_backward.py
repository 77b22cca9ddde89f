"""Gradients of a batch's converged inference, each frame at its own iteration count (include/lccrf.h section 2j:
lccrf_batch_inference_backward_converged; notes/convergence.md section 6), on the streaming sweep and on the one-launch kernel.
Every comparison is bit for bit (cc.same_bits): per frame against a handle holding that frame -- lccrf_inference_backward at t_f,
section 1h's recipe -- against the fixed-count batch call where the counts are equal, and option on against option off.  Then a
real converged run whose device report goes straight into the call, the float64 checker under the existing bars, the refusals and
the torch layers."""
import importlib

import numpy as np
import pytest

import batch_cases as bc
import converge_cases as cv
import crf_cases as cc
import grad_support as gs
from abi_support import dev, hip_malloc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT = pkg.OPT_FUSED_BACKWARD
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
E_STATE = -5
# phantom points at each N % 4, a wavefront edge, a 256-point partial-block edge, one to two points per lane, the plan's limit; chain
# rows from about 1000 points on
NS = (0, 5, 7, 64, 257, 1000, 1025, 2048)
CAP, COUNTS = 5, (3, 0, 1, 5, 2, 5, 9, -1)                       # the last two clamp to 5 and 0
RELAX_SET = [1.0, 0.7]
TERMS = {"both": slice(0, 2), "appearance": slice(0, 1), "smoothness": slice(1, 2)}


def clamped(counts, cap):
    return [min(max(int(c), 0), cap) for c in counts]


def _frames(golden, wl, terms="both", Ns=NS):
    fr = bc.slam_frames(golden, wl, Ns=Ns)
    sl = TERMS[terms]
    return fr if terms == "both" else bc.Frames([dict(pb, kernels=pb["kernels"][sl]) for pb in fr.probs], fr.w[sl])


def _call(b, on, cap, relax, counts, G, K, stream=None):
    """one call with the option on / off, the outputs pre-filled with NaN: (dL/dU, dL/dw, Q left behind, route)"""
    import torch
    b.set_option(OPT, 1 if on else 0)
    it = dev(np.asarray(counts, np.int32))
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((G.shape[0], max(K, 1)), float("nan"), device="cuda")
    torch.cuda.synchronize()
    b.inference_backward_converged_device(cap, relax, it.data_ptr(), g.data_ptr(), gu.data_ptr(), gw.data_ptr() if K else None,
                                          stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return gu.cpu().numpy(), gw[:, :K].cpu().numpy(), b.probability(), b.backward_route()


def _assert_frames_have_handle_bits(fr, handles, got, tfs, relax, G, what):
    """per frame: dL/dU and dL/dw of the handle at t_f, +0 rows beyond n_points, zeros for an empty frame, Q = the handle's Q_{t_f}"""
    gu, gw, q = got[:3]
    for f, n in enumerate(fr.N):
        tag = "%s frame %d (N=%d, t_f=%d)" % (what, f, n, tfs[f])
        assert np.all(gu[f, n:] == 0) and not np.signbit(gu[f, n:]).any(), tag + ": rows beyond n_points not +0"
        if n == 0:
            assert np.all(gw[f] == 0), tag + ": weight gradient not 0"
            continue
        h = handles[f]
        h.set_option(OPT, 0)
        hu, hw = gs.backward(h, tfs[f], relax, G[f, :n], fr.K)
        assert cc.same_bits(gu[f, :n], hu), tag + ": dL/dU differs"
        assert cc.same_bits(gw[f], hw), tag + ": dL/dw differs"
        h.inference(tfs[f], False, relax)
        assert cc.same_bits(q[f, :n], h.probability()), tag + ": Q differs"


def _chain_rows(h, K):
    """did the fused plan put the handle's first term on chain rows?  (the engine's report of an inference on the lattices in HBM,
    where a backward puts them)"""
    gs.backward(h, 1, 1.0, np.zeros((h.N, 2)), K)
    h.inference(1, False)
    e, shape = h.engine()
    assert e == 2, e
    return bool(shape >> 20 & 1)


# ---- 1. per-frame bits against handles, on both routes --------------------------------------------------------------------------
@pytest.mark.parametrize("terms", list(TERMS))
def test_every_frame_has_the_bits_of_its_handle_on_both_routes(wl, golden, terms):
    fr = _frames(golden, wl, terms)
    b = fr.batch()
    handles = {f: fr.handle(f) for f, n in enumerate(fr.N) if n}
    if terms == "both":                                          # as test_short_rows_and_chain_rows_both_occur: both kinds of rows
        chain = {int(fr.N[f]): _chain_rows(h, fr.K) for f, h in handles.items()}
        print("chain rows:", chain)
        assert any(chain.values()) and not all(chain.values()), chain
    b.inference(CAP, True, 1.0)
    b.synchronize()
    labels = b.map()
    tfs = clamped(COUNTS, CAP)
    assert tfs == [3, 0, 1, 5, 2, 5, 5, 0]
    for relax in RELAX_SET:
        what = "%s relax=%g" % (terms, relax)
        G = fr.grad_prob(31 + int(10 * relax))
        off = _call(b, False, CAP, relax, COUNTS, G, fr.K)
        assert off[3] == STREAM, what
        _assert_frames_have_handle_bits(fr, handles, off, tfs, relax, G, what + " streaming")
        on = _call(b, True, CAP, relax, COUNTS, G, fr.K)
        assert on[3] == FUSED, what
        _assert_frames_have_handle_bits(fr, handles, on, tfs, relax, G, what + " one launch")
        assert np.array_equal(b.map(), labels), what + ": the labels changed"
    for h in handles.values():
        h.close()
    b.close()


# ---- 2. degenerate counts ---------------------------------------------------------------------------------------------------------
def _fixed(b, on, T, relax, G, K):
    b.set_option(OPT, 1 if on else 0)
    gu, gw = gs.batch_backward(b, T, relax, G, K)
    return gu, gw, b.probability()


def _assert_same_call(a, ref, N, what):
    assert cc.same_bits(a[0], ref[0]), what + ": dL/dU differs"
    assert cc.same_bits(a[1], ref[1]), what + ": dL/dw differs"
    for f, n in enumerate(N):
        assert cc.same_bits(a[2][f, :n], ref[2][f, :n]), "%s: Q of frame %d differs" % (what, f)


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_degenerate_counts_are_the_fixed_count_call(wl, golden, on):
    fr = _frames(golden, wl)
    b = fr.batch()
    F, relax = len(fr.N), 0.7
    G = fr.grad_prob(5)
    at_cap, at_zero = _fixed(b, on, CAP, relax, G, fr.K), _fixed(b, on, 0, relax, G, fr.K)
    _assert_same_call(_call(b, on, CAP, relax, [CAP] * F, G, fr.K), at_cap, fr.N, "every count at the cap")
    _assert_same_call(_call(b, on, CAP, relax, [CAP + 7] * F, G, fr.K), at_cap, fr.N, "every count beyond the cap")
    _assert_same_call(_call(b, on, CAP, relax, [0] * F, G, fr.K), at_zero, fr.N, "every count 0")
    _assert_same_call(_call(b, on, 0, relax, COUNTS, G, fr.K), at_zero, fr.N, "max_iterations = 0")
    assert np.all(at_zero[1] == 0)
    b.close()


def test_a_batch_of_more_frames_than_one_workgroup_orders(wl):
    """300 small frames: the one-launch route hands its workgroups the frames by descending count, ranked on the device in tiles of
    256 frames -- which workgroup runs a frame changes no bit, so option on equals option off, whatever the counts hold"""
    sizes = (5, 7, 64, 130)
    probs = [wl.slam_problem(sizes[i % 4], seed=400 + i) for i in range(300)]
    fr = bc.Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]])
    b = fr.batch()
    counts = np.random.default_rng(3).integers(-2, CAP + 3, 300)
    assert counts.min() < 0 and counts.max() > CAP and len(set(clamped(counts, CAP))) == CAP + 1
    G = fr.grad_prob(12)
    off = _call(b, False, CAP, 0.7, counts, G, fr.K)
    on = _call(b, True, CAP, 0.7, counts, G, fr.K)
    assert off[3] == STREAM and on[3] == FUSED
    _assert_same_call(on, off, fr.N, "300 frames")
    assert np.isfinite(on[1]).all()
    b.close()


# ---- 3. shapes only the streaming route takes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,L", [([2, 2], 3), ([2, 3], 2)], ids=["three_labels", "d3_term"])
def test_streaming_only_shapes(wl, dims, L):
    probs = [wl.generic_problem(300, dims, L, seed=50 + i) for i in range(3)]
    fr = bc.Frames(probs, [float(w) for _, w in probs[0]["kernels"]])
    b = fr.batch()
    handles = {f: fr.handle(f) for f in range(3)}
    counts, cap, relax = (0, 2, 4), 4, 0.7
    G = fr.grad_prob(9)
    out = {}
    for on in (False, True):
        out[on] = _call(b, on, cap, relax, counts, G, fr.K)
        assert out[on][3] == STREAM, (dims, L, on)
        _assert_frames_have_handle_bits(fr, handles, out[on], list(counts), relax, G, "dims=%s L=%d option %d" % (dims, L, on))
    for h in handles.values():
        h.close()
    b.close()


# ---- 4. from a real converged run, with no host synchronisation in between ----------------------------------------------------------
CONVERGED_CASES = ("N63", "N64", "N65", "N1000", "N1025")       # (LABELS, cap 12, relax 1: they stop at 1, 4, 2, 3, 3 -- asserted below)


def _converged_frames(po, wl):
    """the frames, and the iteration each stops at by the oracle's trace on the batch's own inputs (here, on the CPU)"""
    fr = bc.Frames([cv.problem(wl, name) for name in CONVERGED_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    stops = []
    for f, pb in enumerate(fr.probs):
        n = pb["N"]
        one = dict(N=n, L=fr.L, unary=fr.U[f, :n], kernels=[(ft, fr.w[k]) for k, (ft, _) in enumerate(pb["kernels"])])
        stops.append(cv.expect(cv.oracle_trace(po, one, 1.0), cv.LABELS, 0.0, cv.CAP)[0])
    return fr, stops


@pytest.mark.parametrize("on", [False, True], ids=["stream", "fused"])
def test_the_device_report_of_a_converged_run_goes_straight_in(po, wl, on):
    import torch
    fr, stops = _converged_frames(po, wl)
    assert len(set(stops)) >= 2 and min(stops) < cv.CAP, stops    # else the test would pass with one shared count
    b = fr.batch()
    b.set_option(OPT, 1 if on else 0)
    handles = {f: fr.handle(f) for f in range(len(fr.N))}
    G = fr.grad_prob(17)
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((G.shape[0], fr.K), float("nan"), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.inference_converged(cv.CAP, cv.LABELS, 0.0, True, 1.0, stream=s.cuda_stream)
    q_conv = _device_q(b, fr, s)                                  # (a copy queued on the same stream: no host wait in between)
    b.inference_backward_converged_device(cv.CAP, 1.0, b.device_convergence()["iterations"], g.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                          stream=s.cuda_stream)
    b.synchronize()
    torch.cuda.synchronize()
    assert b.backward_route() == (FUSED if on else STREAM)
    rep = b.convergence()
    assert list(rep["iterations"]) == stops, (rep, stops)
    got = (gu.cpu().numpy(), gw.cpu().numpy(), b.probability())
    q_conv = q_conv.cpu().numpy()
    for f, n in enumerate(fr.N):
        assert cc.same_bits(got[2][f, :n], q_conv[f, :n]), "frame %d: Q is not what the converged call left" % f
    _assert_frames_have_handle_bits(fr, handles, got, stops, 1.0, G, "converged run")
    again = b.convergence()
    assert all(np.array_equal(rep[k].view(np.int32), again[k].view(np.int32)) for k in rep), (rep, again)
    for h in handles.values():
        h.close()
    b.close()


def _device_q(b, fr, stream):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    with torch.cuda.stream(stream):
        return ag._device_view(b.device_buffers()[1], (len(fr.N), fr.maxN, fr.L), torch.device("cuda", 0)).clone()


# ---- 5. the float64 checker, under the existing bars ----------------------------------------------------------------------------------
_CHECKED = {}


def _batch_of_test_1(wl, golden):
    """test 1's batch with both terms at relax 0.7 on the one-launch route: computed once, shared by the frames' cases"""
    if not _CHECKED:
        fr = _frames(golden, wl)
        b = fr.batch()
        G = fr.grad_prob(38)
        _CHECKED.update(fr=fr, G=G, got=_call(b, True, CAP, 0.7, COUNTS, G, fr.K))
        b.close()
    return _CHECKED


@pytest.mark.parametrize("f", [f for f, n in enumerate(NS) if n])
def test_frames_match_the_checker_at_their_own_counts(po, wl, golden, f):
    c = _batch_of_test_1(wl, golden)
    fr, G, got = c["fr"], c["G"], c["got"]
    assert got[3] == FUSED
    n, tf = int(fr.N[f]), clamped(COUNTS, CAP)[f]
    pb = dict(fr.probs[f], kernels=[(ft, w) for (ft, _), w in zip(fr.probs[f]["kernels"], fr.w)])
    o, lats, _ = gs.checker(po, pb)
    o.close()
    gs.assert_matches_checker(got[0][f, :n], got[1][f], fr.U[f, :n].astype(np.float64), np.array(fr.w), lats, tf, 0.7,
                              G[f, :n].astype(np.float64), "frame %d (N=%d)" % (f, n))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def _raw_call(b, cap, relax, it, g, gu, gw):
    import ctypes as C
    vp = C.c_void_p
    it = it if isinstance(it, vp) else vp(it.data_ptr())
    return pkg.lib().lccrf_batch_inference_backward_converged(b.h, cap, relax, it, vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()),
                                                              None)


@pytest.mark.parametrize("what", ["matrix", "mode"])
def test_a_learnt_model_is_refused_and_the_batch_stays_as_it_was(wl, golden, what):
    import torch
    fr = _frames(golden, wl, Ns=(5, 257, 1000))
    b = fr.batch()
    if what == "matrix":
        b.set_pairwise_compatibility(0, np.array([[1.0, 0.25], [0.5, 1.0]], np.float32))
    else:
        b.set_normalization(1, pkg.NORMALIZE_SYMMETRIC)
    b.inference(3, True, 1.0)
    b.synchronize()
    q, labels = b.probability(), b.map()
    G = np.nan_to_num(fr.grad_prob(2))
    it, g = dev(np.array([1, 2, 3], np.int32)), dev(G)
    gu, gw = torch.zeros(G.shape, device="cuda"), torch.zeros((3, 2), device="cuda")
    torch.cuda.synchronize()
    for on in (0, 1):
        b.set_option(OPT, on)
        assert _raw_call(b, 3, 1.0, it, g, gu, gw) == E_STATE
        assert b.backward_route() == pkg.BACKWARD_NONE
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), labels)
    b.inference(3, True, 1.0)                                    # ... and the batch is usable
    assert cc.same_bits(b.probability(), q)
    b.close()


def test_before_build_is_a_state_error_and_a_failed_call_leaves_the_batch_usable(wl, golden):
    import torch
    fr = _frames(golden, wl, Ns=(5, 257, 1000))
    b = fr.batch(build=False)
    G = fr.grad_prob(2)
    it, g = dev(np.array([1, 2, 3], np.int32)), dev(G)
    gu, gw = torch.zeros(G.shape, device="cuda"), torch.zeros((3, 2), device="cuda")
    hl, short = hip_malloc(8)                                    # [n_frames - 1] counts: section 1b refuses it
    torch.cuda.synchronize()
    assert _raw_call(b, 3, 1.0, it, g, gu, gw) == E_STATE
    b.build()
    assert _raw_call(b, 3, 1.0, short, g, gu, gw) == -1
    hl.hipFree(short)
    assert _raw_call(b, -1, 1.0, it, g, gu, gw) == -1
    assert _raw_call(b, 3, float("inf"), it, g, gu, gw) == -1
    assert b.backward_route() == pkg.BACKWARD_NONE
    handles = {f: fr.handle(f) for f in range(3)}
    got = _call(b, False, 3, 1.0, [1, 2, 3], G, fr.K)
    _assert_frames_have_handle_bits(fr, handles, got, [1, 2, 3], 1.0, G, "after the refusals")
    for h in handles.values():
        h.close()
    b.close()


# ---- 7. the torch layers --------------------------------------------------------------------------------------------------------------
TORCH_CASES = ("N2", "N63", "N64", "N65", "N1000", "N1025")


def test_batched_torch_layer_equals_six_handle_layers(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.Frames([cv.problem(wl, name) for name in TORCH_CASES], [wl.TUM3["w1"], wl.TUM3["w2"]])
    U = torch.from_numpy(fr.U).cuda()
    G = torch.from_numpy(np.nan_to_num(fr.grad_prob(5))).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.BatchConvergedMeanFieldCRF(fr.N, fr.feats, fr.w, max_iterations=cv.CAP, **({"fused_backward": True} if fused else {}))
        u = U.clone().requires_grad_(True)
        q, it = layer(u)
        assert not it.requires_grad and it.dtype == torch.int32
        q.backward(G)
        torch.cuda.synchronize()
        out[fused] = (u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), q.detach().cpu().numpy(), it.cpu().numpy(),
                      layer.batch.backward_route())
        layer.close()
    assert out[False][4] == STREAM and out[True][4] == FUSED
    for x, y in zip(out[True][:4], out[False][:4]):
        assert cc.same_bits(x, y)
    # the report, read before any backward
    b = fr.batch()
    w = torch.tensor(fr.w)
    q, it = ag.mean_field_batch_converged(b, U, w, cv.CAP)
    torch.cuda.synchronize()
    rep = b.convergence()["iterations"]
    assert np.array_equal(it.cpu().numpy(), rep) and np.array_equal(out[False][3], rep)
    assert len(set(rep.tolist())) >= 2 and rep.min() < cv.CAP, rep
    b.close()
    # six handle layers at their reported counts
    gw_frames = []
    for f, n in enumerate(fr.N):
        layer = ag.MeanFieldCRF(int(n), 2, [ft[f, :n] for ft in fr.feats], fr.w, n_iterations=int(rep[f]))
        u = U[f, :n].clone().requires_grad_(True)
        qh = layer(u)
        qh.backward(G[f, :n])
        torch.cuda.synchronize()
        assert cc.same_bits(out[False][0][f, :n], u.grad.cpu().numpy()), "frame %d: unary.grad differs" % f
        assert cc.same_bits(out[False][2][f, :n], qh.detach().cpu().numpy()), "frame %d: Q differs" % f
        assert np.all(out[False][0][f, n:] == 0)
        gw_frames.append(layer.weights.grad.clone())
        layer.close()
    gw_sum = torch.stack(gw_frames).cuda().sum(0).cpu().numpy()  # (the batch layer's own reduction of its [F, K] array)
    assert cc.same_bits(out[False][1], gw_sum), (out[False][1], gw_sum)


def test_handle_torch_function_equals_mean_field_at_the_reported_count(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = cv.problem(wl, "N1000")
    feats, w = [f for f, _ in pb["kernels"]], [float(x) for _, x in pb["kernels"]]
    U = torch.from_numpy(cc.raw_unary(pb)).cuda()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((1000, 2)).astype(np.float32)).cuda()
    layer = ag.MeanFieldCRF(1000, 2, feats, w)
    u = U.clone().requires_grad_(True)
    q, it = ag.mean_field_converged(layer.crf, u, layer.weights, cv.CAP)
    t = int(layer.crf.convergence()["iterations"])
    assert int(it) == t and 0 < t < cv.CAP, (it, t)
    q.backward(G)
    torch.cuda.synchronize()
    got = (u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), q.detach().cpu().numpy())
    layer.weights.grad = None
    u2 = U.clone().requires_grad_(True)
    q2 = ag.mean_field(layer.crf, u2, layer.weights, t)
    q2.backward(G)
    torch.cuda.synchronize()
    for x, y in zip(got, (u2.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), q2.detach().cpu().numpy())):
        assert cc.same_bits(x, y)
    layer.close()

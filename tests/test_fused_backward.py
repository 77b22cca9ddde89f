"""The one-launch backward (include/lccrf.h section 1j, LCCRF_OPT_FUSED_BACKWARD; csrc/fused_backward.hip) against the streaming
sweep it replaces: every comparison is bit for bit, option on against option off on the same object -- dL/dU with its zero rows,
dL/dw and the Q left behind -- and the route is asserted both ways.  Then the float64 checker under the existing bars, and the
torch layers' keyword."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
from abi_support import hip_malloc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT = pkg.OPT_FUSED_BACKWARD
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
# phantom points at each N % 4, wavefront and 256-point partial-block edges, 1 -> 2 points per lane, the plan's limit
HANDLE_NS = [1, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2000, 2047, 2048]
T_SET, RELAX_SET = [0, 1, 2, 5, 10], [1.0, 0.7]
TERMS = {"both": slice(0, 2), "appearance": slice(0, 1), "smoothness": slice(1, 2)}


def _problem(wl, N, terms="both", seed=None):
    pb = wl.slam_problem(N, seed=300 + N if seed is None else seed)
    return dict(pb, kernels=pb["kernels"][TERMS[terms]])


def _call(h, on, T, relax, G, K):
    """one backward with the option on / off: (dL/dU, dL/dw, Q left behind, route)"""
    h.set_option(OPT, 1 if on else 0)
    gu, gw = gs.backward(h, T, relax, G, K)
    return gu, gw, h.probability(), h.backward_route()


def _assert_same(a, b, what):
    for name, x, y in zip(("dL/dU", "dL/dw", "Q"), a[:3], b[:3]):
        assert cc.same_bits(x, y), "%s: %s differs (max |d| %g)" % (what, name, np.abs(x.astype(np.float64) - y).max() if x.size else 0)


def _assert_route(on, T, what):
    assert on[3] in ((STREAM, FUSED) if T == 0 else (FUSED,)), "%s: route %d with the option on" % (what, on[3])


def _chain_rows(h):
    """did the fused plan put the handle's first term on chain rows?  (the engine's report of an inference on the lattices in HBM)"""
    h.inference(1, False)
    e, shape = h.engine()
    assert e == 2, e
    return bool(shape >> 20 & 1)


# ---- handles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", HANDLE_NS)
def test_handle_bits_equal_the_streaming_sweep(wl, N):
    for terms in TERMS:
        pb = _problem(wl, N, terms)
        K = len(pb["kernels"])
        h = cc.setup(pkg.DenseCRFHIP, pb)
        assert h.backward_route() == pkg.BACKWARD_NONE
        for T in T_SET:
            for relax in RELAX_SET:
                what = "N=%d %s T=%d relax=%g" % (N, terms, T, relax)
                G = np.random.default_rng(1000 * T + int(10 * relax)).standard_normal((N, 2))
                off = _call(h, False, T, relax, G, K)
                assert off[3] == STREAM, what
                on = _call(h, True, T, relax, G, K)
                _assert_route(on, T, what)
                _assert_same(on, off, what)
        h.close()


def test_short_rows_and_chain_rows_both_occur(wl):
    """which frames of the handle test ran the first term on chain rows (measured on the MI355X: with both terms -- the appearance
    term first -- N = 1023, 1024, 1025, 2000, 2047 and 2048; N = 1 .. 257, and the smoothness term alone at every N, on short rows)"""
    chain = {}
    for terms in ("both", "smoothness"):
        for N in HANDLE_NS:
            pb = _problem(wl, N, terms)
            h = cc.setup(pkg.DenseCRFHIP, pb)
            G = np.zeros((N, 2))
            on = _call(h, True, 1, 1.0, G, len(pb["kernels"]))
            assert on[3] == FUSED
            chain[terms, N] = _chain_rows(h)
            h.close()
    print("chain rows:", sorted(k for k, v in chain.items() if v), "short rows:", sorted(k for k, v in chain.items() if not v))
    assert any(chain.values()) and not all(chain.values())
    assert any(chain["both", N] for N in HANDLE_NS) and not any(chain["smoothness", N] for N in HANDLE_NS)
    assert chain["both", 2048] and not chain["both", 257]


@pytest.mark.parametrize("kind", ["N2049", "three_labels", "d3_term"])
def test_frames_outside_the_plan_keep_the_streaming_route(wl, kind):
    if kind == "N2049":
        pb = _problem(wl, 2049)
    elif kind == "three_labels":
        pb = wl.generic_problem(700, [2, 2], 3, seed=5)
    else:
        pb = wl.generic_problem(700, [2, 3], 2, seed=6)
    K = len(pb["kernels"])
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(8).standard_normal((pb["N"], pb["L"]))
    for T, relax in ((5, 1.0), (2, 0.7)):
        off = _call(h, False, T, relax, G, K)
        on = _call(h, True, T, relax, G, K)
        assert off[3] == STREAM and on[3] == STREAM, (kind, off[3], on[3])
        _assert_same(on, off, kind)
    h.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------
RAGGED = (0, 5, 7, 257, 1000, 1001, 2000, 2048)


def _batch_call(b, on, T, relax, G, K, stream=None):
    b.set_option(OPT, 1 if on else 0)
    gu, gw = gs.batch_backward(b, T, relax, G, K, stream=stream)
    return gu, gw, b.probability(), b.backward_route()


def _assert_same_frames(a, b, N, what):
    assert cc.same_bits(a[0], b[0]), what + ": dL/dU differs"
    assert cc.same_bits(a[1], b[1]), what + ": dL/dw differs"
    for f, n in enumerate(N):
        assert cc.same_bits(a[2][f, :n], b[2][f, :n]), "%s: Q of frame %d differs" % (what, f)


def _assert_handle_bits(fr, handles, gu, gw, T, relax, G):
    for f, n in enumerate(fr.N):
        assert np.all(gu[f, n:] == 0) and not np.signbit(gu[f, n:]).any(), "frame %d: rows beyond n_points not +0" % f
        if n == 0:
            assert np.all(gw[f] == 0), "frame %d (0 points): weight gradient not 0" % f
            continue
        handles[f].set_option(OPT, 0)
        hu, hw = gs.backward(handles[f], T, relax, G[f, :n], fr.K)
        assert cc.same_bits(gu[f, :n], hu) and cc.same_bits(gw[f], hw), "frame %d (N=%d) T=%d relax=%g" % (f, n, T, relax)


def test_ragged_batch_has_the_bits_of_the_sweep_and_of_its_handles(wl, golden):
    fr = bc.slam_frames(golden, wl, Ns=RAGGED)
    b = fr.batch()
    assert b.backward_route() == pkg.BACKWARD_NONE
    handles = {f: fr.handle(f) for f, n in enumerate(fr.N) if n}
    for T, relax in ((0, 1.0), (1, 0.7), (5, 1.0), (10, 0.7)):
        what = "T=%d relax=%g" % (T, relax)
        G = fr.grad_prob(7 + T)
        off = _batch_call(b, False, T, relax, G, fr.K)
        assert off[3] == STREAM
        on = _batch_call(b, True, T, relax, G, fr.K)
        _assert_route(on, T, what)
        _assert_same_frames(on, off, fr.N, what)
        _assert_handle_bits(fr, handles, on[0], on[1], T, relax, G)
    for h in handles.values():
        h.close()
    b.close()


def test_one_frame_beyond_the_plan_streams_the_whole_batch(wl, golden):
    fr = bc.slam_frames(golden, wl, Ns=RAGGED + (3000,))
    b = fr.batch()
    G = fr.grad_prob(3)
    off = _batch_call(b, False, 5, 0.7, G, fr.K)
    on = _batch_call(b, True, 5, 0.7, G, fr.K)
    assert off[3] == STREAM and on[3] == STREAM
    _assert_same_frames(on, off, fr.N, "with a 3000-point frame")
    b.close()


def test_rebound_batch_carries_no_stale_rows(wl, golden):
    big = bc.slam_frames(golden, wl, Ns=(2002, 2002, 1500))
    b = big.batch()
    b.set_option(OPT, 1)
    G = big.grad_prob(11)
    a1 = gs.batch_backward(b, 5, 1.0, G, 2)
    assert b.backward_route() == FUSED
    small = bc.slam_frames(golden, wl, Ns=(1001, 5))
    small = bc.Frames(small.probs, small.w, max_points=2002)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    handles = {f: small.handle(f) for f in range(2)}
    for T, relax in ((5, 1.0), (10, 0.7), (1, 1.0)):
        G = small.grad_prob(T)
        on = _batch_call(b, True, T, relax, G, 2)
        assert on[3] == FUSED
        _assert_handle_bits(small, handles, on[0], on[1], T, relax, G)
        off = _batch_call(b, False, T, relax, G, 2)
        _assert_same_frames(on, off, small.N, "rebound T=%d" % T)
    for h in handles.values():
        h.close()
    b.close()
    assert np.isfinite(a1[1]).all()


def test_a_user_stream_is_honoured(wl, golden):
    import torch
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000))
    b = fr.batch()
    G = fr.grad_prob(4)
    off = _batch_call(b, False, 5, 0.7, G, fr.K)
    s = torch.cuda.Stream()
    on = _batch_call(b, True, 5, 0.7, G, fr.K, stream=s.cuda_stream)
    assert on[3] == FUSED
    _assert_same_frames(on, off, fr.N, "user stream")
    b.close()


# ---- state and determinism -----------------------------------------------------------------------------------------------------
def test_toggling_the_option_and_repeating_the_call(wl):
    pb = _problem(wl, 2000, seed=12)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(9).standard_normal((2000, 2))
    runs = [_call(h, on, 5, 0.7, G, 2) for on in (True, False, True, True, False)]
    assert [r[3] for r in runs] == [FUSED, STREAM, FUSED, FUSED, STREAM]
    for r in runs[1:]:
        _assert_same(r, runs[0], "toggled")
    h.inference(5, True, 0.7)                                   # the next inference is unchanged
    assert cc.same_bits(h.probability(), runs[0][2])
    h.close()


@pytest.mark.parametrize("how", ["engine1", "engine2", "pending_run"])
def test_backward_leaves_what_inference_leaves(wl, golden, how):
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000, 1500))
    T, relax = 5, 0.7
    G = fr.grad_prob(3)
    ref = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000, 1500)).batch()
    off = _batch_call(ref, False, T, relax, G, fr.K)
    ref.close()
    b = fr.batch()
    b.set_option(OPT, 1)
    b.set_engine(1 if how == "engine1" else 2 if how == "engine2" else 0)
    b.inference(T, False, relax)
    q_ref = b.probability()
    if how == "pending_run":
        b.run(T, True, relax)                                   # one launch per frame, left pending: the backward settles it
    on = _batch_call(b, True, T, relax, G, fr.K)
    assert on[3] == FUSED
    _assert_same_frames(on, off, fr.N, how)
    assert all(cc.same_bits(on[2][f, :n], q_ref[f, :n]) for f, n in enumerate(fr.N))
    b.inference(T, True, relax)                                 # ... and the next inference is unchanged
    q = b.probability()
    assert all(cc.same_bits(q[f, :n], q_ref[f, :n]) for f, n in enumerate(fr.N))
    b.close()


def test_after_set_pairwise_weight(wl):
    pb = _problem(wl, 1500, seed=8)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(3).standard_normal((1500, 2))
    first = _call(h, True, 5, 1.0, G, 2)
    for k, w in enumerate((4.5, 17.25)):
        h.set_pairwise_weight(k, w)
    on = _call(h, True, 5, 1.0, G, 2)
    off = _call(h, False, 5, 1.0, G, 2)
    assert on[3] == FUSED and off[3] == STREAM
    _assert_same(on, off, "new weights")
    assert not cc.same_bits(on[0], first[0])
    fresh = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, np.float32(w)) for (f, _), w in zip(pb["kernels"], (4.5, 17.25))]))
    _assert_same(_call(fresh, True, 5, 1.0, G, 2), on, "a handle built with the weights")
    h.close(), fresh.close()


def test_argument_checks_with_the_option_on(po, wl):
    """the cases of test_backward_argument_checks_leave_the_handle_usable, with the same codes"""
    import torch
    pb = _problem(wl, 2000, seed=4)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.set_option(OPT, 1)
    L = pkg.lib()
    g = torch.zeros((2000, 2), device="cuda")
    gu = torch.zeros((2000, 2), device="cuda")
    gw = torch.zeros(2, device="cuda")
    host = np.zeros((2000, 2), np.float32)
    hl, small = hip_malloc(64)
    try:
        vp = C.c_void_p
        for args in ((1, 1.0, None, vp(gu.data_ptr()), None),
                     (1, 1.0, vp(g.data_ptr()), None, None),
                     (1, 1.0, vp(host.ctypes.data), vp(gu.data_ptr()), None),
                     (1, 1.0, small, vp(gu.data_ptr()), None),
                     (1, 1.0, vp(g.data_ptr()), small, None),
                     (-1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None),
                     (1, float("nan"), vp(g.data_ptr()), vp(gu.data_ptr()), None)):
            assert L.lccrf_inference_backward(h.h, *args) == -1, args
        hl2, small4 = hip_malloc(4)
        assert L.lccrf_inference_backward(h.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), small4) == -1
        hl2.hipFree(small4)
        h0 = pkg.DenseCRFHIP(2000, 2)
        h0.set_option(OPT, 1)
        assert L.lccrf_inference_backward(h0.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None) == -5
        assert h0.backward_route() == pkg.BACKWARD_NONE
        h0.close()
    finally:
        hl.hipFree(small)
    assert h.backward_route() == pkg.BACKWARD_NONE               # no call has succeeded yet
    o = cc.setup(po.OracleCRF, pb)
    h.inference(5, True)
    o.inference_native(5, True)
    assert cc.same_bits(h.probability(), o.probability())
    torch.cuda.synchronize()
    h.inference_backward_device(5, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr())
    h.synchronize()
    assert h.backward_route() == FUSED
    assert np.all(gu.cpu().numpy() == 0) and np.all(gw.cpu().numpy() == 0)   # dL/dQ = 0
    assert cc.same_bits(h.probability(), o.probability())
    h.close()


# ---- the float64 checker ---------------------------------------------------------------------------------------------------------
def test_slam_frame_matches_the_checker(po, wl, golden):
    T, relax = 5, 0.7
    s = gset.meanfield(po, wl, golden, "slam:N1001", T, relax)
    h, keep = gs.gpu_handle(s["pb"], s["image"])
    on = _call(h, True, T, relax, s["G"], 2)
    h.close()
    assert on[3] == FUSED
    s["ref"].check({"dL/dU": on[0], "dL/dw": on[1]})


def test_one_term_frame_matches_the_checker(po, wl):
    T, relax = 5, 1.0
    pb = _problem(wl, 700, "smoothness", seed=2)
    o, lats, U = gs.checker(po, pb)
    o.close()
    G = gset.grad_prob(pb)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    on = _call(h, True, T, relax, G, 1)
    h.close()
    assert on[3] == FUSED
    gs.assert_matches_checker(on[0], on[1], U, gs.weights(pb), lats, T, relax, G, "smoothness alone, N=700")


# ---- the torch layers ---------------------------------------------------------------------------------------------------------------
def test_torch_layer_keyword(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.slam_problem(1500, seed=6)
    feats, w = [f for f, _ in pb["kernels"]], [float(x) for _, x in pb["kernels"]]
    U = torch.from_numpy(cc.raw_unary(pb)).cuda()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((1500, 2)).astype(np.float32)).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.MeanFieldCRF(1500, 2, feats, w, n_iterations=5, relax=0.7, **({"fused_backward": True} if fused else {}))
        u = U.clone().requires_grad_(True)
        q = layer(u)
        q.backward(G)
        torch.cuda.synchronize()
        out[fused] = (u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), q.detach().cpu().numpy(), layer.crf.backward_route())
        layer.close()
    assert out[False][3] == STREAM and out[True][3] == FUSED
    _assert_same(out[True], out[False], "MeanFieldCRF")


def test_batched_torch_layer_keyword(wl, golden):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000))
    U = torch.from_numpy(fr.U).cuda()
    G = torch.from_numpy(np.nan_to_num(fr.grad_prob(5))).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.BatchMeanFieldCRF(fr.N, fr.feats, fr.w, n_iterations=5, relax=0.7, **({"fused_backward": True} if fused else {}))
        u = U.clone().requires_grad_(True)
        q = layer(u)
        q.backward(G)
        torch.cuda.synchronize()
        out[fused] = (u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), q.detach().cpu().numpy(), layer.batch.backward_route())
        layer.close()
    assert out[False][3] == STREAM and out[True][3] == FUSED
    _assert_same(out[True], out[False], "BatchMeanFieldCRF")

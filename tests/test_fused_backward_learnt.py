"""The one-launch backward of learnt models (include/lccrf.h section 1k, LCCRF_OPT_FUSED_BACKWARD_LEARNT;
csrc/fused_backward_general.hip) against the streaming sweep it replaces: every comparison is bit for bit, option on against option
off on the same object -- dL/dU with its zero rows, dL/dw, dL/dmu and the Q left behind -- and the route is asserted both ways.  Then
the routing between the two options, the float64 checkers under the existing bars, and the layers' keyword."""
import importlib

import numpy as np
import pytest

import batch_cases as bc
import batch_learned_cases as bl
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import joint_checker as jc
import normalization_checker as nc
import test_fused_general as fg
from abi_support import dev

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT6, OPT7 = pkg.OPT_FUSED_BACKWARD, getattr(pkg, "OPT_FUSED_BACKWARD_LEARNT", 7)
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
# phantom points at each N % 4, wavefront edges, 256 / 257: one chunk of dL/dmu -> two of 129 + 128, 513: three of 171, 1 -> 2 points
# per lane, 2000: eight chunks of 250, one across point 1024, 2047: a last chunk of 255, the plan's limit
HANDLE_NS = [1, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 513, 1023, 1024, 1025, 2000, 2047, 2048]
T_SET, RELAX_SET = [0, 1, 2, 5], [1.0, 0.7]
TERMS = {"both": slice(0, 2), "appearance": slice(0, 1), "smoothness": slice(1, 2)}
NAMES = ("dL/dU", "dL/dw", "dL/dmu", "Q")


def _problem(wl, N, terms="both", seed=None):
    pb = wl.slam_problem(N, seed=300 + N if seed is None else seed)
    return dict(pb, kernels=pb["kernels"][TERMS[terms]])


def _setting(po, pb, sname):
    """(modes, matrices, weights) of test_fused_general's setting `sname` on the problem's terms; a term in mode NONE has its weight
    scaled by its mean norm (normalization_checker.weights_f32), as batch_learned_cases.setting does"""
    K = len(pb["kernels"])
    modes, mats = fg._settings(K)[sname]
    w = [np.float32(x) for _, x in pb["kernels"]]
    if nc.NONE in modes:
        o = cc.setup(po.OracleCRF, pb)
        nrm = [o.kernel(k)["norm"] for k in range(K)]
        o.close()
        w = nc.weights_f32(pb, nrm, modes)
    return modes, mats, [float(x) for x in w]


def _handle(po, pb, sname):
    modes, mats, w = _setting(po, pb, sname)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    bl.apply(h, modes, mats, w)
    general = any(m != nc.AFTER for m in modes) or any(m is not None for m in mats)
    return h, general


def _call(h, on, call, T, relax, G, K, skip=None, opt6=False):
    """one backward with option 7 on / off: (dL/dU, dL/dw, dL/dmu, Q left behind, route); every output pre-filled with NaN, the one
    named by `skip` passed as NULL"""
    import torch
    h.set_option(OPT7, 1 if on else 0)
    h.set_option(OPT6, 1 if opt6 else 0)
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    gm = torch.full((max(K, 1), 2, 2), float("nan"), device="cuda")
    p = lambda t, name: None if skip == name else t.data_ptr()
    torch.cuda.synchronize()
    if call == "backward":
        h.inference_backward_device(T, relax, g.data_ptr(), gu.data_ptr(), p(gw, "dL/dw"))
    elif call == "compat":
        h.inference_backward_compat_device(T, relax, g.data_ptr(), p(gu, "dL/dU"), p(gw, "dL/dw"), p(gm, "dL/dmu"))
    else:
        h.inference_backward_all_device(T, relax, g.data_ptr(), p(gu, "dL/dU"), p(gw, "dL/dw"), None, p(gm, "dL/dmu"))
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy(), gm[:K].cpu().numpy(), h.probability(), h.backward_route()


def _assert_same(a, b, what):
    for name, x, y in zip(NAMES, a[:4], b[:4]):
        assert cc.same_bits(x, y), "%s: %s differs (max |d| %g)" % (what, name, np.nanmax(np.abs(x.astype(np.float64) - y)) if x.size else 0)


def _assert_route(on, T, fused, what):
    want = (STREAM,) if not fused else (STREAM, FUSED) if T == 0 else (FUSED,)
    assert on[4] in want, "%s: route %d with the option on" % (what, on[4])


def _compare(h, call, T, relax, G, K, fused, what, skip=None):
    off = _call(h, False, call, T, relax, G, K, skip)
    assert off[4] == STREAM, what
    on = _call(h, True, call, T, relax, G, K, skip)
    _assert_route(on, T, fused, what)
    _assert_same(on, off, what)
    return on


# ---- handles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", HANDLE_NS)
def test_handle_bits_equal_the_streaming_sweep(po, wl, N):
    """the six settings x both / one term x T x relax through lccrf_inference_backward_compat; at (5, 0.7) and (1, 1.0) also
    lccrf_inference_backward (general models) and lccrf_inference_backward_all without feature arrays; at (2, 0.7) every output NULL
    in turn"""
    for terms in TERMS:
        pb = _problem(wl, N, terms)
        K = len(pb["kernels"])
        for sname in bl.SETTINGS:
            h, general = _handle(po, pb, sname)
            assert h.backward_route() == pkg.BACKWARD_NONE
            for T in T_SET:
                for relax in RELAX_SET:
                    what = "N=%d %s %s T=%d relax=%g" % (N, terms, sname, T, relax)
                    G = np.random.default_rng(1000 * T + int(10 * relax)).standard_normal((N, 2))
                    on = _compare(h, "compat", T, relax, G, K, True, what)
                    assert np.isfinite(on[2]).all(), what
                    if T == 0:
                        assert np.all(on[2] == 0) and not np.signbit(on[2]).any(), what
                    if (T, relax) in ((5, 0.7), (1, 1.0)):
                        if general:
                            _compare(h, "backward", T, relax, G, K, True, what + " backward")
                        _compare(h, "all", T, relax, G, K, True, what + " all")
                    if (T, relax) == (2, 0.7):
                        for skip in NAMES[:3]:
                            # (without d_grad_compat a Potts model's request is section 1c's: option 6's, not this route's)
                            fused = general or skip != "dL/dmu"
                            for call in ("compat", "all"):
                                o = _compare(h, call, T, relax, G, K, fused, "%s %s without %s" % (what, call, skip), skip)
                                for name, x, y in zip(NAMES[:3], o[:3], on[:3]):
                                    assert np.isnan(x).all() if name == skip else cc.same_bits(x, y), (what, call, skip, name)
            h.close()


def _chain_rows(h):
    """did the fused plan put the handle's first term on chain rows?  (the engine's report of an inference on the lattices in HBM)"""
    h.inference(1, False)
    e, shape = h.engine()
    assert e in (2, 4), e
    return bool(shape >> 20 & 1)


def test_short_rows_and_chain_rows_both_occur(po, wl):
    chain = {}
    for terms in ("both", "smoothness"):
        for N in HANDLE_NS:
            pb = _problem(wl, N, terms)
            h, _ = _handle(po, pb, "matrices")
            on = _call(h, True, "compat", 1, 1.0, np.zeros((N, 2)), len(pb["kernels"]))
            assert on[4] == FUSED
            chain[terms, N] = _chain_rows(h)
            h.close()
    print("chain rows:", sorted(k for k, v in chain.items() if v), "short rows:", sorted(k for k, v in chain.items() if not v))
    assert any(chain["both", N] for N in HANDLE_NS) and not any(chain["smoothness", N] for N in HANDLE_NS)
    assert chain["both", 2048] and not chain["both", 257]


# ---- batches ------------------------------------------------------------------------------------------------------------------
RAGGED = bl.RAGGED + (2048,)
KEYS = ("gu", "gw", "gm", "model")


def _batch_call(b, fr, on, T, relax, G, opt6=False, **kw):
    b.set_option(OPT7, 1 if on else 0)
    b.set_option(OPT6, 1 if opt6 else 0)
    out = bl.backward_all(b, fr, T, relax, G, **kw)
    return out, b.probability(), b.backward_route()


def _assert_same_frames(a, b, N, what):
    for k in KEYS:
        assert cc.same_bits(a[0][k], b[0][k]), "%s: %s differs" % (what, k)
    for f, n in enumerate(N):
        assert cc.same_bits(a[1][f, :n], b[1][f, :n]), "%s: Q of frame %d differs" % (what, f)


@pytest.mark.parametrize("sname", bl.SETTINGS)
def test_ragged_batch_has_the_bits_of_the_sweep_and_of_its_handles(po, wl, golden, sname):
    fr = bl.ragged(golden, wl, Ns=RAGGED)
    assert fr.maxN == 2048 + bl.SLACK
    modes, mats, w = bl.setting(fr, sname, po)
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    assert b.backward_route() == pkg.BACKWARD_NONE
    handles = {f: bl.handle(fr, f, modes, mats, w) for f, n in enumerate(fr.N) if n}
    for T, relax in ((0, 1.0), (1, 0.7), (5, 1.0), (2, 0.7)):
        what = "%s T=%d relax=%g" % (sname, T, relax)
        G = fr.grad_prob(7 + T)
        off = _batch_call(b, fr, False, T, relax, G)
        assert off[2] == STREAM
        on = _batch_call(b, fr, True, T, relax, G)
        _assert_route((None,) * 4 + (on[2],), T, True, what)
        _assert_same_frames(on, off, fr.N, what)
        out = on[0]
        assert not np.signbit(out["gu"][np.arange(fr.maxN)[None, :] >= fr.N[:, None]]).any(), what + ": rows beyond n_points not +0"
        f0 = list(fr.N).index(0)
        assert np.all(out["gm"][f0] == 0) and not np.signbit(out["gm"][f0]).any() and not np.signbit(out["gw"][f0]).any(), what
        bl.check_frames(out, fr, handles, T, relax, G, False, what)           # (the handles run the sweep: option 7 is off on them)
        assert cc.same_bits(out["model"], bl.model_of(out["gw"], out["gm"]))
    # d_grad_model with the per-frame arrays passed or NULL
    G = fr.grad_prob(3)
    full = _batch_call(b, fr, True, 5, 0.7, G)[0]
    for keep in (dict(weights=False), dict(compat=False), dict(weights=False, compat=False, unary=False)):
        out, _, route = _batch_call(b, fr, True, 5, 0.7, G, **keep)
        assert route == FUSED and cc.same_bits(out["model"], full["model"]), keep
        assert np.isnan(out["gw"]).all() == ("weights" in keep) and np.isnan(out["gm"]).all() == ("compat" in keep), keep
    for h in handles.values():
        h.close()
    b.close()


def test_one_frame_beyond_the_plan_streams_the_whole_batch(po, wl, golden):
    fr = bl.ragged(golden, wl, Ns=RAGGED + (3000,))
    modes, mats, w = bl.setting(fr, "mixed", po)
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    G = fr.grad_prob(3)
    off = _batch_call(b, fr, False, 5, 0.7, G)
    on = _batch_call(b, fr, True, 5, 0.7, G)
    assert off[2] == STREAM and on[2] == STREAM
    _assert_same_frames(on, off, fr.N, "with a 3000-point frame")
    b.close()


def test_rebound_batch_carries_no_stale_rows(po, wl, golden):
    big = bc.slam_frames(golden, wl, Ns=(2002, 2002, 1500))
    modes, mats, w = bl.setting(big, "matrices", po)
    b = big.batch()
    bl.apply(b, modes, mats, w)
    a1, _, route = _batch_call(b, big, True, 5, 1.0, big.grad_prob(11))
    assert route == FUSED and np.isfinite(a1["model"]).all()
    small = bc.slam_frames(golden, wl, Ns=(1001, 5))
    small = bc.Frames(small.probs, small.w, max_points=2002)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    handles = {f: bl.handle(small, f, modes, mats, w) for f in range(2)}
    for T, relax in ((5, 1.0), (1, 0.7)):
        G = small.grad_prob(T)
        on = _batch_call(b, small, True, T, relax, G, F=2)
        assert on[2] == FUSED
        bl.check_frames(on[0], small, handles, T, relax, G, False, "rebound")
        off = _batch_call(b, small, False, T, relax, G, F=2)
        _assert_same_frames(on, off, small.N, "rebound T=%d" % T)
    for h in handles.values():
        h.close()
    b.close()


def test_a_user_stream_is_honoured(po, wl, golden):
    import torch
    fr = bl.ragged(golden, wl, Ns=(5, 1000, 0, 2000))
    modes, mats, w = bl.setting(fr, "symmetric", po)
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    G = fr.grad_prob(4)
    off = _batch_call(b, fr, False, 5, 0.7, G)
    s = torch.cuda.Stream()
    on = _batch_call(b, fr, True, 5, 0.7, G, stream=s.cuda_stream)
    assert on[2] == FUSED
    _assert_same_frames(on, off, fr.N, "user stream")
    b.close()


# ---- routing ------------------------------------------------------------------------------------------------------------------
def test_each_option_selects_its_own_requests(po, wl):
    pb = _problem(wl, 2000, seed=12)
    G = np.random.default_rng(9).standard_normal((2000, 2))
    T, relax = 5, 0.7
    learnt, general = _handle(po, pb, "mixed")
    potts, plain = _handle(po, pb, "after")
    assert general and not plain
    ref_l = _call(learnt, False, "backward", T, relax, G, 2)
    ref_p = _call(potts, False, "backward", T, relax, G, 2)
    ref_pc = _call(potts, False, "compat", T, relax, G, 2)
    assert [r[4] for r in (ref_l, ref_p, ref_pc)] == [STREAM] * 3
    # option 6 alone on a learnt model streams; option 7 alone on a Potts dU / dw request streams
    r = _call(learnt, False, "backward", T, relax, G, 2, opt6=True)
    assert r[4] == STREAM
    _assert_same(r, ref_l, "option 6 on a learnt model")
    r = _call(potts, True, "backward", T, relax, G, 2)
    assert r[4] == STREAM
    _assert_same(r, ref_p, "option 7 on a Potts dU / dw request")
    r = _call(potts, False, "compat", T, relax, G, 2, opt6=True)
    assert r[4] == STREAM                                       # (dL/dmu is not option 6's)
    # both set: each request goes to its kernel
    for h, call, ref in ((learnt, "backward", ref_l), (potts, "backward", ref_p), (potts, "compat", ref_pc)):
        r = _call(h, True, call, T, relax, G, 2, opt6=True)
        assert r[4] == FUSED, call
        _assert_same(r, ref, "both options, " + call)
    learnt.close(), potts.close()


def test_a_request_with_a_feature_array_streams(po, wl):
    import torch
    pb = _problem(wl, 1500, seed=3)
    h, _ = _handle(po, pb, "matrices")
    h.set_option(OPT7, 1)
    h.set_option(OPT6, 1)
    g = dev(np.random.default_rng(1).standard_normal((1500, 2)).astype(np.float32))
    gu, gm = torch.zeros((1500, 2), device="cuda"), torch.zeros((2, 2, 2), device="cuda")
    gf = torch.zeros((1500, 2), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_all_device(5, 0.7, g.data_ptr(), gu.data_ptr(), None, [gf.data_ptr(), None], gm.data_ptr())
    h.synchronize()
    assert h.backward_route() == STREAM
    h.inference_backward_all_device(5, 0.7, g.data_ptr(), gu.data_ptr(), None, [None, None], gm.data_ptr())
    h.synchronize()
    assert h.backward_route() == FUSED                           # (an array of NULLs asks for no feature gradient)
    h.close()


@pytest.mark.parametrize("kind", ["N2049", "three_labels", "d3_term"])
def test_frames_outside_the_plan_keep_the_streaming_route(wl, kind):
    if kind == "N2049":
        pb = _problem(wl, 2049)
    elif kind == "three_labels":
        pb = wl.generic_problem(700, [2, 2], 3, seed=5)
    else:
        pb = wl.generic_problem(700, [2, 3], 2, seed=6)
    K, L = len(pb["kernels"]), pb["L"]
    h = cc.setup(pkg.DenseCRFHIP, pb)
    jc.set_all(h, jc.dense(K, L))
    G = np.random.default_rng(8).standard_normal((pb["N"], L))
    out = {}
    for on in (False, True):
        h.set_option(OPT7, 1 if on else 0)
        out[on] = jc.backward_compat(h, K, L, 5, 0.7, G) + (h.probability(), h.backward_route())
    assert out[False][4] == STREAM and out[True][4] == STREAM, kind
    _assert_same(out[True], out[False], kind)
    h.close()


def test_toggling_the_option_and_repeating_the_call(po, wl):
    pb = _problem(wl, 2000, seed=12)
    h, _ = _handle(po, pb, "mixed")
    G = np.random.default_rng(9).standard_normal((2000, 2))
    h.inference(5, True, 0.7)
    q_ref = h.probability()
    runs = [_call(h, on, "compat", 5, 0.7, G, 2) for on in (True, False, True, True, False)]
    assert [r[4] for r in runs] == [FUSED, STREAM, FUSED, FUSED, STREAM]
    for r in runs[1:]:
        _assert_same(r, runs[0], "toggled")
    assert cc.same_bits(runs[0][3], q_ref)
    h.inference(5, True, 0.7)                                   # the next inference is unchanged
    assert cc.same_bits(h.probability(), q_ref)
    h.close()


def test_a_parked_handle_comes_back_with_the_option_off(po, wl):
    pb = _problem(wl, 1500, seed=8)
    G = np.random.default_rng(3).standard_normal((1500, 2))
    h, _ = _handle(po, pb, "matrices")
    assert _call(h, True, "compat", 2, 1.0, G, 2)[4] == FUSED
    h.close()                                                   # parked with the option on
    h2, _ = _handle(po, pb, "matrices")
    h2.set_option(OPT6, 0)
    import torch
    g, gu = dev(G.astype(np.float32)), torch.zeros((1500, 2), device="cuda")
    gm = torch.zeros((2, 2, 2), device="cuda")
    torch.cuda.synchronize()
    h2.inference_backward_compat_device(2, 1.0, g.data_ptr(), gu.data_ptr(), None, gm.data_ptr())
    h2.synchronize()
    assert h2.backward_route() == STREAM
    h2.close()


# ---- the float64 checkers ---------------------------------------------------------------------------------------------------------
CHECK_SLAM = ("slam1001:s38", nc.SYMMETRIC, 5, 0.7)              # slam:N1001's twin with matrices (gradient_settings.COMPAT_TWINS)


def test_slam_frame_with_matrices_and_symmetric_terms_matches_the_checker(po, wl, golden):
    name, mode, T, relax = CHECK_SLAM
    assert CHECK_SLAM in gset.NORM_SETTINGS and CHECK_SLAM not in gset.DROPPED["normalization"]
    assert gset.COMPAT_TWINS["slam:N1001"] == name and ("slam:N1001", T, relax) not in jc.DROPPED
    s = gset.normalization(po, wl, golden, name, mode, T, relax)
    pb = dict(s["pb"], kernels=[(f, w) for (f, _), w in zip(s["pb"]["kernels"], s["w"])])
    h = cc.setup(pkg.DenseCRFHIP, pb)
    bl.apply(h, s["modes"], s["mats"])
    on = _call(h, True, "compat", T, relax, s["G"], 2)
    h.close()
    assert on[4] == FUSED
    s["ref"].check(dict(zip(NAMES[:3], on[:3])))


def test_one_term_frame_matches_the_checker(po, wl):
    """the smoothness term alone as a Potts term: dL/dmu at mu = I against the compat checker at the identity"""
    T, relax = 5, 1.0
    pb = _problem(wl, 700, "smoothness", seed=2)
    o, lats, U = gs.checker(po, pb)
    o.close()
    G = gset.grad_prob(pb)
    ref = gs.compat_reference(U, gs.weights(pb), jc.eyes(1, 2), lats, T, relax, G, "smoothness alone, N=700")
    h = cc.setup(pkg.DenseCRFHIP, pb)
    on = _call(h, True, "compat", T, relax, G, 1)
    h.close()
    assert on[4] == FUSED
    ref.check(dict(zip(NAMES[:3], on[:3])))


# ---- the torch layers ---------------------------------------------------------------------------------------------------------------
def _layer_run(layer, U, G, route):
    import torch
    with torch.no_grad():
        layer.compat.copy_(torch.from_numpy(np.stack(jc.dense(2, 2))).to(layer.compat.device))
    u = U.clone().requires_grad_(True)
    q = layer(u)
    q.backward(G)
    torch.cuda.synchronize()
    out = (u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), layer.compat.grad.cpu().numpy(), q.detach().cpu().numpy(), route())
    layer.close()
    return out


def test_compat_layer_keyword(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.slam_problem(1500, seed=6)
    feats, w = [f for f, _ in pb["kernels"]], [float(x) for _, x in pb["kernels"]]
    U = torch.from_numpy(cc.raw_unary(pb)).cuda()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((1500, 2)).astype(np.float32)).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.CompatMeanFieldCRF(1500, 2, feats, w, n_iterations=5, relax=0.7, normalization=nc.SYMMETRIC,
                                      **({"fused_backward": True} if fused else {}))
        out[fused] = _layer_run(layer, U, G, layer.crf.backward_route)
    assert out[False][4] == STREAM and out[True][4] == FUSED
    _assert_same(out[True], out[False], "CompatMeanFieldCRF")


def test_batched_compat_layer_keyword(wl, golden):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000))
    U = torch.from_numpy(fr.U).cuda()
    G = torch.from_numpy(np.nan_to_num(fr.grad_prob(5))).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.BatchCompatMeanFieldCRF(fr.N, fr.feats, fr.w, n_iterations=5, relax=0.7, normalization=nc.SYMMETRIC,
                                           **({"fused_backward": True} if fused else {}))
        out[fused] = _layer_run(layer, U, G, layer.batch.backward_route)
    assert out[False][4] == STREAM and out[True][4] == FUSED
    _assert_same(out[True], out[False], "BatchCompatMeanFieldCRF")

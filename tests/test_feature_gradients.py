"""Gradients of mean-field inference with respect to the features of the pairwise terms (include/lccrf.h sections 1d and 2d) and
the torch layers on top (lc-crf-slam_amd/autograd.py: mean_field_features, LearnedKernelCRF).

CPU: the new symbols, and the new kernels' freedom from scratch memory.  GPU: lccrf_inference_backward_features against the
float64 checker with the weights a function of the features (tests/meanfield_f64_features.py; pinned on the CPU by
test_feature_gradients_checker.py), its bit contracts (dL/dU, dL/dw and Q as section 1c; run to run; a NULL entry; a batch's frames
against handles), locality-mode frames, argument checks and the torch layers."""
import ctypes as C
import importlib
import os
import re
import shutil

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import feature_cases as fc
import grad_support as gs
import gradient_settings as gset
import kernel_resources as kr
import meanfield_f64_features as mff
from abi_support import assert_declared_exported_bound, dev, hip_malloc, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_inference_backward_features", "lccrf_batch_inference_backward_features")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_feature_gradient_symbols_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3                         # sections 1d / 2d came without a version step
    assert hasattr(pkg.DenseCRFHIP, "inference_backward_features_device")
    assert hasattr(pkg.BatchCRF, "inference_backward_features_device")
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    assert callable(ag.mean_field_features) and issubclass(ag.LearnedKernelCRF, __import__("torch").nn.Module)


def test_feature_gradient_entry_points_reject_a_null_handle(lib):
    assert lib.lccrf_inference_backward_features(None, 1, 1.0, None, None, None, None) == -1
    assert lib.lccrf_batch_inference_backward_features(None, 1, 1.0, None, None, None, None, None) == -1


@pytest.mark.skipif(shutil.which(kr.HIPCC) is None, reason="hipcc not installed")
def test_backward_kernels_use_no_scratch():
    """The sweep's kernels are small; scratch there is an accident (a register array indexed at run time).  Every kernel of
    meanfield_backward.hip -- the corner dots (five lane groups), the corner-to-feature kernel (d = 1 .. 8), the norm adjoint
    and both forms of the softmax backward -- compiles without it."""
    use = kr.resource_usage("meanfield_backward.hip")
    names = {k: v for k, v in use.items() if re.search(r"k_(corner_dot|corner_to_feature|norm_adjoint|softmax_bwd|bwd_)", k)}
    assert sum("k_corner_dot" in k for k in names) == 5
    assert sum("k_corner_to_feature" in k for k in names) == 8
    assert sum("k_softmax_bwd" in k for k in names) == 10 and sum("k_norm_adjoint" in k for k in names) == 1
    for name, r in names.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _dims(pb, image):
    return [2, 5] if image is not None else [int(f.shape[1]) for f, _ in pb["kernels"]]


def _backward_features(h, dims, T, relax, G, skip=(), unary=True, weights=True):
    """(dL/dU, dL/dw, [dL/df_k or None]) from lccrf_inference_backward_features; every output pre-filled with NaN"""
    import torch
    K, N = len(dims), G.shape[0]
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    gf = [None if k in skip else torch.full((N, d), float("nan"), device="cuda") for k, d in enumerate(dims)]
    torch.cuda.synchronize()
    h.inference_backward_features_device(T, relax, g.data_ptr(), gu.data_ptr() if unary else None,
                                         gw.data_ptr() if K and weights else None, [t.data_ptr() if t is not None else None for t in gf])
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy(), [t.cpu().numpy() if t is not None else None for t in gf]


def _checker(po, pb):
    o = cc.setup(po.OracleCRF, pb)
    return o, mff.lattices(o, pb), o.unary().astype(np.float64)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,T,relax", gset.FEATURE_SETTINGS, ids=gset.FEATURE_IDS)
def test_feature_gradients_match_the_checker(po, wl, golden, name, T, relax):
    """dL/df of every term against the float64 checker on the cases of test_gradients_match_the_checker without the tie cases
    (tests/feature_cases.py; large:c5 runs in locality mode), under that test's bars: relative L2 error and worst row, every bar
    capped at 1e-2 (grad_support.assert_within_bar).  dL/dU and dL/dw of the same call are held to the same checker too.  The
    settings, the seeds behind the names and the three settings dropped: tests/gradient_settings.py.  Measured on the MI355X (the
    figures are printed, -s; notes/gradient_bars.md section 4): every L2 error of dL/df is <= 6e-5 (nt:d8_L33, bar 4.2e-4) and
    every worst row <= 5.1e-4 (nt:d2-5-3_L9, T = 5, relax 1, bar 1.8e-3); the largest bar is the row bar of image64x48, T = 10,
    relax 1, RGB term: 5.5e-3."""
    s = gset.features(po, wl, golden, name, T, relax)
    h, keep = gs.gpu_handle(s["pb"], s["image"])
    gu, gw, gf = _backward_features(h, _dims(s["pb"], s["image"]), T, relax, s["G"])
    h.close()
    assert all(np.isfinite(a).all() for a in gf)
    s["ref"].check({"dL/df%d" % k: a for k, a in enumerate(gf)})
    s["ref_1c"].check({"dL/dU": gu, "dL/dw": gw})
    if T == 0:
        assert np.all(gw == 0) and all(np.all(a == 0) for a in gf)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,relax", gset.TIES, ids=gset.TIES_IDS)
def test_feature_gradients_at_exact_lattice_ties(po, wl, golden, name, T, relax):
    """Frames whose points sit ON the lattice build's rounding ties and rank ties (tests/lattice_tie_cases.py): the derivative is
    one-sided there, the side is the simplex, and the backward recomputes the simplex itself (k_corner_to_feature through
    lattice_simplex).  Held to the float64 checker over the ORACLE's simplex under the bars and the cap of every other list
    (gradient_settings.TIES; tests/test_gradient_bars.py covers the list): a device that rounds a tie or ranks a tie another way
    differentiates another simplex's weights."""
    s = gset.ties(po, wl, golden, name, T, relax)
    h, keep = gs.gpu_handle(s["pb"], None)
    gu, gw, gf = _backward_features(h, _dims(s["pb"], None), T, relax, s["G"])
    h.close()
    assert all(np.isfinite(a).all() for a in gf)
    s["ref"].check({"dL/df%d" % k: a for k, a in enumerate(gf)})
    s["ref_1c"].check({"dL/dU": gu, "dL/dw": gw})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "nt:d3_L21", "nt:d2-5-3_L9", "large:c5", "image64x48"])
def test_bits_of_section_1c_determinism_null_entries_and_state(po, wl, golden, name):
    """dL/dU and dL/dw are bit for bit lccrf_inference_backward's; Q afterwards is lccrf_inference(h, T, 0, relax)'s; two runs
    give the same bits; a NULL entry leaves the other terms' bits unchanged; d_grad_features == NULL is section 1c; NULL
    d_grad_unary / d_grad_weights change nothing else; no NaN comes back from arrays pre-filled with it."""
    pb, image = fc.case(name, golden, po, wl)
    dims = _dims(pb, image)
    K = len(dims)
    G = np.random.default_rng(9).standard_normal((pb["N"], pb["L"]))
    h, keep = gs.gpu_handle(pb, image)
    T, relax = 5, 0.7
    ru, rw = gs.backward(h, T, relax, G, K)
    a = _backward_features(h, dims, T, relax, G)
    q_after = h.probability()
    b = _backward_features(h, dims, T, relax, G)
    assert cc.same_bits(a[0], ru) and cc.same_bits(a[1], rw)
    assert cc.same_bits(b[0], ru) and cc.same_bits(b[1], rw)
    for x, y in zip(a[2], b[2]):
        assert np.isfinite(x).all() and cc.same_bits(x, y)
    h.inference(T, False, relax)
    assert cc.same_bits(q_after, h.probability())
    for skip in range(K):
        c = _backward_features(h, dims, T, relax, G, skip=(skip,))
        assert cc.same_bits(c[0], ru) and cc.same_bits(c[1], rw) and c[2][skip] is None
        assert all(cc.same_bits(x, y) for k, (x, y) in enumerate(zip(a[2], c[2])) if k != skip)
    c = _backward_features(h, dims, T, relax, G, skip=tuple(range(K)))
    assert cc.same_bits(c[0], ru) and cc.same_bits(c[1], rw)
    c = _backward_features(h, dims, T, relax, G, unary=False, weights=False)
    assert np.isnan(c[0]).all() and np.isnan(c[1]).all()        # (untouched)
    assert all(cc.same_bits(x, y) for x, y in zip(a[2], c[2]))
    import torch
    g, gu = dev(G.astype(np.float32)), torch.full(G.shape, float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_features_device(T, relax, g.data_ptr(), gu.data_ptr(), None, None)
    h.synchronize()
    assert cc.same_bits(gu.cpu().numpy(), ru)
    # a fresh handle whose first call is this one gives the same bits
    h2, keep2 = gs.gpu_handle(pb, image)
    d = _backward_features(h2, dims, T, relax, G)
    assert cc.same_bits(d[0], ru) and all(cc.same_bits(x, y) for x, y in zip(a[2], d[2]))
    h.close(), h2.close()


@pytest.mark.gpu
def test_t0_is_exactly_zero_and_k0_is_legal(wl):
    pb = wl.slam_problem(700, seed=2)
    G = np.random.default_rng(5).standard_normal((pb["N"], 2))
    h = cc.setup(pkg.DenseCRFHIP, pb)
    ru, rw = gs.backward(h, 0, 1.0, G, 2)
    gu, gw, gf = _backward_features(h, [2, 2], 0, 1.0, G)
    assert cc.same_bits(gu, ru) and np.all(gw == 0) and all(np.all(a == 0) for a in gf)
    h.close()
    gen = wl.generic_problem(300, [2], 5, seed=3)
    h0 = pkg.DenseCRFHIP(300, 5)
    h0.set_unary(gen["unary"])
    G5 = np.random.default_rng(6).standard_normal((300, 5))
    ru, _ = gs.backward(h0, 3, 0.7, G5, 0)
    gu, _, gf = _backward_features(h0, [], 3, 0.7, G5)
    assert cc.same_bits(gu, ru) and gf == []
    h0.close()


def _batch_backward_features(b, fr, T, relax, G, skip=()):
    import torch
    F = len(fr.probs)
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((F, max(fr.K, 1)), float("nan"), device="cuda")
    gf = [None if k in skip else torch.full((F, fr.maxN, d), float("nan"), device="cuda") for k, d in enumerate(fr.dims)]
    torch.cuda.synchronize()
    b.inference_backward_features_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr() if fr.K else None,
                                         [t.data_ptr() if t is not None else None for t in gf])
    b.synchronize()
    torch.cuda.synchronize()
    return gu.cpu().numpy(), gw[:, :fr.K].cpu().numpy(), [t.cpu().numpy() if t is not None else None for t in gf]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["slam", "generic", "K8_L9", "K8_L33"])
def test_every_frame_of_a_batch_has_the_bits_of_its_handle(wl, golden, kind):
    """ragged frames (0 points, 1 point, a full frame among them): per frame dL/df, dL/dU and dL/dw are the bits of a handle
    holding that frame; rows beyond a frame's points and frames of 0 points come back 0 from arrays pre-filled with NaN; the
    batch's dL/dU and dL/dw are lccrf_batch_inference_backward's bits"""
    if kind == "slam":
        fr = bc.slam_frames(golden, wl, Ns=(0, 1, 5, 1000, 1001, 2002, 3000))
    elif kind == "generic":
        fr = bc.generic_frames(wl, Ns=(300, 0, 1, 1500, 77, 2500))
    else:
        fr = bc.label_frames(int(kind[4:]), (300, 0, 1100, 1, 650), seed=400)
    assert fr.maxN == max(fr.N)
    b = fr.batch()
    handles = {f: fr.handle(f) for f, n in enumerate(fr.N) if n}
    for T, relax in ((0, 1.0), (1, 1.0), (5, 0.7), (10, 1.0)):
        G = fr.grad_prob(100 * T + int(relax * 10))
        ru, rw = gs.batch_backward(b, T, relax, G, fr.K)
        gu, gw, gf = _batch_backward_features(b, fr, T, relax, G)
        assert cc.same_bits(gu, ru) and cc.same_bits(gw, rw)
        for f, n in enumerate(fr.N):
            for k in range(fr.K):
                assert np.all(gf[k][f, n:] == 0), "frame %d term %d: rows beyond n_points not 0" % (f, k)
            if n == 0:
                continue
            hu, hw, hf = _backward_features(handles[f], fr.dims, T, relax, G[f, :n])
            assert cc.same_bits(gu[f, :n], hu) and cc.same_bits(gw[f], hw)
            for k in range(fr.K):
                assert cc.same_bits(gf[k][f, :n], hf[k]), "frame %d (N=%d) term %d T=%d relax=%g" % (f, n, k, T, relax)
        if T == 5 and fr.K > 1:
            c = _batch_backward_features(b, fr, T, relax, G, skip=(0,))
            assert c[2][0] is None and all(cc.same_bits(x, y) for x, y in zip(gf[1:], c[2][1:]))
    for h in handles.values():
        h.close()
    b.close()


@pytest.mark.gpu
def test_locality_mode_frame_gives_the_gradient_in_the_callers_order(po, golden):
    """one frame of >= 8192 points after a locality-mode inference(): the lattices are re-built the plain way, the gradient comes
    in the caller's point order (same bar), and a handle that never ran in locality mode gives the same bits"""
    s = gset.features(po, None, golden, "large:c5", 5, 1.0)      # (the setting of test_feature_gradients_match_the_checker)
    pb, G = s["pb"], s["G"]
    assert pb["N"] >= 8192
    dims = _dims(pb, None)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.inference(5, True)                                         # locality mode
    gu, gw, gf = _backward_features(h, dims, 5, 1.0, G)
    s["ref"].check({"dL/df%d" % k: a for k, a in enumerate(gf)})
    h2 = cc.setup(pkg.DenseCRFHIP, pb)
    d = _backward_features(h2, dims, 5, 1.0, G)
    assert cc.same_bits(gu, d[0]) and all(cc.same_bits(x, y) for x, y in zip(gf, d[2]))
    h.close(), h2.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_handle_usable(po, wl):
    import torch
    pb = wl.slam_problem(2000, seed=4)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    L = pkg.lib()
    g = torch.zeros((2000, 2), device="cuda")
    gu = torch.zeros((2000, 2), device="cuda")
    gf = [torch.zeros((2000, 2), device="cuda") for _ in range(2)]
    host = np.zeros((2000, 2), np.float32)
    hl, small = hip_malloc(64)
    vp = C.c_void_p

    def arr(*ps):
        return (vp * 2)(*ps)
    good = arr(vp(gf[0].data_ptr()), vp(gf[1].data_ptr()))
    try:
        for args in ((1, 1.0, None, vp(gu.data_ptr()), None, good),                              # no dL/dQ
                     (1, 1.0, vp(host.ctypes.data), vp(gu.data_ptr()), None, good),             # pageable host memory
                     (1, 1.0, vp(g.data_ptr()), vp(host.ctypes.data), None, good),
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, arr(vp(gf[0].data_ptr()), vp(host.ctypes.data))),
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, arr(small, None)),     # undersized
                     (-1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, good),                # n_iterations < 0
                     (1, float("nan"), vp(g.data_ptr()), vp(gu.data_ptr()), None, good),
                     (1, float("inf"), vp(g.data_ptr()), vp(gu.data_ptr()), None, good)):
            assert L.lccrf_inference_backward_features(h.h, *args) == -1, args
        h0 = pkg.DenseCRFHIP(2000, 2)                            # no unary yet
        assert L.lccrf_inference_backward_features(h0.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, None) == -5
        h0.close()
    finally:
        hl.hipFree(small)
    o = cc.setup(po.OracleCRF, pb)                               # still usable
    h.inference(5, True)
    o.inference_native(5, True)
    assert cc.same_bits(h.probability(), o.probability())
    torch.cuda.synchronize()
    h.inference_backward_features_device(5, 1.0, g.data_ptr(), gu.data_ptr(), None, [t.data_ptr() for t in gf])
    h.synchronize()
    assert np.all(gu.cpu().numpy() == 0) and all(np.all(t.cpu().numpy() == 0) for t in gf)      # dL/dQ = 0
    h.close()
    # the batch entry point: the same checks
    fr = bc.slam_frames({"slam": np.load(os.path.join(os.path.dirname(__file__), "golden", "slam.npz"))}, wl, Ns=(5, 1000))
    b = fr.batch()
    G = dev(np.zeros((2, fr.maxN, 2), np.float32))
    gub = torch.zeros((2, fr.maxN, 2), device="cuda")
    gfb = [torch.zeros((2, fr.maxN, 2), device="cuda") for _ in range(2)]
    goodb = arr(vp(gfb[0].data_ptr()), vp(gfb[1].data_ptr()))
    hostb = np.zeros((2, fr.maxN, 2), np.float32)
    for args in ((1, 1.0, None, vp(gub.data_ptr()), None, goodb),
                 (1, 1.0, vp(G.data_ptr()), vp(gub.data_ptr()), None, arr(vp(hostb.ctypes.data), None)),
                 (-1, 1.0, vp(G.data_ptr()), vp(gub.data_ptr()), None, goodb),
                 (1, float("nan"), vp(G.data_ptr()), vp(gub.data_ptr()), None, goodb)):
        assert L.lccrf_batch_inference_backward_features(b.h, *args, None) == -1, args
    nb = fr.batch(build=False)
    assert L.lccrf_batch_inference_backward_features(nb.h, 5, 1.0, vp(G.data_ptr()), vp(gub.data_ptr()), None, goodb, None) == -5
    nb.close()
    b.inference_backward_features_device(5, 1.0, G.data_ptr(), gub.data_ptr(), None, [t.data_ptr() for t in gfb])
    b.synchronize()
    assert all(np.all(t.cpu().numpy() == 0) for t in gfb)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "nt:d2-5-3_L9"])
def test_torch_mean_field_features_matches_the_checker(po, wl, golden, name):
    """mean_field_features: unary, features and weights at once against the checker (same bar), Q against the handle's bits"""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    T, relax = 5, 0.7
    s = gset.features(po, wl, golden, name, T, relax)            # (the setting of test_feature_gradients_match_the_checker)
    pb, G = s["pb"], s["G"]
    U, w = cc.setup(po.OracleCRF, pb).unary(), gs.weights(pb)
    u = torch.from_numpy(U.astype(np.float32)).cuda().requires_grad_(True)
    wt = torch.tensor(w, dtype=torch.float32, requires_grad=True)
    fs = [torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda().requires_grad_(True) for f, _ in pb["kernels"]]
    q = ag.mean_field_features(u, fs, wt, T, relax)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.inference(T, False, relax)
    assert cc.same_bits(q.detach().cpu().numpy(), h.probability())
    h.close()
    q.backward(torch.from_numpy(G.astype(np.float32)).cuda())
    torch.cuda.synchronize()
    s["ref"].check({"dL/df%d" % k: f.grad.cpu().numpy() for k, f in enumerate(fs)})
    s["ref_1c"].check({"dL/dU": u.grad.cpu().numpy(), "dL/dw": wt.grad.numpy()})


@pytest.mark.gpu
def test_learned_kernel_crf_chain_rule_and_fit(po, wl):
    """LearnedKernelCRF: log_sd.grad is the chain rule applied to the checker's dL/df (d f / d log_sd = -f; same bar, with the
    columns of a group summed), and 20 Adam steps on a slam_problem(2000) whose features were built with wrong bandwidths end
    below the first step's loss (no rate is promised)."""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    p = wl.TUM3
    pb = wl.slam_problem(2000, seed=31)
    fr = pb["frame"]
    raw = [np.stack([fr["obs"], fr["err"]], 1).astype(np.float32), fr["uv"].astype(np.float32)]
    sd_true = [[p["stdev_beta"], p["stdev_alpha"]], [p["point2d_stdev"]]]
    groups = [None, [[0, 1]]]
    w = [p["w1"] / 10, p["w2"] / 10]
    o = cc.setup(po.OracleCRF, pb)
    U32 = o.unary()
    U = torch.from_numpy(U32).cuda()
    layer = ag.LearnedKernelCRF(raw, sd_true, w, groups=groups, n_iterations=5)
    # chain rule against the checker at the layer's own features
    G = np.random.default_rng(8).standard_normal((pb["N"], 2))
    feats = [f.detach().cpu().numpy() for f in layer.features()]
    pbl = dict(pb, kernels=[(f, np.float32(x)) for f, x in zip(feats, w)])
    ol, lats, Ul = _checker(po, pbl)
    (layer(U) * torch.from_numpy(G.astype(np.float32)).cuda()).sum().backward()
    _, _, ref_f, _ = mff.feature_gradients(Ul, np.array(w), lats, 5, 1.0, G)
    _, _, f32_f, _ = mff.feature_gradients(Ul, np.array(w), lats, 5, 1.0, G, dtype=torch.float32)

    def chain(gf):
        return [-(gf[0] * feats[0].astype(np.float64)).sum(0), np.array([-(gf[1] * feats[1].astype(np.float64)).sum()])]
    for k, (got, r, s) in enumerate(zip([x.grad.cpu().numpy() for x in layer.log_sd], chain(ref_f), chain(f32_f))):
        gs.assert_within_bar("log_sd.grad of term %d (grad %s checker %s)" % (k, got, r), got, r, s)
    # fit: targets from the true bandwidths, a start at wrong ones
    with torch.no_grad():
        target = layer(U).clone()
    wrong = ag.LearnedKernelCRF(raw, [[2.5, 1.0], [30.0]], w, groups=groups, n_iterations=5)
    opt = torch.optim.Adam(list(wrong.log_sd.parameters()), lr=0.05)
    losses = []
    for _ in range(20):
        loss = ((wrong(U) - target) ** 2).sum()
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        final = ((wrong(U) - target) ** 2).sum().item()
    print("losses", losses, "final", final, "sd", wrong.sd())
    assert final < losses[0], (losses, final)

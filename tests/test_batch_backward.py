"""Gradients of a batch's inference (include/lccrf.h section 2c) and the batched torch layer (lc-crf-slam_amd/autograd.py).

CPU: the new symbols.  GPU: lccrf_batch_inference_backward frame by frame against lccrf_inference_backward on a handle of that
frame (bit for bit) and against the float64 checker, its state, determinism, rebinding, locality-mode and argument contracts,
lccrf_batch_set_pairwise_weight / lccrf_batch_set_unary_device against freshly bound batches, and the torch layer."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
from abi_support import assert_declared_exported_bound, dev, hip_malloc, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_batch_set_pairwise_weight", "lccrf_batch_set_unary_device", "lccrf_batch_inference_backward")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_batch_backward_symbols_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3
    for m in ("set_pairwise_weight", "set_unary_device", "inference_backward_device"):
        assert hasattr(pkg.BatchCRF, m), m
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    assert callable(ag.mean_field_batch) and issubclass(ag.BatchMeanFieldCRF, __import__("torch").nn.Module)


def test_batch_backward_rejects_a_null_handle(lib):
    assert lib.lccrf_batch_set_pairwise_weight(None, 0, 1.0) == -1
    assert lib.lccrf_batch_set_unary_device(None, None) == -1
    assert lib.lccrf_batch_inference_backward(None, 1, 1.0, None, None, None, None) == -1


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _check_parity(fr, handles, gu, gw, T, relax, G):
    """every frame: the handle's bits; zero rows beyond its points; a frame of 0 points all zeros"""
    for f, n in enumerate(fr.N):
        assert np.all(gu[f, n:] == 0), "frame %d: rows beyond n_points not 0" % f
        if n == 0:
            assert np.all(gw[f] == 0), "frame %d (0 points): weight gradient not 0" % f
            continue
        hu, hw = gs.backward(handles[f], T, relax, G[f, :n], fr.K)
        assert cc.same_bits(gu[f, :n], hu), "frame %d (N=%d) T=%d relax=%g: dL/dU differs from the handle's" % (f, n, T, relax)
        assert cc.same_bits(gw[f], hw), "frame %d (N=%d) T=%d relax=%g: dL/dw %s, handle %s" % (f, n, T, relax, gw[f], hw)


def _probs_valid(q, N):
    return [q[f, :n].copy() for f, n in enumerate(N)]


def _same_valid(a, b, N):
    return all(cc.same_bits(a[f, :n], b[f, :n]) for f, n in enumerate(N))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["slam", "generic", "K8_L9", "K8_L33", "K8_L64"])
def test_every_frame_has_the_bits_of_its_handle(wl, golden, kind):
    """every frame of a ragged batch (0-point frames among them) gets the bits of a handle of its own points; the K8_L* kinds:
    eight terms of d = 1 .. 8 at 9, 33 and 64 labels (the backward's lane groups of 4 and 16 lanes, its partials at K = 8)"""
    if kind == "slam":
        fr = bc.slam_frames(golden, wl)
    elif kind == "generic":
        fr = bc.generic_frames(wl)
    else:
        fr = bc.label_frames(int(kind[4:]), (300, 0, 1100, 77, 650), seed=400)
    assert fr.K == {"slam": 2, "generic": 1}.get(kind, 8)
    b = fr.batch()
    handles = {f: fr.handle(f) for f, n in enumerate(fr.N) if n}
    for T in (0, 1, 5, 10):
        for relax in (1.0, 0.7):
            G = fr.grad_prob(100 * T + int(relax * 10))
            gu, gw = gs.batch_backward(b, T, relax, G, fr.K)
            _check_parity(fr, handles, gu, gw, T, relax, G)
            if T == 0:
                assert np.all(gw == 0)
    for h in handles.values():
        h.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("relax", gset.RELAX_SET)
def test_batch_gradients_match_the_checker(po, wl, golden, relax):
    """every frame of more than 0 points under the bars of grad_support.assert_within_bar (L2 and worst row) and, as before them,
    the L2 errors of dL/dU and dL/dw under GRAD_TOL itself, dL/dw against a floor of 1e-6 |dL/dQ|"""
    fr = bc.slam_frames(golden, wl, Ns=gset.BATCH_FRAMES)
    b = fr.batch()
    T = gset.BATCH_T
    G = fr.grad_prob(gset.BATCH_GRAD_SEED)
    gu, gw = gs.batch_backward(b, T, relax, G, fr.K)
    for f, n in enumerate(fr.N):
        if n == 0:
            continue
        r = gset.batch_frame(po, fr, G, f, T, relax, "frame N=%d" % n, "batch:slam")["ref"]
        r.check({"dL/dU": gu[f, :n], "dL/dw": gw[f]})
        eu = gs.rel(gu[f, :n], r.ref["dL/dU"], r.floors["dL/dU"])
        ew = gs.rel(gw[f], r.ref["dL/dw"], r.floors["dL/dU"])
        assert eu <= gs.GRAD_TOL and ew <= gs.GRAD_TOL, (eu, ew)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["engine1", "engine2", "pending_run"])
def test_backward_leaves_what_inference_leaves(wl, golden, how):
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000, 1500))
    T, relax = 5, 0.7
    b = fr.batch()
    b.set_engine(1 if how == "engine1" else 2 if how == "engine2" else 0)
    b.inference(T, False, relax)
    q_ref = b.probability()
    if how == "pending_run":
        b.run(T, True, relax)                                   # one launch per frame, left pending: the backward settles it
    G = fr.grad_prob(3)
    gs.batch_backward(b, T, relax, G, fr.K)
    assert _same_valid(b.probability(), q_ref, fr.N)
    if how == "engine2":
        assert b.engine() == 2
    b.inference(T, True, relax)                                 # ... and the next inference is unchanged
    assert _same_valid(b.probability(), q_ref, fr.N)
    b.close()


@pytest.mark.gpu
def test_backward_is_deterministic_and_survives_rebinding(wl, golden):
    big = bc.slam_frames(golden, wl, Ns=(2002, 2002))
    b = big.batch()
    G = big.grad_prob(11)
    a1 = gs.batch_backward(b, 5, 1.0, G, 2)
    a2 = gs.batch_backward(b, 5, 1.0, G, 2)
    assert cc.same_bits(a1[0], a2[0]) and cc.same_bits(a1[1], a2[1])
    # the same batch rebound to fewer points per frame: stale rows of the larger frames stay in its area and must not be read
    small = bc.slam_frames(golden, wl, Ns=(1001, 5))
    small = bc.Frames(small.probs, small.w, max_points=2002)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    handles = {f: small.handle(f) for f in range(2)}
    for T, relax in ((5, 1.0), (10, 0.7), (1, 1.0)):
        G = small.grad_prob(T)
        gu, gw = gs.batch_backward(b, T, relax, G, 2)
        _check_parity(small, handles, gu, gw, T, relax, G)
    for h in handles.values():
        h.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["engine1", "engine2", "run"])
def test_batch_set_pairwise_weight_equals_a_fresh_batch(wl, how):
    rng = np.random.default_rng(5)
    fr = bc.Frames([wl.slam_problem(int(n), seed=60 + i) for i, n in enumerate(rng.integers(513, 2049, 64))], [1.0, 2.0], max_points=2048)
    new = [7.25, 21.5]
    b, fresh = fr.batch(), fr.batch(weights=new)
    for x in (b, fresh):
        if how != "run":
            x.set_engine(1 if how == "engine1" else 2)

    def go(x):
        if how == "run":
            x.run(5, True)
        else:
            x.inference(5, True)
        return x.probability(), x.map()
    for _ in range(2):                                          # the second inference on engine 2 runs from prepared records
        go(b)
    b.set_pairwise_weight(0, new[0])
    b.set_pairwise_weight(1, new[1])
    for _ in range(2):
        qb, mb = go(b)
        qf, mf_ = go(fresh)
        assert _same_valid(qb, qf, fr.N) and all(np.array_equal(mb[f, :n], mf_[f, :n]) for f, n in enumerate(fr.N))
    b.close(), fresh.close()


@pytest.mark.gpu
def test_batch_set_unary_device_equals_a_fresh_batch(wl):
    import torch
    # inputs from labels, then raw unaries
    probs = [wl.slam_problem(n, seed=80 + i) for i, n in enumerate((1500, 700, 2000))]
    fr = bc.Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]])
    b = pkg.BatchCRF(3, fr.maxN, 2, fr.dims, fr.w)
    lab = np.full((3, fr.maxN), -1, np.int16)
    for f, pb in enumerate(probs):
        lab[f, :pb["N"]] = pb["label"]
    b.set_inputs_host(fr.N, fr.feats, label=lab, conf=probs[0]["conf"])
    b.build()
    b.inference(5, True)
    U1 = fr.U + np.random.default_rng(1).standard_normal(fr.U.shape).astype(np.float32)
    d = dev(U1)
    torch.cuda.synchronize()
    b.set_unary_device(d.data_ptr())
    del d                                                        # copied: the caller's array may go
    torch.cuda.synchronize()
    fresh = bc.Frames(probs, fr.w)
    fresh.U = U1
    f2 = fresh.batch()
    for x in (b, f2):
        x.inference(5, True, 0.7)
    assert _same_valid(b.probability(), f2.probability(), fr.N)
    b.run(5, True)
    f2.run(5, True)
    assert _same_valid(b.probability(), f2.probability(), fr.N)
    b.close(), f2.close()


@pytest.mark.gpu
def test_locality_mode_frame_has_the_bits_of_its_handle(wl):
    import torch
    fr = bc.Frames([wl.slam_problem(9000, seed=90), wl.slam_problem(1200, seed=91)], [wl.TUM3["w1"], wl.TUM3["w2"]])
    b = fr.batch()
    b.inference(5, True)
    assert b.locality_mode()[0], "the 9000-point frame should be in locality mode"
    handles = {f: fr.handle(f) for f in range(2)}
    for T, relax in ((5, 1.0), (2, 0.7)):
        G = fr.grad_prob(T)
        gu, gw = gs.batch_backward(b, T, relax, G, 2)
        _check_parity(fr, handles, gu, gw, T, relax, G)
    # set_unary_device on a batch whose lattices were built in locality mode
    U1 = fr.U * np.float32(0.5)
    b.build()
    b.inference(5, True)
    d = dev(U1)
    torch.cuda.synchronize()
    b.set_unary_device(d.data_ptr())
    b.inference(5, True)
    fresh = bc.Frames(fr.probs, fr.w)
    fresh.U = U1
    f2 = fresh.batch()
    f2.inference(5, True)
    assert _same_valid(b.probability(), f2.probability(), fr.N)
    for h in handles.values():
        h.close()
    b.close(), f2.close()


@pytest.mark.gpu
def test_batch_backward_argument_checks_leave_the_batch_usable(wl, golden):
    import torch
    fr = bc.slam_frames(golden, wl, Ns=(1000, 5, 2000))
    b = fr.batch()
    G = fr.grad_prob(21)
    ref = gs.batch_backward(b, 5, 1.0, G, 2)
    q_ref = b.probability()
    L = pkg.lib()
    shape = (3, fr.maxN, 2)
    g, gu, gw = dev(G), torch.zeros(shape, device="cuda"), torch.zeros((3, 2), device="cuda")
    host = np.zeros(shape, np.float32)
    hl, small = hip_malloc(64)
    _, small4 = hip_malloc(4)
    vp = C.c_void_p
    try:
        for args in ((5, 1.0, None, vp(gu.data_ptr()), None),
                     (5, 1.0, vp(g.data_ptr()), None, None),
                     (5, 1.0, vp(host.ctypes.data), vp(gu.data_ptr()), None),     # pageable host memory
                     (5, 1.0, small, vp(gu.data_ptr()), None),                    # too short
                     (5, 1.0, vp(g.data_ptr()), small, None),
                     (5, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), small4),       # [F][K] too short
                     (-1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None),
                     (5, float("nan"), vp(g.data_ptr()), vp(gu.data_ptr()), None)):
            assert L.lccrf_batch_inference_backward(b.h, *args, None) == -1, args
        assert L.lccrf_batch_set_pairwise_weight(b.h, 2, 1.0) == -1
        assert L.lccrf_batch_set_unary_device(b.h, vp(host.ctypes.data)) == -1
        assert L.lccrf_batch_set_unary_device(b.h, small) == -1
        # no build for these inputs: LCCRF_E_STATE, and nothing is touched
        nb = fr.batch(build=False)
        assert L.lccrf_batch_inference_backward(nb.h, 5, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, None) == -5
        nb.close()
        empty = pkg.BatchCRF(3, fr.maxN, 2, fr.dims, fr.w)
        assert L.lccrf_batch_set_unary_device(empty.h, vp(g.data_ptr())) == -5
        empty.close()
    finally:
        hl.hipFree(small)
        hl.hipFree(small4)
    torch.cuda.synchronize()
    assert _same_valid(b.probability(), q_ref, fr.N)
    again = gs.batch_backward(b, 5, 1.0, G, 2)
    assert cc.same_bits(again[0], ref[0]) and cc.same_bits(again[1], ref[1])
    handles = {f: fr.handle(f) for f in range(3)}
    _check_parity(fr, handles, again[0], again[1], 5, 1.0, G)
    for h in handles.values():
        h.close()
    b.close()


@pytest.mark.gpu
def test_mean_field_batch_matches_the_c_abi_and_streams(wl, golden):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    fr = bc.slam_frames(golden, wl, Ns=(1200, 0, 2000, 7))
    T, relax = 5, 0.7
    ref = fr.batch()
    ref.inference(T, False, relax)
    q_ref = ref.probability()
    G = np.nan_to_num(fr.grad_prob(31), nan=0.0)
    ref_u, ref_w = gs.batch_backward(ref, T, relax, G, 2)
    ref.close()
    b = fr.batch()

    def run(stream):
        with torch.cuda.stream(stream):
            u = torch.from_numpy(fr.U).cuda().requires_grad_(True)
            w = torch.tensor(fr.w, requires_grad=True)
            q = ag.mean_field_batch(b, u, w, T, relax)
            q.backward(torch.from_numpy(G).cuda())
            torch.cuda.current_stream().synchronize()
            return q.detach().cpu().numpy(), u.grad.cpu().numpy(), w.grad.numpy()

    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        q, gu, gw = run(stream)
        assert _same_valid(q, q_ref, fr.N)
        assert all(np.all(q[f, n:] == 0) for f, n in enumerate(fr.N))
        assert cc.same_bits(gu, ref_u)
        want = ref_w.astype(np.float64).sum(0)
        assert np.all(np.abs(gw - want) <= 1e-6 * np.abs(want)), (gw, want)
    b.close()


@pytest.mark.gpu
def test_fitting_the_weights_over_many_frames_lowers_the_nll(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    rng = np.random.default_rng(17)
    probs = [wl.slam_problem(int(n), seed=200 + i) for i, n in enumerate(rng.integers(300, 1200, 64))]
    fr = bc.Frames(probs, [1.0, 3.0])
    layer = ag.BatchMeanFieldCRF(fr.N, fr.feats, fr.w, n_iterations=5)
    U = torch.from_numpy(fr.U).cuda()
    truth = np.zeros((64, fr.maxN), np.int64)
    live = np.zeros((64, fr.maxN), bool)
    for f, pb in enumerate(probs):
        truth[f, :pb["N"]] = pb["truth"]
        live[f, :pb["N"]] = True
    truth, live = torch.from_numpy(truth).cuda(), torch.from_numpy(live).cuda()

    def nll():
        q = layer(U)
        p = q.gather(2, truth[:, :, None])[:, :, 0].clamp_min(1e-12)
        return -(torch.log(p) * live).sum() / live.sum()
    opt = torch.optim.Adam(layer.parameters(), lr=0.3)
    losses = []
    for _ in range(30):
        loss = nll()
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    final = nll().item()
    layer.close()
    print("NLL %.4f -> %.4f, weights %s" % (losses[0], final, layer.weights.detach().numpy()))
    assert final < losses[0], (losses, final)

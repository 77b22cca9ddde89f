"""Gradients of a batch's inference for learnt models (include/lccrf.h section 2h: lccrf_batch_inference_backward_all) and the batched
torch layer over them (lc-crf-slam_amd/autograd.py: mean_field_batch_compat, BatchCompatMeanFieldCRF).

CPU: the symbol, the ABI version, the NULL handle, the Python methods and layers, the host restatement of k_sum_frames' order.  GPU:
every frame of a batch against lccrf_inference_backward_all on a handle holding that frame, bit for bit -- under every setting of a
learnt model, at the label counts of the sweep's lane shapes, at the chunk cap of k_compat_bwd -- d_grad_model against the restated
ordered sum, the float64 checker under the project's bars, the contracts of section 2c, and the layer.  What the tests share is in
tests/batch_learned_cases.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import batch_learned_cases as bl
import crf_cases as cc
import gradient_settings as gset
import joint_checker as jc
import normalization_checker as nc
import test_fused_general as fg
from abi_support import assert_declared_exported_bound, dev, hip_malloc, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
F32 = np.float32
E_INVALID, E_STATE = -1, -5
SYMBOL = "lccrf_batch_inference_backward_all"


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, (SYMBOL,))
    assert lib.lccrf_abi_version() == 3                           # added without a step: callers probe by symbol


def test_a_null_batch_is_refused(lib):
    assert lib.lccrf_batch_inference_backward_all(None, 1, 1.0, None, None, None, None, None, None, None) == E_INVALID
    assert b"NULL" in lib.lccrf_last_error()


def test_python_methods_and_layers_exist():
    import torch
    assert callable(getattr(pkg.BatchCRF, "inference_backward_all_device", None))
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    assert callable(ag.mean_field_batch_compat) and issubclass(ag.BatchCompatMeanFieldCRF, torch.nn.Module)
    assert callable(ag.mean_field_batch) and issubclass(ag.BatchMeanFieldCRF, torch.nn.Module)      # ... and the Potts layer stays


def test_the_restated_sum_is_a_plain_loop_of_float32_adds_in_frame_order():
    """values whose float32 sum depends on the order: the restatement must be the left-to-right one, entry by entry, and differ from
    the pairwise and the float64 sums it is not"""
    x = np.array([[1.0, 1e8], [1e8, 1.0], [-1e8, 1.0], [3e-8, -1e8]], F32)
    want = []
    for j in range(2):
        s = x[0, j]
        for f in range(1, 4):
            s = F32(s + x[f, j])
        want.append(s)
    got = bl.sum_frames_host(x)
    assert got.dtype == np.float32 and cc.same_bits(got, np.array(want, F32))
    assert got[0] == F32(3e-8) and got[1] == 0.0                  # ((1 + 1e8) - 1e8) + 3e-8; ((1e8 + 1) + 1) - 1e8: the 1s are lost
    assert got[1] != F32(x[:, 1].astype(np.float64).sum())        # (the float64 sum keeps them: 2)
    assert cc.same_bits(bl.sum_frames_host(np.zeros((0, 3), F32)), np.zeros(3, F32))
    assert np.signbit(bl.sum_frames_host(np.array([[-0.0]], F32)))[0]          # one frame: its own bits, not 0 + x
    rng = np.random.default_rng(1)
    big = rng.standard_normal((bl.SUM_TILE + 6, 2, 3, 3)).astype(F32)
    got = bl.sum_frames_host(big)
    s = big[0, 1, 2, 0]
    for f in range(1, big.shape[0]):
        s = F32(s + big[f, 1, 2, 0])
    assert got.shape == (2, 3, 3) and got[1, 2, 0].view(np.int32) == s.view(np.int32)
    m = bl.model_of(big[:, :, 0, 0], big)
    assert m.shape == (2 + 2 * 9,) and cc.same_bits(m[2:], got.reshape(-1))


# ---- GPU 1: handle bits, frame by frame ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sname", bl.SETTINGS)
def test_every_frame_has_the_bits_of_its_handle_under_every_setting(po, wl, golden, sname):
    """a ragged batch whose max_points lies 7 beyond its largest frame: the batch's chunk count of k_compat_bwd is no frame's own"""
    fr = bl.ragged(golden, wl)
    assert tuple(fr.N) == bl.RAGGED and fr.maxN == 2007
    modes, mats, w = bl.setting(fr, sname, po)
    features = all(m == nc.AFTER for m in modes)                  # (section 1g: dL/df under a mode is refused)
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    handles = {f: bl.handle(fr, f, modes, mats, w) for f, n in enumerate(fr.N) if n}
    for T in (0, 1, 5):
        for relax in (1.0, 0.7):
            G = fr.grad_prob(100 * T + int(relax * 10))
            out = bl.backward_all(b, fr, T, relax, G, features=features)
            bl.check_frames(out, fr, handles, T, relax, G, features, sname)
            if T == 0:
                assert np.all(out["gm"] == 0) and np.all(out["gw"] == 0) and all(np.all(a == 0) for a in out["gf"] if features)
    for h in handles.values():
        h.close()
    b.close()


# ---- GPU 2: label counts and lane shapes ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 9, 33, 64])
def test_label_counts_and_lane_shapes(wl, L):
    """eight terms with dense matrices: R = 256 / L rows per tile, the L | 1 stride, 16 entries of mu per lane at L = 64"""
    fr = bc.label_frames(L, (300, 0, 1100, 77, 650), seed=800 + L)
    fr = bc.Frames(fr.probs, fr.w, max_points=int(fr.N.max()) + bl.SLACK)
    modes, mats = [nc.AFTER] * fr.K, jc.dense(fr.K, L)
    b = fr.batch()
    bl.apply(b, modes, mats)
    handles = {f: bl.handle(fr, f, modes, mats, None) for f, n in enumerate(fr.N) if n}
    for T, relax in ((1, 1.0), (5, 0.7)):
        G = fr.grad_prob(L + T)
        out = bl.backward_all(b, fr, T, relax, G, features=True)
        bl.check_frames(out, fr, handles, T, relax, G, True, "L=%d" % L)
    for h in handles.values():
        h.close()
    b.close()


# ---- GPU 3: the chunk cap ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_chunk_cap_and_a_locality_mode_frame(wl):
    """33000 > 128 * 256 points: that frame's chunk count is clamped to 128, the 300-point frame's is 2; the large frame is in locality
    mode and is rebuilt the plain way"""
    probs = [fg._terms(wl.slam_problem(n, seed=900 + i), [1]) for i, n in enumerate((33000, 300))]
    fr = bc.Frames(probs, [wl.TUM3["w2"]], max_points=33000 + bl.SLACK)
    modes, mats = [nc.AFTER], jc.dense(1, 2)
    b = fr.batch()
    bl.apply(b, modes, mats)
    b.inference(1, True)
    assert b.locality_mode()[0], "the 33000-point frame should be in locality mode"
    handles = {f: bl.handle(fr, f, modes, mats, None) for f in range(2)}
    G = fr.grad_prob(3)
    out = bl.backward_all(b, fr, 1, 1.0, G)
    bl.check_frames(out, fr, handles, 1, 1.0, G, False, "chunk cap")
    assert np.abs(out["gm"]).min() > 0
    for h in handles.values():
        h.close()
    b.close()


# ---- GPU 4: the ordered sum ------------------------------------------------------------------------------------------------------
def _small_frames(wl, F, seed):
    Ns = [(5, 0, 33, 77, 1, 130)[i % 6] for i in range(F)]
    probs = [wl.slam_problem(n, seed=seed + i) if n else cc.empty_problem(2, [2, 2]) for i, n in enumerate(Ns)]
    return bc.Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]], max_points=137)


@pytest.mark.gpu
@pytest.mark.parametrize("F,max_frames", [(1, 1), (5, 8), (bl.SUM_TILE + 6, bl.SUM_TILE + 6), (2 * bl.SUM_TILE, 2 * bl.SUM_TILE + 3)])
def test_the_model_gradient_is_the_ordered_sum_of_the_frames(wl, F, max_frames):
    """d_grad_model against the host restatement applied to the per-frame arrays of the same call, and the same bits with the
    per-frame pointers NULL (the batch's area holds them); frames beyond n_frames are never read"""
    fr = _small_frames(wl, F, 1000)
    modes, mats = [nc.SYMMETRIC, nc.AFTER], jc.dense(2, 2)
    b = fr.batch(max_frames=max_frames)
    bl.apply(b, modes, mats)
    G = fr.grad_prob(F)
    full = bl.backward_all(b, fr, 5, 0.7, G)
    want = bl.model_of(full["gw"], full["gm"])
    assert np.isfinite(want).all() and np.abs(want).min() > 0
    assert cc.same_bits(full["model"], want), (full["model"], want)
    for keep in ({}, dict(weights=False), dict(compat=False), dict(weights=False, compat=False, unary=False)):
        out = bl.backward_all(b, fr, 5, 0.7, G, **keep)
        assert cc.same_bits(out["model"], want), (keep, out["model"], want)
        assert np.isnan(out["gw"]).all() == ("weights" in keep) and np.isnan(out["gm"]).all() == ("compat" in keep), keep
    b.close()


# ---- GPU 5: the float64 checker --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", nc.MODES, ids=[nc.MODE_NAMES[m] for m in nc.MODES])
def test_batch_gradients_match_the_float64_checker_under_every_mode(po, wl, golden, mode):
    """every term in `mode` with dense matrices, the setting and the bars of tests/test_normalization.py (gradient_settings.normalization:
    10 x the float32 checker's error, capped at BAR_CAP): the 1001-point frame those bars were found for, at both ends of a batch with
    a 0-point frame between them"""
    T, relax = 5, 0.7
    s = gset.normalization(po, wl, golden, "slam1001:s38", mode, T, relax)
    pb, n = s["pb"], s["pb"]["N"]
    fr = bc.Frames([pb, cc.empty_problem(2, [2, 2]), pb], [float(x) for x in s["w"]], max_points=n + bl.SLACK)
    fr.U[0, :n] = fr.U[2, :n] = s["U"]                            # (the unary the reference was computed for)
    b = fr.batch()
    bl.apply(b, s["modes"], s["mats"])
    G = np.full((3, fr.maxN, 2), np.nan, F32)
    G[0, :n] = G[2, :n] = s["G"]
    out = bl.backward_all(b, fr, T, relax, G)
    for f in (0, 2):
        s["ref"].check({"dL/dU": out["gu"][f, :n], "dL/dw": out["gw"][f], "dL/dmu": out["gm"][f]})
    assert np.all(out["gu"][1] == 0) and np.all(out["gw"][1] == 0) and np.all(out["gm"][1] == 0)
    assert cc.same_bits(out["model"], bl.model_of(out["gw"], out["gm"]))
    b.close()


# ---- GPU 6: contracts ------------------------------------------------------------------------------------------------------------
def _valid(q, N):
    return [q[f, :n].copy() for f, n in enumerate(N)]


def _same_valid(a, b, N):
    return all(cc.same_bits(a[f, :n], b[f, :n]) for f, n in enumerate(N))


def _same_out(a, b):
    return all(cc.same_bits(a[k], b[k]) for k in ("gu", "gw", "gm", "model")) and all(cc.same_bits(x, y) for x, y in zip(a["gf"], b["gf"]))


@pytest.mark.gpu
def test_deterministic_and_leaves_what_inference_leaves(po, wl, golden):
    fr = bl.ragged(golden, wl, Ns=(5, 1000, 0, 2000, 257))
    modes, mats, w = bl.setting(fr, "mixed", po)
    T, relax = 5, 0.7
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    b.inference(T, True, relax)
    q_ref, m_ref = b.probability(), b.map()
    G = fr.grad_prob(3)
    a1 = bl.backward_all(b, fr, T, relax, G)
    assert _same_valid(b.probability(), q_ref, fr.N) and np.array_equal(b.map(), m_ref)      # Q as inference leaves it; the labels untouched
    a2 = bl.backward_all(b, fr, T, relax, G)
    assert _same_out(a1, a2)
    b.run(T, True, relax)                                       # a run left pending: the backward settles it
    a3 = bl.backward_all(b, fr, T, relax, G)
    assert _same_out(a1, a3) and _same_valid(b.probability(), q_ref, fr.N)
    b.inference(T, True, relax)                                 # ... and the next inference is unchanged
    assert _same_valid(b.probability(), q_ref, fr.N) and np.array_equal(b.map(), m_ref)
    b.close()


@pytest.mark.gpu
def test_every_output_alone_has_the_bits_of_the_full_call(po, wl, golden):
    fr = bl.ragged(golden, wl, Ns=(257, 0, 1001, 5))
    modes, mats, w = bl.setting(fr, "matrices", po)
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    G = fr.grad_prob(8)
    full = bl.backward_all(b, fr, 5, 1.0, G, features=True)
    none = dict(unary=False, weights=False, features=False, compat=False, model=False)
    for one, key in (("unary", "gu"), ("weights", "gw"), ("features", "gf"), ("compat", "gm"), ("model", "model")):
        out = bl.backward_all(b, fr, 5, 1.0, G, **dict(none, **{one: True}))
        for k in ("gu", "gw", "gm", "model"):
            assert cc.same_bits(out[k], full[k]) if k == key else np.isnan(out[k]).all(), (one, k)
        for x, y in zip(out["gf"], full["gf"]):
            assert cc.same_bits(x, y) if key == "gf" else np.isnan(x).all(), one
    b.close()


@pytest.mark.gpu
def test_state_and_argument_checks_leave_the_batch_as_it_was(po, wl, golden, lib):
    import torch
    fr = bl.ragged(golden, wl, Ns=(300, 5, 1001))
    modes, mats, w = bl.setting(fr, "mixed", po)
    F, K, L = 3, 2, 2
    vp = C.c_void_p
    g = dev(np.nan_to_num(fr.grad_prob(2)))
    gu = torch.zeros((F, fr.maxN, L), device="cuda")
    gw, gm, md = torch.zeros((F, K), device="cuda"), torch.zeros((F, K, L, L), device="cuda"), torch.zeros(K * (1 + L * L), device="cuda")
    gf = [torch.zeros((F, fr.maxN, 2), device="cuda") for _ in range(K)]
    gfp = (vp * K)(*[vp(t.data_ptr()) for t in gf])
    call = lambda h, T, relax, feats=None: lib.lccrf_batch_inference_backward_all(
        h, T, C.c_float(relax), vp(g.data_ptr()), vp(gu.data_ptr()), vp(gw.data_ptr()), feats, vp(gm.data_ptr()), vp(md.data_ptr()), None)
    nb = fr.batch(build=False)                                   # before lccrf_batch_build
    bl.apply(nb, modes, mats, w)
    assert call(nb.h, 5, 1.0) == E_STATE
    nb.close()
    b = fr.batch()
    bl.apply(b, modes, mats, w)
    b.inference(3, True, 1.0)
    q, m = b.probability(), b.map()
    assert call(b.h, 5, 1.0, gfp) == E_STATE                     # features under a mode
    assert b"AFTER" in lib.lccrf_last_error()
    assert call(b.h, -1, 1.0) == E_INVALID
    for bad in (float("nan"), float("inf")):
        assert call(b.h, 5, bad) == E_INVALID
    hl, short_model = hip_malloc(4 * (K * (1 + L * L) - 1))       # d_grad_model one float short
    _, one_frame = hip_malloc(4 * K * L * L)                      # d_grad_compat sized for one frame, as section 1e's
    try:
        for args in ((vp(g.data_ptr()), None, None, None, None, short_model), (vp(g.data_ptr()), None, None, None, one_frame, None),
                     (None, None, None, None, None, vp(md.data_ptr()))):
            assert lib.lccrf_batch_inference_backward_all(b.h, 5, C.c_float(1.0), *args, None) == E_INVALID, args
    finally:
        hl.hipFree(short_model)
        hl.hipFree(one_frame)
    torch.cuda.synchronize()
    for t in [gu, gw, gm, md] + gf:                               # nothing was written
        assert float(t.abs().max()) == 0.0
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), m)      # ... and the batch is intact
    b.inference(3, True, 1.0)
    assert b.engine() == 4 and cc.same_bits(b.probability(), q)
    # the old calls still refuse such a batch (tests/test_batch_general.py pins the same)
    with pytest.raises(pkg.LccrfError) as e1:
        b.inference_backward_device(3, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr())
    with pytest.raises(pkg.LccrfError) as e2:
        b.inference_backward_features_device(3, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [t.data_ptr() for t in gf])
    assert e1.value.code == e2.value.code == E_STATE
    torch.cuda.synchronize()
    assert float(gu.abs().max()) == 0.0 and float(gw.abs().max()) == 0.0
    assert call(b.h, 3, 1.0) == 0                                # the new call takes it
    b.synchronize()
    torch.cuda.synchronize()
    assert float(gu.abs().max()) > 0.0 and float(md.abs().min()) > 0.0
    b.close()


@pytest.mark.gpu
def test_a_batch_rebound_with_fewer_and_smaller_frames(po, wl, golden):
    """stale rows and stale partials of the larger frames stay in the batch's area and must not be read"""
    big = bl.ragged(golden, wl, Ns=(2000, 1001, 2000, 257))
    modes, mats, w = bl.setting(big, "matrices", po)
    b = big.batch()
    bl.apply(b, modes, mats, w)
    bl.backward_all(b, big, 5, 1.0, big.grad_prob(1))
    small = bl.ragged(golden, wl, Ns=(5, 256))
    small = bc.Frames(small.probs, small.w, max_points=big.maxN)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    handles = {f: bl.handle(small, f, modes, mats, w) for f in range(2)}
    for T, relax in ((5, 1.0), (1, 0.7)):
        G = small.grad_prob(T)
        out = bl.backward_all(b, small, T, relax, G, features=True)
        bl.check_frames(out, small, handles, T, relax, G, True, "rebound")
    for h in handles.values():
        h.close()
    b.close()


@pytest.mark.gpu
def test_a_potts_batch_gets_the_bits_of_section_2d(wl, golden):
    import torch
    fr = bl.ragged(golden, wl, Ns=(1001, 0, 5, 2000))
    b = fr.batch()
    G = fr.grad_prob(5)
    out = bl.backward_all(b, fr, 5, 0.7, G, features=True, compat=False, model=False)
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((4, 2), float("nan"), device="cuda")
    gf = [torch.full((4, fr.maxN, 2), float("nan"), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    b.inference_backward_features_device(5, 0.7, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [t.data_ptr() for t in gf])
    b.synchronize()
    torch.cuda.synchronize()
    assert cc.same_bits(out["gu"], gu.cpu().numpy()) and cc.same_bits(out["gw"], gw.cpu().numpy())
    assert all(cc.same_bits(x, t.cpu().numpy()) for x, t in zip(out["gf"], gf))
    b.run(5, True, 0.7)                                         # one launch per frame, left pending: the backward settles it
    again = bl.backward_all(b, fr, 5, 0.7, G, features=True, compat=False, model=False)
    assert _same_out(out, again)
    b.close()


# ---- GPU 7: the layer --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_batched_layer_sums_six_handle_layers_in_frame_order(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    Ns = (5, 77, 300, 256, 257, 130)
    probs = [wl.slam_problem(n, seed=1100 + i) for i, n in enumerate(Ns)]
    fr = bc.Frames(probs, [3.0, 5.0], max_points=300 + bl.SLACK)
    T, relax, modes = 5, 0.7, [nc.SYMMETRIC, nc.AFTER]
    mu = torch.tensor(np.stack(jc.dense(2, 2)))
    G = np.nan_to_num(fr.grad_prob(9))
    layer = ag.BatchCompatMeanFieldCRF(fr.N, fr.feats, fr.w, T, relax, n_labels=2, normalization=modes)
    assert [layer.batch.normalization(k) for k in range(2)] == modes
    assert torch.equal(layer.compat.detach(), torch.eye(2).repeat(2, 1, 1))      # starts from the Potts model
    layer.compat.data.copy_(mu)
    u = torch.from_numpy(fr.U).cuda().requires_grad_(True)
    layer(u).backward(torch.from_numpy(G).cuda())
    gws, gms = [], []
    for f, n in enumerate(Ns):
        one = ag.CompatMeanFieldCRF(n, 2, [ft[f, :n] for ft in fr.feats], fr.w, T, relax, normalization=modes)
        one.compat.data.copy_(mu)
        uf = torch.from_numpy(fr.U[f, :n]).cuda().requires_grad_(True)
        one(uf).backward(torch.from_numpy(G[f, :n]).cuda())
        assert cc.same_bits(u.grad[f, :n].cpu().numpy(), uf.grad.cpu().numpy()), f
        assert float(u.grad[f, n:].abs().max()) == 0.0
        gws.append(one.weights.grad.numpy().copy())
        gms.append(one.compat.grad.numpy().copy())
        one.close()
    assert cc.same_bits(layer.weights.grad.numpy(), bl.sum_frames_host(np.stack(gws)))
    assert cc.same_bits(layer.compat.grad.numpy(), bl.sum_frames_host(np.stack(gms)))
    # a few small steps against the gradient lower the loss every time: the signs are right (a smoke test, not a bar)
    truth = np.zeros((len(Ns), fr.maxN), np.int64)
    live = np.zeros((len(Ns), fr.maxN), bool)
    for f, pb in enumerate(probs):
        truth[f, :pb["N"]], live[f, :pb["N"]] = pb["truth"], True
    truth, live, U = torch.from_numpy(truth).cuda(), torch.from_numpy(live).cuda(), torch.from_numpy(fr.U).cuda()

    def nll():
        p = layer(U).gather(2, truth[:, :, None])[:, :, 0].clamp_min(1e-12)
        return -(torch.log(p) * live).sum() / live.sum()
    losses = []
    for _ in range(4):
        layer.zero_grad()
        loss = nll()
        loss.backward()
        losses.append(loss.item())
        norm = float(sum((p.grad ** 2).sum() for p in layer.parameters()) ** 0.5)
        assert np.isfinite(norm) and norm > 0
        with torch.no_grad():
            for p in layer.parameters():
                p -= 0.02 * p.grad / norm                            # a step of length 0.02 in parameter space
    losses.append(nll().item())
    layer.close()
    print("NLL", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses

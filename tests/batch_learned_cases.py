"""What the tests of lccrf_batch_inference_backward_all share (include/lccrf.h section 2h; tests/test_batch_learned_backward.py): the
host restatement of k_sum_frames' order, the call with every output pre-filled with NaN, the settings of a learnt model applied to a
batch and to the handle of one of its frames, and the frame-by-frame comparison against handles."""
import importlib

import numpy as np

import batch_cases as bc
import crf_cases as cc
import joint_checker as jc
import normalization_checker as nc
import test_fused_general as fg

F32 = np.float32
SUM_TILE = 64                                                     # frames per tile of k_sum_frames (csrc/meanfield_backward.hip: kSumFrames)
RAGGED = (0, 1, 5, 255, 256, 257, 1001, 2000)                     # the 256 / 257 pair straddles a chunk boundary of k_compat_bwd
SLACK = 7                                                         # max_points beyond the largest frame: the batch's chunk count is no frame's
SETTINGS = list(fg._settings(2))                                  # after (Potts), before, symmetric, none, matrices, mixed


def sum_frames_host(x):
    """k_sum_frames' order restated: out[j] = ((x[0][j] + x[1][j]) + ..) + x[F-1][j], a plain loop of float32 adds over the frames in
    ascending order, starting from frame 0's value; x [F][...] -> [...] (F = 0: zeros)"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], np.float32)
    out = x[0].copy()
    for f in range(1, x.shape[0]):
        out = np.add(out, x[f], dtype=np.float32)                 # (every entry on its own: one float32 add per frame)
    return out


def model_of(gw, gm):
    """d_grad_model [K + K*L*L] restated from the per-frame dL/dw [F][K] and dL/dmu [F][K][L][L]"""
    return np.concatenate([sum_frames_host(gw).reshape(-1), sum_frames_host(gm).reshape(-1)])


def ragged(golden, wl, Ns=RAGGED):
    fr = bc.slam_frames(golden, wl, Ns=Ns)
    return bc.Frames(fr.probs, fr.w, max_points=int(fr.N.max()) + SLACK)


def setting(fr, sname, po):
    """(modes, matrices, weights) of fg._settings' entry; a term in mode NONE has its weight scaled by the mean norm of the largest
    frame (normalization_checker.weights_f32), so that x stays in the softmax's range"""
    modes, mats = fg._settings(fr.K)[sname]
    w = [F32(x) for x in fr.w]
    if nc.NONE in modes:
        f = int(np.argmax(fr.N))
        o = cc.setup(po.OracleCRF, fr.probs[f])
        nrm = [o.kernel(k)["norm"] for k in range(fr.K)]
        o.close()
        w = nc.weights_f32(dict(kernels=[(None, x) for x in fr.w]), nrm, modes)
    return modes, mats, [float(x) for x in w]


def apply(c, modes, mats, weights=None):
    """the setting on a batch or a handle, through the setters both have"""
    for k, w in enumerate(weights or []):
        c.set_pairwise_weight(k, w)
    for k, m in enumerate(modes):
        c.set_normalization(k, m)
    for k, m in enumerate(mats):
        if m is not None:
            c.set_pairwise_compatibility(k, m)


def handle(fr, f, modes, mats, weights):
    h = fr.handle(f)
    apply(h, modes, mats, weights)
    return h


def backward_all(b, fr, T, relax, G, unary=True, weights=True, features=False, compat=True, model=True, stream=None, F=None):
    """dict(gu, gw, gf, gm, model) of lccrf_batch_inference_backward_all, every output pre-filled with NaN; an output that is not asked
    for (a NULL pointer) comes back as filled"""
    import torch
    from abi_support import dev
    F, K, L = len(fr.N) if F is None else F, fr.K, fr.L
    g = dev(np.ascontiguousarray(G[:F], np.float32))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, max(K, 1)), nan(F, max(K, 1), L, L), nan(max(K, 1) * (1 + L * L))
    gf = [nan(F, fr.maxN, d) for d in fr.dims]
    torch.cuda.synchronize()
    b.inference_backward_all_device(T, relax, g.data_ptr(), gu.data_ptr() if unary else None, gw.data_ptr() if weights and K else None,
                                    [t.data_ptr() for t in gf] if features else None, gm.data_ptr() if compat and K else None,
                                    md.data_ptr() if model and K else None, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return dict(gu=gu.cpu().numpy(), gw=gw[:, :K].cpu().numpy(), gm=gm[:, :K].cpu().numpy(), gf=[t.cpu().numpy() for t in gf],
                model=md[:K * (1 + L * L)].cpu().numpy())


def check_frames(out, fr, handles, T, relax, G, features, tag):
    """every frame: the bits of lccrf_inference_backward_all on its handle; rows beyond its points 0; a frame of 0 points all 0"""
    for f, n in enumerate(fr.N):
        where = "%s frame %d (N=%d) T=%d relax=%g" % (tag, f, n, T, relax)
        assert np.all(out["gu"][f, n:] == 0), where
        assert all(np.all(a[f, n:] == 0) for a in out["gf"]) or not features, where
        if n == 0:
            assert np.all(out["gw"][f] == 0) and np.all(out["gm"][f] == 0), where
            continue
        hu, hw, hm, hf = jc.backward_all(handles[f], fr.dims, fr.L, T, relax, G[f, :n], features=features)
        assert cc.same_bits(out["gu"][f, :n], hu), where + ": dL/dU"
        assert cc.same_bits(out["gw"][f], hw), where + ": dL/dw %s, handle %s" % (out["gw"][f], hw)
        assert cc.same_bits(out["gm"][f], hm), where + ": dL/dmu, largest difference %g" % np.abs(out["gm"][f] - hm).max()
        if features:
            for k in range(fr.K):
                assert cc.same_bits(out["gf"][k][f, :n], hf[k]), where + ": dL/df%d" % k
        if T == 0:
            assert np.all(out["gm"][f] == 0) and np.all(out["gw"][f] == 0), where
    assert cc.same_bits(out["model"], model_of(out["gw"], out["gm"])), tag + ": d_grad_model is not the ordered sum"

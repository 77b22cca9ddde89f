"""Feature gradients on handles whose terms carry label-compatibility matrices: lccrf_inference_backward_all (include/lccrf.h
section 1f) and the torch layers on top (lc-crf-slam_amd/autograd.py: mean_field_learned, LearnedCRF).

CPU: the joint checker (tests/joint_checker.py) against the two checkers it joins and against gradcheck, the new symbol, the new
kernels' freedom from scratch memory.  GPU: the entry point against the joint checker on the bar of sections 1d and 1e, its bit
contracts against sections 1d and 1e, its edge cases and argument checks, and the torch layers."""
import ctypes as C
import importlib
import shutil

import numpy as np
import pytest

import compat_checker as ck
import crf_cases as cc
import feature_cases as fc
import grad_support as gs
import joint_checker as jc
import kernel_resources as kr
import meanfield_f64_features as mff
from abi_support import assert_declared_exported_bound, dev, hip_malloc, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_inference_backward_all",)
E_INVALID, E_STATE = -1, -5


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_joint_symbol_is_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3                         # section 1f came without a version step
    assert hasattr(pkg.DenseCRFHIP, "inference_backward_all_device")
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    assert callable(ag.mean_field_learned) and issubclass(ag.LearnedCRF, ag.LearnedKernelCRF)


def test_joint_entry_point_rejects_a_null_handle(lib):
    assert lib.lccrf_inference_backward_all(None, 1, 1.0, None, None, None, None, None) == E_INVALID


def _rel12(a, b):
    return np.linalg.norm(a - b) <= 1e-12 * max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("T,relax", [(1, 1.0), (3, 0.7)])
def test_joint_checker_with_identities_is_the_feature_checker(po, wl, T, relax):
    pb = wl.generic_problem(200, [2, 3], 4, seed=5, spread=1.5)
    o, lats, U = jc.checker(po, pb)
    w, G = gs.weights(pb), jc.grad_prob(pb)
    gu, gw, gm, gf = jc.joint_gradients(U, w, jc.checker_mu(jc.eyes(2, 4), 4), lats, T, relax, G)
    ru, rw, rf, _ = mff.feature_gradients(U, w, lats, T, relax, G)
    assert _rel12(gu, ru) and _rel12(gw, rw) and all(_rel12(a, b) for a, b in zip(gf, rf))
    assert np.linalg.norm(gm) > 0


@pytest.mark.parametrize("T,relax", [(1, 1.0), (3, 0.7)])
def test_joint_checker_with_fixed_features_is_the_compat_checker(po, wl, T, relax):
    pb = wl.generic_problem(200, [2, 3], 4, seed=5, spread=1.5)
    o, lats, U = jc.checker(po, pb)
    w, G, mu = gs.weights(pb), jc.grad_prob(pb), jc.checker_mu(jc.dense(2, 4), 4)
    gu, gw, gm, gf = jc.joint_gradients(U, w, mu, lats, T, relax, G)
    ru, rw, rm = ck.gradients_f64(U, w, mu, lats, T, relax, G)
    assert _rel12(gu, ru) and _rel12(gw, rw) and _rel12(gm, rm)
    assert all(np.linalg.norm(a) > 0 for a in gf)


def test_joint_checker_gradcheck_over_features_and_matrices(po, wl):
    import torch
    pb = wl.generic_problem(40, [2, 3], 3, seed=7, spread=1.5)
    o, lats, U = jc.checker(po, pb)
    u, w = torch.as_tensor(U), torch.as_tensor(gs.weights(pb))
    mu = torch.as_tensor(jc.checker_mu(jc.dense(2, 3), 3)).requires_grad_(True)
    fs = [torch.as_tensor(lat.feat32.astype(np.float64)).clone().requires_grad_(True) for lat in lats]

    def f(m, *feats):
        for lat, x in zip(lats, feats):
            lat.bind(x)
        return ck.forward_f64(u, w, m, lats, 2, 0.7)
    assert torch.autograd.gradcheck(f, (mu,) + tuple(fs), eps=1e-7, atol=1e-6)


@pytest.mark.skipif(shutil.which(kr.HIPCC) is None, reason="hipcc not installed")
def test_joint_softmax_kernels_use_no_scratch():
    """the compatibility softmax backward with the feature part, k_joint_softmax<G> for the five lane groups: no scratch, no
    spilled VGPR (resource metadata only)"""
    use = kr.resource_usage("meanfield_backward.hip")
    names = {k: v for k, v in use.items() if "k_joint_softmax" in k}
    assert len(names) == 5, sorted(names)
    for name, r in names.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)


# ---- GPU: against the checker ---------------------------------------------------------------------------------------------
SETTINGS = jc.SETTINGS


def _handle(r):
    h, keep = gs.gpu_handle(r["pb"], r["image"])
    jc.set_all(h, r["mats"])
    return h, keep


def _run(r, T, relax, **kw):
    h, keep = _handle(r)
    got = jc.backward_all(h, jc.dims_of(r["pb"], r["image"]), r["pb"]["L"], T, relax, r["G"], **kw)
    h.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,relax", SETTINGS)
def test_joint_gradients_match_the_checker(po, wl, golden, name, T, relax):
    """All four outputs against the float64 joint checker, matrices I + 0.3 N(0, 1) on every term.  Measured on the MI355X:
    notes/compatibility.md section 6 lists the largest error per case and output."""
    r = jc.reference_for(po, wl, golden, name, T, relax)
    got = _run(r, T, relax)
    assert all(np.isfinite(a).all() for a in got[:3]) and all(np.isfinite(a).all() for a in got[3])
    jc.assert_within_bars(got, r, T)


@pytest.mark.gpu
@pytest.mark.parametrize("name", jc.MIXED_CASES)
@pytest.mark.parametrize("T,relax", jc.MIXED_SETTINGS)
def test_one_term_with_a_matrix_and_one_without(po, wl, golden, name, T, relax):
    """even terms carry a matrix, odd terms are Potts: d_grad_compat[k] of a Potts term is the derivative at the identity"""
    r = jc.reference_for(po, wl, golden, name, T, relax, "mixed")
    assert any(m is None for m in r["mats"]) and any(m is not None for m in r["mats"])
    jc.assert_within_bars(_run(r, T, relax), r, T)


# ---- GPU: bits ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(cc.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slam:N1001", "nt:d3_L21", "image64x48"])
def test_bits_of_section_1e_determinism_null_outputs_and_state(po, wl, golden, name):
    pb, image = fc.case(name, golden, po, wl)
    K, L, dims = len(pb["kernels"]), pb["L"], jc.dims_of(pb, image)
    mats, G = jc.dense(K, L), np.random.default_rng(9).standard_normal((pb["N"], pb["L"]))
    T, relax = 5, 0.7
    h, keep = gs.gpu_handle(pb, image)
    jc.set_all(h, mats)
    e = jc.backward_compat(h, K, L, T, relax, G)                 # section 1e on the same handle
    a = jc.backward_all(h, dims, L, T, relax, G)
    assert _same(a[:3], e)
    assert all(np.isfinite(x).all() for x in a[:3]) and all(np.isfinite(x).all() for x in a[3])
    q_after = h.probability()
    assert cc.same_bits(q_after, ck.restate_f32(cc.setup(po.OracleCRF, pb).unary(), [f for f, _ in pb["kernels"]],
                                                [np.float32(w) for _, w in pb["kernels"]], mats, T, relax))
    b = jc.backward_all(h, dims, L, T, relax, G)                 # run to run
    assert _same(a[:3], b[:3]) and _same(a[3], b[3])
    c = jc.backward_all(h, dims, L, T, relax, G, features=False)  # d_grad_features == NULL: section 1e
    assert _same(c[:3], e)
    for skip in range(K):                                        # a NULL entry
        c = jc.backward_all(h, dims, L, T, relax, G, skip=(skip,))
        assert _same(c[:3], e) and c[3][skip] is None
        assert all(cc.same_bits(x, y) for k, (x, y) in enumerate(zip(a[3], c[3])) if k != skip)
    c = jc.backward_all(h, dims, L, T, relax, G, unary=False)
    assert np.isnan(c[0]).all() and _same(c[1:3], e[1:]) and _same(c[3], a[3])
    c = jc.backward_all(h, dims, L, T, relax, G, weights=False)
    assert np.isnan(c[1]).all() and cc.same_bits(c[0], e[0]) and cc.same_bits(c[2], e[2]) and _same(c[3], a[3])
    c = jc.backward_all(h, dims, L, T, relax, G, compat=False)
    assert np.isnan(c[2]).all() and _same(c[:2], e[:2]) and _same(c[3], a[3])
    h.inference(T, False, relax)
    assert cc.same_bits(h.probability(), q_after)
    h2, keep2 = gs.gpu_handle(pb, image)                         # a fresh handle whose first call is this one
    jc.set_all(h2, mats)
    d = jc.backward_all(h2, dims, L, T, relax, G)
    assert _same(d[:3], a[:3]) and _same(d[3], a[3])
    h.close(), h2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", jc.POTTS_CASES)
def test_potts_handles_give_section_1d_and_identities_stay_within_the_bar(po, wl, golden, name):
    """Without matrices and without d_grad_compat the call is section 1d's, bit for bit.  With explicit identity matrices dL/df is
    held to the bar against the Potts handle's; whether the two are in fact the same bits is printed (notes/compatibility.md
    section 6 records it), not asserted."""
    T, relax = jc.POTTS_SETTING
    r = jc.reference_for(po, wl, golden, name, T, relax, "potts")
    pb, image, G = r["pb"], r["image"], r["G"]
    K, L, dims = len(pb["kernels"]), pb["L"], jc.dims_of(pb, image)
    h, keep = gs.gpu_handle(pb, image)
    f = jc.backward_features(h, dims, T, relax, G)
    a = jc.backward_all(h, dims, L, T, relax, G, compat=False)
    assert cc.same_bits(a[0], f[0]) and cc.same_bits(a[1], f[1]) and _same(a[3], f[2]) and np.isnan(a[2]).all()
    b = jc.backward_all(h, dims, L, T, relax, G)                 # ... and with dL/dmu at the identity: every output within the bar
    jc.assert_within_bars(b, r, T)
    h2, keep2 = gs.gpu_handle(pb, image)
    jc.set_all(h2, jc.eyes(K, L))
    c = jc.backward_all(h2, dims, L, T, relax, G)
    jc.assert_within_bars(c, r, T)
    floor, bars = 1e-6 * np.linalg.norm(G), r["ref"].bars()
    for k in range(K):
        between, bar = gs.rel(c[3][k], a[3][k], floor), bars["dL/df%d" % k][0]
        print("dL/df of term %d with explicit identities against the Potts handle's, %s: relative L2 difference %.3g (bar %.3g), "
              "bit-identical: %s" % (k, name, between, bar, cc.same_bits(c[3][k], a[3][k])))
        assert between <= bar
    h.close(), h2.close()


# ---- GPU: edge cases --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_t0_is_exactly_zero_and_k0_is_legal(wl):
    pb = wl.slam_problem(700, seed=2)
    G = np.random.default_rng(5).standard_normal((pb["N"], 2))
    h = cc.setup(pkg.DenseCRFHIP, pb)
    jc.set_all(h, jc.dense(2, 2))
    ru, _ = gs.backward(h, 0, 1.0, G, 2)
    gu, gw, gm, gf = jc.backward_all(h, [2, 2], 2, 0, 1.0, G)
    assert cc.same_bits(gu, ru) and np.all(gw == 0) and np.all(gm == 0) and all(np.all(a == 0) for a in gf)
    h.close()
    gen = wl.generic_problem(300, [2], 5, seed=3)
    h0 = pkg.DenseCRFHIP(300, 5)
    h0.set_unary(gen["unary"])
    G5 = np.random.default_rng(6).standard_normal((300, 5))
    ru, _ = gs.backward(h0, 3, 0.7, G5, 0)
    gu, _, _, gf = jc.backward_all(h0, [], 5, 3, 0.7, G5)
    assert cc.same_bits(gu, ru) and gf == []
    h0.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_handle_as_it_was(po, wl):
    import torch
    pb = wl.generic_problem(500, [2, 3], 4, seed=17)
    N, L = 500, 4
    h = cc.setup(pkg.DenseCRFHIP, pb)
    jc.set_all(h, jc.dense(2, L))
    h.inference(4, False, 0.7)
    before = h.probability()
    lb = pkg.lib()
    g, gu = torch.zeros((N, L), device="cuda"), torch.zeros((N, L), device="cuda")
    gf = [torch.zeros((N, 2), device="cuda"), torch.zeros((N, 3), device="cuda")]
    gm = torch.zeros((2, L, L), device="cuda")
    host = np.zeros((N, L), np.float32)
    hl, small = hip_malloc(64)
    vp = C.c_void_p

    def arr(*ps):
        return (vp * 2)(*ps)
    good, m = arr(vp(gf[0].data_ptr()), vp(gf[1].data_ptr())), vp(gm.data_ptr())
    torch.cuda.synchronize()
    try:
        for args in ((-1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, good, m),                 # n_iterations < 0
                     (1, float("nan"), vp(g.data_ptr()), vp(gu.data_ptr()), None, good, m),         # relax not finite
                     (1, float("inf"), vp(g.data_ptr()), vp(gu.data_ptr()), None, good, m),
                     (1, 1.0, None, vp(gu.data_ptr()), None, good, m),                              # no dL/dQ
                     (1, 1.0, vp(host.ctypes.data), vp(gu.data_ptr()), None, good, m),              # pageable host memory
                     (1, 1.0, vp(g.data_ptr()), vp(host.ctypes.data), None, good, m),
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, arr(vp(gf[0].data_ptr()), vp(host.ctypes.data)), m),
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, good, vp(host.ctypes.data)),
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, arr(small, None), m),      # undersized
                     (1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, good, small)):
            assert lb.lccrf_inference_backward_all(h.h, *args) == E_INVALID, args
        h0 = pkg.DenseCRFHIP(N, L)                               # no unary yet
        assert lb.lccrf_inference_backward_all(h0.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, None, None) == E_STATE
        h0.close()
    finally:
        hl.hipFree(small)
    h.inference(4, False, 0.7)
    assert cc.same_bits(h.probability(), before)
    h.close()


# ---- GPU: torch -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mean_field_learned_returns_the_c_abi_bits(po, wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.generic_problem(800, [2, 3], 5, seed=23)
    K, L = 2, 5
    mats = jc.dense(K, L)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    jc.set_all(h, mats)
    G = np.random.default_rng(2).standard_normal((pb["N"], L)).astype(np.float32)
    ref = jc.backward_all(h, [2, 3], L, 5, 0.7, G)
    h.inference(5, False, 0.7)
    ref_q = h.probability()
    h.close()
    u = torch.from_numpy(pb["unary"]).cuda().requires_grad_(True)
    w = torch.tensor([float(np.float32(x)) for _, x in pb["kernels"]], requires_grad=True)
    m = torch.tensor(np.stack(mats), requires_grad=True)
    fs = [torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda().requires_grad_(True) for f, _ in pb["kernels"]]
    q = ag.mean_field_learned(u, fs, w, m, 5, 0.7)
    q.backward(torch.from_numpy(G).cuda())
    torch.cuda.synchronize()
    assert cc.same_bits(q.detach().cpu().numpy(), ref_q)
    assert cc.same_bits(u.grad.cpu().numpy(), ref[0]) and cc.same_bits(w.grad.numpy(), ref[1]) and cc.same_bits(m.grad.numpy(), ref[2])
    assert all(cc.same_bits(f.grad.cpu().numpy(), x) for f, x in zip(fs, ref[3]))


@pytest.mark.gpu
def test_three_sgd_steps_of_learned_crf_on_the_image_crop_lower_the_cross_entropy(po, wl, golden):
    """Teacher and student share the crop's terms at a tenth of the example's weights (at the full weights every row saturates and a
    cross-entropy has nothing left to lose); the teacher has the standard deviations scaled by 1.3 and the matrices I + 0.3 N(0, 1),
    the student starts at the nominal standard deviations and the Potts model.
    The unary: every pixel of this crop carries the same label in the example's annotation, so with the unary built from it every
    Q_t is one row repeated, no output depends on the features, and dL/d log_sd is exactly 0 -- in the float64 joint checker and,
    measured, on the MI355X (log_sd moved by exactly 0 over three steps).  No correct layer can move log_sd there.  The unary
    here is therefore built from labels that vary over the crop: the quartile (0 .. 3) of the pixel's r + g + b, at the case's
    confidence, through the same label-and-confidence form.
    Plain SGD on the mean cross-entropy against the teacher's Q with a step of 10, chosen on the float64 joint checker (lattices
    rebuilt at every step's features): there the loss falls 1.836706 -> 1.836418 -> 1.836206 -> 1.836020, 1500 to 2400 float32 ulps
    per step, log_sd moves by -4.1e-4 (position term) and -1.8e-3 / -1.6e-2 (position / colour of the RGB term) and |compat - I|
    reaches 0.145; a step of 30 overshoots at the third step."""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb, (W, H, im) = cc.case("image64x48", golden, po, wl)
    K, L = 2, pb["L"]
    gray = im.reshape(-1, 3).astype(np.float64).sum(1)
    pb = dict(pb, label=np.digitize(gray, np.quantile(gray, [0.25, 0.5, 0.75])).astype(np.int16))
    o = cc.setup(po.OracleCRF, pb)
    U = torch.from_numpy(o.unary()).cuda()
    o.close()
    sd, groups = [[3.0], [60.0, 20.0]], [[[0, 1]], [[0, 1], [2, 3, 4]]]
    cols = [np.array([0, 0]), np.array([0, 0, 1, 1, 1])]
    # the raw pixel coordinates and colours back from the case's features (integers: the rounding is exact)
    raw = [np.rint(f.astype(np.float64) * np.array(s)[c]).astype(np.float32) for (f, _), s, c in zip(pb["kernels"], sd, cols)]
    weights = [float(np.float32(w)) / 10 for _, w in pb["kernels"]]
    teacher = ag.LearnedCRF(raw, [[1.3 * x for x in s] for s in sd], weights, groups=groups, n_labels=L, n_iterations=5)
    layer = ag.LearnedCRF(raw, sd, weights, groups=groups, n_labels=L, n_iterations=5)
    assert torch.equal(layer.compat.detach(), torch.eye(L).repeat(K, 1, 1))
    with torch.no_grad():
        teacher.compat.copy_(torch.tensor(np.stack(jc.dense(K, L))))
        target = teacher(U).clone()
    start_sd = [p.detach().clone() for p in layer.log_sd]
    opt = torch.optim.SGD(layer.parameters(), lr=10.0)

    def loss_of():
        return -(target * torch.log(layer(U).clamp_min(1e-12))).sum(1).mean()

    losses = []
    for _ in range(3):
        loss = loss_of()
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        losses.append(loss_of().item())
    print("cross-entropy over three SGD steps:", losses)
    print("log_sd moved by", [(p.detach() - s).cpu().numpy() for p, s in zip(layer.log_sd, start_sd)],
          "|compat - I|", float((layer.compat.detach() - torch.eye(L)).norm()))
    assert losses[-1] < losses[0], losses
    assert not torch.equal(layer.compat.detach(), torch.eye(L).repeat(K, 1, 1))
    assert all(not torch.equal(p.detach(), s) for p, s in zip(layer.log_sd, start_sd))

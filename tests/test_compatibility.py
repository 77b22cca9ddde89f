"""Label-compatibility matrices of the pairwise terms (include/lccrf.h section 1e) and their gradients.

CPU: the new symbols, and the two restatements of tests/compat_checker.py against the oracle and against tests/meanfield_f64.py.
GPU: every entry point that honours a matrix against the float32 restatement, bit for bit; routing (identity matrices and a cleared
matrix give the fast engines' bits); lccrf_inference_backward_compat against the float64 checker on the bar of
tests/test_meanfield_backward.py, its determinism and state contract; the torch layer."""
import ctypes as C
import importlib

import numpy as np
import pytest

import compat_checker as ck
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import meanfield_f64 as mf
from abi_support import assert_declared_exported_bound, dev, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_set_pairwise_compatibility", "lccrf_get_pairwise_compatibility", "lccrf_inference_backward_compat")
E_INVALID, E_STATE = -1, -5


def _dense(K, L, seed=77):
    """I + 0.3 N(0, 1), seeded"""
    rng = np.random.default_rng([seed, K, L])
    return [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]


def _potts_penalty(K, L):
    return [(1.0 - np.eye(L)).astype(np.float32) for _ in range(K)]


def _eyes(K, L):
    return [np.eye(L, dtype=np.float32) for _ in range(K)]


def _feats(pb):
    return [f for f, _ in pb["kernels"]]


def _w32(pb):
    return [np.float32(w) for _, w in pb["kernels"]]


def _unary(po, pb):
    o = cc.setup(po.OracleCRF, pb)
    u = o.unary()
    o.close()
    return u


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_compat_symbols_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3
    for m in ("set_pairwise_compatibility", "get_pairwise_compatibility", "inference_backward_compat_device"):
        assert hasattr(pkg.DenseCRFHIP, m), m


def test_compat_symbols_reject_a_null_handle(lib):
    assert lib.lccrf_set_pairwise_compatibility(None, 0, None) == E_INVALID
    assert lib.lccrf_get_pairwise_compatibility(None, 0, None, None) == E_INVALID
    assert lib.lccrf_inference_backward_compat(None, 1, 1.0, None, None, None, None) == E_INVALID


@pytest.mark.parametrize("N,L,dims,relax", [(500, 2, (2, 2), 1.0), (777, 5, (2, 5), 1.0), (300, 21, (2, 5), 0.5), (1000, 3, (3,), 1.0)])
def test_restatement_with_identities_is_the_oracle(po, wl, N, L, dims, relax):
    pb = wl.generic_problem(N, list(dims), L, seed=21)
    o = cc.setup(po.OracleCRF, pb)
    o.inference(5, False, relax)
    q = ck.restate_f32(o.unary(), _feats(pb), _w32(pb), _eyes(len(dims), L), 5, relax)
    assert cc.same_bits(q, o.probability())
    q = ck.restate_f32(o.unary(), _feats(pb), _w32(pb), [None] * len(dims), 5, relax)
    assert cc.same_bits(q, o.probability())


def test_f64_checker_with_identities_is_the_potts_checker(po, wl):
    import torch
    pb = wl.generic_problem(200, [2, 3], 4, seed=5)
    o, lats, U = gs.checker(po, pb)
    u, w = torch.as_tensor(U), torch.as_tensor(gs.weights(pb))
    mu = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    for relax in (1.0, 0.7):
        a, b = ck.forward_f64(u, w, mu, lats, 5, relax), mf.forward(u, w, lats, 5, relax)
        assert float((a - b).abs().max()) <= 1e-12


def test_f64_checker_gradcheck_in_the_matrices(po, wl):
    import torch
    pb = wl.generic_problem(40, [2, 3], 3, seed=4)
    o, lats, U = gs.checker(po, pb)
    u, w = torch.as_tensor(U), torch.as_tensor(gs.weights(pb))
    mu = torch.as_tensor(np.stack(_dense(2, 3)).astype(np.float64)).requires_grad_(True)
    for relax in (1.0, 0.7):
        assert torch.autograd.gradcheck(lambda m: ck.forward_f64(u, w, m, lats, 3, relax), (mu,), eps=1e-6, atol=1e-7)


# ---- GPU: forward -----------------------------------------------------------------------------------------------------------
FORWARD_CASES = ["generic:d3_L21", "generic:d1_L3", "generic:multi", "slam:N1001", "image64x48", "locality9000"]


def _fcase(name, golden, po, wl):
    if name == "locality9000":                                   # >= 8192 points: lccrf_inference runs in locality mode
        return wl.generic_problem(9000, [2, 3], 3, seed=31), None
    return cc.case(name, golden, po, wl)


def _set_all(h, mats):
    for k, m in enumerate(mats):
        h.set_pairwise_compatibility(k, m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FORWARD_CASES)
@pytest.mark.parametrize("kind", ["dense", "potts_penalty"])
def test_inference_is_the_restatement(po, wl, golden, name, kind):
    pb, image = _fcase(name, golden, po, wl)
    K, L = len(pb["kernels"]), pb["L"]
    mats = _dense(K, L) if kind == "dense" else _potts_penalty(K, L)
    U = _unary(po, pb)
    h, keep = gs.gpu_handle(pb, image)
    _set_all(h, mats)
    for T in (0, 1, 5):
        for relax in (1.0, 0.7):
            ref = ck.restate_f32(U, _feats(pb), _w32(pb), mats, T, relax)
            h.inference(T, True, relax)
            q = h.probability()
            assert cc.same_bits(q, ref), (name, kind, T, relax, float(np.abs(q - ref).max()))
            assert np.array_equal(h.map(), ck.map_of(ref)), (name, kind, T, relax)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["generic:multi", "slam:N1001", "image64x48"])
def test_one_term_with_a_matrix_and_one_without(po, wl, golden, name):
    pb, image = cc.case(name, golden, po, wl)
    K, L = len(pb["kernels"]), pb["L"]
    mats = [m if k % 2 == 0 else None for k, m in enumerate(_dense(K, L))]
    U = _unary(po, pb)
    h, keep = gs.gpu_handle(pb, image)
    _set_all(h, mats)
    for T, relax in ((1, 1.0), (5, 0.7)):
        ref = ck.restate_f32(U, _feats(pb), _w32(pb), mats, T, relax)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref))
    h.close()


def _identity_problem(name, golden, po, wl):
    if name == "L64":
        return cc.label_problem(900, 64, [2, 3], seed=6), None
    return cc.case(name, golden, po, wl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slam:C3", "generic:d3_L21", "L64"])
def test_identity_matrices_and_a_cleared_matrix_give_the_fast_engines_bits(po, wl, golden, name):
    pb, image = _identity_problem(name, golden, po, wl)
    K, L = len(pb["kernels"]), pb["L"]
    fresh, keep = gs.gpu_handle(pb, image)
    h, keep2 = gs.gpu_handle(pb, image)
    _set_all(h, _eyes(K, L))
    for T, relax in ((5, 1.0), (5, 0.7), (0, 1.0)):
        fresh.inference(T, True, relax)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), fresh.probability()) and np.array_equal(h.map(), fresh.map()), (name, T, relax)
    # set then clear: the bits of a handle that never had a matrix (handles expose no engine probe: bits only)
    _set_all(h, _dense(K, L))
    h.inference(5, True, 1.0)
    _set_all(h, [None] * K)
    for k in range(K):
        assert h.get_pairwise_compatibility(k)[1] is False
    for T, relax in ((5, 1.0), (3, 0.7)):
        fresh.inference(T, True, relax)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), fresh.probability()) and np.array_equal(h.map(), fresh.map()), (name, T, relax)
    h.close(), fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["generic:d3_L21", "slam:N1001", "generic:multi"])
def test_steps_equal_inference_and_apply_is_one_term(po, wl, golden, name):
    import torch
    pb, image = cc.case(name, golden, po, wl)
    K, L, N = len(pb["kernels"]), pb["L"], pb["N"]
    mats = _dense(K, L)
    h, keep = gs.gpu_handle(pb, image)
    _set_all(h, mats)
    for relax in (1.0, 0.7):
        h.inference(4, False, relax)
        q = h.probability()
        h.start_inference()
        for _ in range(4):
            h.step_inference(relax)
        assert cc.same_bits(h.probability(), q)
    # PairwisePotential::apply of every term: out + w * norm * (mu applied to Phi(x))
    rng = np.random.default_rng(8)
    x = rng.random((N, L)).astype(np.float32)
    out = rng.standard_normal((N, L)).astype(np.float32)
    nrm = ck.norms(N, L, _feats(pb))
    for k in range(K):
        ref = ck.term_f32(out, _feats(pb)[k], _w32(pb)[k], nrm[k], mats[k], x)
        assert cc.same_bits(h.apply(k, out, x), ref), k
        d_out, d_x = dev(out), dev(x)
        torch.cuda.synchronize()
        h.pairwise_apply_device(k, d_out.data_ptr(), d_x.data_ptr())
        h.synchronize()
        assert cc.same_bits(d_out.cpu().numpy(), ref), k
    h.close()


@pytest.mark.gpu
def test_setter_getter_errors_and_the_handle_cache(po, wl, lib):
    pb = wl.generic_problem(600, [2, 3], 5, seed=13)
    K, L = 2, 5
    mats = _dense(K, L)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for k in range(K):
        m, is_set = h.get_pairwise_compatibility(k)
        assert not is_set and np.array_equal(m, np.eye(L, dtype=np.float32))
    h.set_pairwise_compatibility(1, mats[1])
    m, is_set = h.get_pairwise_compatibility(1)
    assert is_set and cc.same_bits(m, mats[1])
    assert not h.get_pairwise_compatibility(0)[1]
    f32p = C.POINTER(C.c_float)
    for bad in (np.nan, np.inf, -np.inf):
        m = mats[0].copy()
        m[2, 3] = bad
        assert lib.lccrf_set_pairwise_compatibility(h.h, 0, m.ctypes.data_as(f32p)) == E_INVALID
    assert not h.get_pairwise_compatibility(0)[1]
    for k in (-1, K, 99):
        assert lib.lccrf_set_pairwise_compatibility(h.h, k, mats[0].ctypes.data_as(f32p)) == E_INVALID
        assert lib.lccrf_get_pairwise_compatibility(h.h, k, None, None) == E_INVALID
    # a rejected setter left the handle as it was
    ref = ck.restate_f32(pb["unary"], _feats(pb), _w32(pb), [None, mats[1]], 3, 1.0)
    h.inference(3, False)
    assert cc.same_bits(h.probability(), ref)
    # destroyed and recreated (a cache hit): no matrices, Potts bits
    h.close()
    h2 = cc.setup(pkg.DenseCRFHIP, pb)
    assert not any(h2.get_pairwise_compatibility(k)[1] for k in range(K))
    o = cc.setup(po.OracleCRF, pb)
    h2.inference(3, True)
    o.inference_native(3, True)
    assert cc.same_bits(h2.probability(), o.probability()) and np.array_equal(h2.map(), o.map())
    h2.close()


@pytest.mark.gpu
def test_feature_gradients_are_refused_while_a_matrix_is_set(po, wl, lib):
    import torch
    pb = wl.generic_problem(500, [2, 3], 4, seed=17)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.set_pairwise_compatibility(0, _dense(2, 4)[0])
    h.inference(4, False, 0.7)
    before = h.probability()
    g = torch.zeros((500, 4), device="cuda")
    gu = torch.zeros((500, 4), device="cuda")
    gf = [torch.zeros((500, 2), device="cuda"), torch.zeros((500, 3), device="cuda")]
    ptrs = (C.c_void_p * 2)(*[C.c_void_p(t.data_ptr()) for t in gf])
    torch.cuda.synchronize()
    rc = lib.lccrf_inference_backward_features(h.h, 4, 0.7, C.c_void_p(g.data_ptr()), C.c_void_p(gu.data_ptr()), None, ptrs)
    assert rc == E_STATE
    h.inference(4, False, 0.7)
    assert cc.same_bits(h.probability(), before)
    h.close()


# ---- GPU: gradients ---------------------------------------------------------------------------------------------------------
def _backward_compat(h, T, relax, G, K, L, with_u=True, with_w=True):
    import torch
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    gm = torch.full((max(K, 1), L, L), float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_compat_device(T, relax, g.data_ptr(), gu.data_ptr() if with_u else None,
                                       gw.data_ptr() if K and with_w else None, gm.data_ptr())
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy(), gm[:K].cpu().numpy()


def assert_matches_compat_checker(got, U, w, mats, lats, T, relax, G, name=""):
    """The bar of tests/grad_support.py (assert_within_bar), applied to dL/dmu as to dL/dU and dL/dw; gradients below 1e-6 |dL/dQ|
    (x max(|w|, 1) for dL/dw and dL/dmu) are compared in absolute terms against that floor.  Returns the grad_support.Reference."""
    r = gs.compat_reference(U, w, mats, lats, T, relax, G, name)
    r.check(dict(zip(("dL/dU", "dL/dw", "dL/dmu"), got)))
    return r


GRAD_CASES = gset.COMPAT_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,relax", gset.COMPAT_SETTINGS, ids=gset.COMPAT_IDS)
def test_compat_gradients_match_the_checker(po, wl, golden, name, T, relax):
    """Measured on the MI355X: notes/gradient_bars.md lists the largest error per case."""
    s = gset.compat(po, wl, golden, name, T, relax)
    pb, image, G, mats = s["pb"], s["image"], s["G"], s["mats"]
    K, L = len(pb["kernels"]), pb["L"]
    h, keep = gs.gpu_handle(pb, image)
    _set_all(h, mats)
    got = _backward_compat(h, T, relax, G, K, L)
    s["ref"].check(dict(zip(("dL/dU", "dL/dw", "dL/dmu"), got)))
    if T == 0:
        assert np.all(got[2] == 0) and np.all(got[1] == 0)
    # lccrf_inference_backward on the same handle: the same dL/dU and dL/dw
    import torch
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((K,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr())
    h.synchronize()
    assert cc.same_bits(gu.cpu().numpy(), got[0]) and cc.same_bits(gw.cpu().numpy(), got[1])
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["generic:d3_L21", "slam:N1001"])
def test_gradient_at_a_potts_term_is_that_at_the_identity(po, wl, golden, name):
    pb, image, _ = gset.compat_case(name, golden, po, wl)
    K, L = len(pb["kernels"]), pb["L"]
    o, lats, U = gs.checker(po, pb)
    G = np.random.default_rng(4).standard_normal((pb["N"], L))
    T, relax = 5, 0.7
    h, keep = gs.gpu_handle(pb, image)
    a = _backward_compat(h, T, relax, G, K, L)
    r = assert_matches_compat_checker(a, U, gs.weights(pb), _eyes(K, L), lats, T, relax, G, name + " (no matrix)")
    bar, floor = r.bars()["dL/dmu"][0], r.floors["dL/dmu"]
    h2, keep2 = gs.gpu_handle(pb, image)
    _set_all(h2, _eyes(K, L))
    b = _backward_compat(h2, T, relax, G, K, L)
    assert_matches_compat_checker(b, U, gs.weights(pb), _eyes(K, L), lats, T, relax, G, name + " (identity)")
    assert cc.same_bits(a[0], b[0]) and cc.same_bits(a[1], b[1])
    between = gs.rel(a[2], b[2], floor)                           # ... and one against the other, to the same bar
    print("dL/dmu without a matrix against an explicit identity, %s: relative L2 difference %.3g (bar %.3g)" % (name, between, bar))
    assert between <= bar
    h.close(), h2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["generic:d3_L21", "slam:N1001", "image64x48"])
def test_compat_backward_is_deterministic_and_leaves_the_inference_state(po, wl, golden, name):
    pb, image = cc.case(name, golden, po, wl)
    K, L = len(pb["kernels"]), pb["L"]
    mats = _dense(K, L)
    G = np.random.default_rng(9).standard_normal((pb["N"], L))
    T, relax = 5, 0.7
    h, keep = gs.gpu_handle(pb, image)
    _set_all(h, mats)
    h.inference(T, False, relax)
    q = h.probability()
    a = _backward_compat(h, T, relax, G, K, L)
    assert cc.same_bits(h.probability(), q)                     # Q is what inference(T, 0, relax) leaves
    b = _backward_compat(h, T, relax, G, K, L)
    assert all(cc.same_bits(x, y) for x, y in zip(a, b))
    c = _backward_compat(h, T, relax, G, K, L, with_u=False, with_w=False)   # NULL dL/dU and dL/dw: dL/dmu unchanged
    assert cc.same_bits(c[2], a[2])
    assert cc.same_bits(h.probability(), ck.restate_f32(_unary(po, pb), _feats(pb), _w32(pb), mats, T, relax))
    h.close()


# ---- GPU: torch -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_torch_layer_returns_the_c_abi_gradients(po, wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.generic_problem(800, [2, 3], 5, seed=23)
    K, L = 2, 5
    mats = _dense(K, L)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    _set_all(h, mats)
    G = np.random.default_rng(2).standard_normal((pb["N"], L)).astype(np.float32)
    ref = _backward_compat(h, 5, 0.7, G, K, L)
    h.inference(5, False, 0.7)
    ref_q = h.probability()
    _set_all(h, [None] * K)                                      # the layer arms the handle itself
    u = torch.from_numpy(pb["unary"]).cuda().requires_grad_(True)
    w = torch.tensor([float(x) for x in _w32(pb)], requires_grad=True)
    m = torch.tensor(np.stack(mats), requires_grad=True)
    q = ag.mean_field_compat(h, u, w, m, 5, 0.7)
    q.backward(torch.from_numpy(G).cuda())
    torch.cuda.synchronize()
    assert cc.same_bits(q.detach().cpu().numpy(), ref_q)
    assert cc.same_bits(u.grad.cpu().numpy(), ref[0]) and cc.same_bits(w.grad.numpy(), ref[1]) and cc.same_bits(m.grad.numpy(), ref[2])
    h.close()


@pytest.mark.gpu
def test_three_sgd_steps_on_the_image_crop_lower_the_cross_entropy(po, wl, golden):
    """Teacher and student share the crop's terms at a tenth of the example's weights (at the full weights every row saturates and a
    cross-entropy has nothing left to lose); the teacher has the matrices I + 0.3 N(0, 1), the student starts at the Potts model.
    Plain SGD on the mean cross-entropy against the teacher's Q with a step of 1.0, chosen on the float64 checker: there the loss
    falls 1.48302 -> 1.48284 -> 1.48271 -> 1.48259, thousands of float32 ulps per step (a step of 5 overshoots)."""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb, _ = cc.case("image64x48", golden, po, wl)
    K, L = 2, pb["L"]
    U = torch.from_numpy(_unary(po, pb)).cuda()
    weights = [float(w) / 10 for w in _w32(pb)]
    layer = ag.CompatMeanFieldCRF(pb["N"], L, _feats(pb), weights, n_iterations=5)
    assert torch.equal(layer.compat.detach(), torch.eye(L).repeat(K, 1, 1))
    with torch.no_grad():
        target = ag.mean_field_compat(layer.crf, U, layer.weights, torch.tensor(np.stack(_dense(K, L))), 5).clone()
    opt = torch.optim.SGD(layer.parameters(), lr=1.0)

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
    layer.close()
    print("cross-entropy over three SGD steps:", losses)
    assert losses[-1] < losses[0], losses
    assert not torch.equal(layer.compat.detach(), torch.eye(L).repeat(K, 1, 1))

"""Per-term normalisation modes (include/lccrf.h section 1g) and their gradients.

CPU: the new symbols, the float32 restatement of tests/normalization_checker.py against the oracle, and which splat kernel each
forward case reaches (from the oracle's lattices).  GPU: every entry point that honours a mode against the restatement, bit for bit;
routing (explicit AFTER and SYMMETRIC-then-AFTER give the fast engines' bits); lccrf_inference_backward_compat against the float64
checker on the bar of tests/test_compatibility.py, its determinism; the refusals; the torch layer."""
import ctypes as C
import importlib

import numpy as np
import pytest

import compat_checker as ck
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import normalization_checker as nc
from abi_support import assert_declared_exported_bound, dev, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_set_pairwise_normalization", "lccrf_get_pairwise_normalization")
E_INVALID, E_STATE = -1, -5


def _dense(K, L, seed=77):
    """I + 0.3 N(0, 1), seeded"""
    rng = np.random.default_rng([seed, K, L])
    return [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]


_prepared = gset.norm_prepared


def _handle(pb, weights, modes, mats=None):
    """a GPU handle of the problem with the given weights, modes and matrices"""
    h = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, w) for (f, _), w in zip(pb["kernels"], weights)]))
    for k, m in enumerate(modes):
        h.set_normalization(k, m)
    for k, m in enumerate(mats or []):
        h.set_pairwise_compatibility(k, m)
    return h


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_normalization_symbols_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3
    for m in ("set_normalization", "get_normalization"):
        assert hasattr(pkg.DenseCRFHIP, m), m
    assert (pkg.NORMALIZE_AFTER, pkg.NORMALIZE_BEFORE, pkg.NORMALIZE_SYMMETRIC, pkg.NORMALIZE_NONE) == nc.MODES


def test_normalization_symbols_reject_a_null_handle(lib):
    mode = C.c_int(7)
    assert lib.lccrf_set_pairwise_normalization(None, 0, 2) == E_INVALID
    assert lib.lccrf_get_pairwise_normalization(None, 0, C.byref(mode)) == E_INVALID


@pytest.mark.parametrize("name,relax", [("slam:N1001", 1.0), ("generic:d3_L21", 0.7)])
def test_restatement_with_every_term_after_is_the_oracle(po, wl, golden, name, relax):
    pb, U, nrm = _prepared(name, golden, po, wl)
    K = len(pb["kernels"])
    o = cc.setup(po.OracleCRF, pb)
    o.inference(5, False, relax)
    q = nc.restate_f32(U, nc.feats(pb), nc.weights_f32(pb, nrm, [nc.AFTER] * K), [None] * K, [nc.AFTER] * K, 5, relax)
    assert cc.same_bits(q, o.probability())
    o.close()


def test_f64_checker_with_every_term_after_is_the_compat_checker(po, wl):
    import torch
    pb = wl.generic_problem(200, [2, 3], 4, seed=5)
    o, lats, U = gs.checker(po, pb)
    u, w = torch.as_tensor(U), torch.as_tensor(gs.weights(pb))
    mu = torch.as_tensor(np.stack(_dense(2, 4)).astype(np.float64))
    for relax in (1.0, 0.7):
        a, b = nc.forward_f64(u, w, mu, lats, [nc.AFTER] * 2, 5, relax), ck.forward_f64(u, w, mu, lats, 5, relax)
        assert float((a - b).abs().max()) <= 1e-12


FORWARD_CASES = ["slam:N1001", "generic:d1_L3", "L21:d3_d5", "L64:N300", "crop64x48", "crop96x48"]


def test_forward_cases_reach_the_splat_kernels_they_are_there_for(po, wl, golden):
    """launch_splat (csrc/stream_filter.hip) takes k_splat4 from four labels on when capacity * (d + 1) <= 4 V, k_splat otherwise, and
    k_splat_long beside either for the rows of more than 512 entries of a handle whose capacity exceeds 4096 points."""
    def lattices(name):
        pb, _, _ = _prepared(name, golden, po, wl)
        o = cc.setup(po.OracleCRF, pb)
        out = [(k["d"], k["V"], int(np.bincount(k["offset"].reshape(-1), minlength=k["V"]).max()))
               for k in (o.kernel(i) for i in range(len(pb["kernels"])))]
        o.close()
        return nc.handle_capacity(pb["N"]), out
    cap, lat = lattices("L21:d3_d5")
    assert all(cap * (d + 1) <= 4 * V for d, V, _ in lat), lat                    # k_splat4, both terms
    cap, lat = lattices("crop96x48")
    assert cap > 4096 and sum(row > 512 for _, _, row in lat) == 2, (cap, lat)    # k_splat_long: the RGB and the coarse term
    assert all(cap * (d + 1) > 4 * V for d, V, _ in lat), lat                     # ... beside k_splat
    cap, lat = lattices("crop64x48")
    assert cap == 4096 and max(row for _, _, row in lat) > 512, (cap, lat)        # no list at this capacity: long rows in line, k_splat
    for name in ("slam:N1001", "generic:d1_L3", "L64:N300"):
        cap, lat = lattices(name)
        assert all(cap * (d + 1) > 4 * V for d, V, _ in lat), (name, lat)         # k_splat


# ---- GPU: forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FORWARD_CASES)
@pytest.mark.parametrize("mode", nc.MODES, ids=[nc.MODE_NAMES[m] for m in nc.MODES])
def test_inference_is_the_restatement(po, wl, golden, name, mode):
    """Which case reaches which splat kernel (checked without a GPU by test_forward_cases_reach_the_splat_kernels_they_are_there_for):
    slam:N1001 (L = 2, two 2-D terms), generic:d1_L3 and L64:N300 -- k_splat; L21:d3_d5 (fine lattices, about one entry per row) --
    k_splat4; crop64x48 (the RGB and the coarse position term have rows of 1596 and 3004 entries) -- k_splat, the long rows in
    line: a handle of 3072 points has a capacity of 4096, for which the engine keeps no list of long rows; crop96x48 (4608 points,
    capacity 6144, the same three terms) -- k_splat + k_splat_long.  The scaled instantiations in every mode but AFTER and NONE.
    NONE: the weights are scaled by the mean of n (normalization_checker.weights_f32)."""
    pb, U, nrm = _prepared(name, golden, po, wl)
    K = len(pb["kernels"])
    modes = [mode] * K
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes)
    assert [h.get_normalization(k) for k in range(K)] == modes
    for relax in (1.0, 0.7):
        trace = nc.restate_trace_f32(U, nc.feats(pb), w, [None] * K, modes, 5, relax, nrm)
        for T in (0, 1, 5):
            h.inference(T, True, relax)
            q = h.probability()
            assert cc.same_bits(q, trace[T]), (name, mode, T, relax, float(np.abs(q - trace[T]).max()))
            assert np.array_equal(h.map(), ck.map_of(trace[T])), (name, mode, T, relax)
    for k in range(K):                                           # lccrf_get_norm is the same in every mode
        assert cc.same_bits(h.kernel(k)["norm"], nrm[k]), k
    h.close()


@pytest.mark.gpu
def test_three_terms_in_three_modes_one_with_a_matrix(po, wl):
    pb = wl.generic_problem(600, [2, 3, 2], 5, seed=19)
    K, L = 3, 5
    nrm = ck.norms(pb["N"], L, nc.feats(pb))
    modes = [nc.SYMMETRIC, nc.BEFORE, nc.NONE]
    mats = [None, _dense(K, L)[1], None]
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes)
    h.set_pairwise_compatibility(1, mats[1])
    for T, relax in ((1, 1.0), (5, 0.7)):
        ref = nc.restate_f32(pb["unary"], nc.feats(pb), w, mats, modes, T, relax, nrm)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref)), (T, relax)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slam:N1001", "c2", "generic:d3_L21"])
def test_explicit_after_and_a_mode_set_and_taken_back_give_the_fast_engines_bits(po, wl, golden, name):
    """(handles expose no engine probe: the fast engines' bits are the evidence, as in tests/test_compatibility.py)  c2: the
    2000-point two-label frame."""
    pb, _ = cc.case(name, golden, po, wl)
    K = len(pb["kernels"])
    fresh, h = cc.setup(pkg.DenseCRFHIP, pb), cc.setup(pkg.DenseCRFHIP, pb)
    for k in range(K):
        assert h.get_normalization(k) == nc.AFTER
        h.set_normalization(k, nc.AFTER)
    for T, relax in ((5, 1.0), (5, 0.7), (0, 1.0)):
        fresh.inference(T, True, relax)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), fresh.probability()) and np.array_equal(h.map(), fresh.map()), (name, T, relax)
    for k in range(K):
        h.set_normalization(k, nc.SYMMETRIC)
    h.inference(5, True, 1.0)
    assert not cc.same_bits(h.probability(), fresh.probability())
    for k in range(K):
        h.set_normalization(k, nc.AFTER)
    for T, relax in ((5, 1.0), (3, 0.7)):
        fresh.inference(T, True, relax)
        h.inference(T, True, relax)
        assert cc.same_bits(h.probability(), fresh.probability()) and np.array_equal(h.map(), fresh.map()), (name, T, relax)
    h.close(), fresh.close()
    h2 = cc.setup(pkg.DenseCRFHIP, pb)                           # a recycled handle: every term at AFTER again
    assert all(h2.get_normalization(k) == nc.AFTER for k in range(K))
    h2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slam:N1001", "L21:d3_d5"])
@pytest.mark.parametrize("mode", nc.MODES, ids=[nc.MODE_NAMES[m] for m in nc.MODES])
def test_steps_equal_inference_and_apply_is_one_term(po, wl, golden, name, mode):
    import torch
    pb, U, nrm = _prepared(name, golden, po, wl)
    K, L, N = len(pb["kernels"]), pb["L"], pb["N"]
    modes = [mode] * K
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes)
    for relax in (1.0, 0.7):
        h.inference(3, False, relax)
        q = h.probability()
        h.start_inference()
        for _ in range(3):
            h.step_inference(relax)
        assert cc.same_bits(h.probability(), q)
    # PairwisePotential::apply of every term: out + (w * post) * Phi(pre * x)
    rng = np.random.default_rng(8)
    x = rng.random((N, L)).astype(np.float32)
    out = rng.standard_normal((N, L)).astype(np.float32)
    for k in range(K):
        ref = nc.term_f32(out, nc.feats(pb)[k], w[k], nrm[k], None, mode, x)
        assert cc.same_bits(h.apply(k, out, x), ref), k
        d_out, d_x = dev(out), dev(x)
        torch.cuda.synchronize()
        h.pairwise_apply_device(k, d_out.data_ptr(), d_x.data_ptr())
        h.synchronize()
        assert cc.same_bits(d_out.cpu().numpy(), ref), k
    h.close()


@pytest.mark.gpu
def test_locality_mode_symmetric(po, wl):
    """8200 points (>= 8192: lccrf_inference runs in its internal point order), two labels, two 2-D terms: the caller's order out"""
    pb = wl.generic_problem(8200, [2, 2], 2, seed=31)
    nrm = ck.norms(pb["N"], 2, nc.feats(pb))
    modes = [nc.SYMMETRIC] * 2
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes)
    ref = nc.restate_f32(pb["unary"], nc.feats(pb), w, [None] * 2, modes, 2, 1.0, nrm)
    h.inference(2, True, 1.0)
    assert cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref))
    h.close()


# ---- GPU: gradients ---------------------------------------------------------------------------------------------------------
def _backward_compat(h, T, relax, G, K, L):
    import torch
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    gm = torch.full((max(K, 1), L, L), float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_compat_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), gm.data_ptr())
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy(), gm[:K].cpu().numpy()


GRAD_SETTINGS = gset.NORM_SETTINGS                               # (the cases and why: tests/gradient_settings.py)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,T,relax", GRAD_SETTINGS,
                         ids=["%s-%s-T%d-r%g" % (n, nc.MODE_NAMES[m], T, r) for n, m, T, r in GRAD_SETTINGS])
def test_gradients_match_the_checker(po, wl, golden, name, mode, T, relax):
    """Every term in `mode`, with the matrices I + 0.3 N(0, 1).  Measured on the MI355X: notes/normalization.md section 5 lists the
    largest error per case and mode."""
    s = gset.normalization(po, wl, golden, name, mode, T, relax)
    pb, U, nrm, modes, mats, w, G = (s[x] for x in ("pb", "U", "nrm", "modes", "mats", "w", "G"))
    K, L = len(pb["kernels"]), pb["L"]
    h = _handle(pb, w, modes, mats)
    got = _backward_compat(h, T, relax, G, K, L)
    s["ref"].check(dict(zip(("dL/dU", "dL/dw", "dL/dmu"), got)))  # (a bar beyond 1e-2 fails there: it would check nothing)
    if T == 0:
        assert np.all(got[1] == 0) and np.all(got[2] == 0)
    again = _backward_compat(h, T, relax, G, K, L)               # the same bits from run to run
    assert all(cc.same_bits(a, b) for a, b in zip(got, again))
    # ... Q afterwards as lccrf_inference(T, 0, relax) leaves it, and lccrf_inference_backward gives the same dL/dU and dL/dw
    assert cc.same_bits(h.probability(), nc.restate_f32(U, nc.feats(pb), w, mats, modes, T, relax, nrm))
    gu, gw = gs.backward(h, T, relax, G, K)
    assert cc.same_bits(gu, got[0]) and cc.same_bits(gw, got[1])
    h.close()


@pytest.mark.gpu
def test_refusals(po, wl, lib):
    import torch
    pb = wl.generic_problem(500, [2, 3], 4, seed=17)
    K = 2
    h = cc.setup(pkg.DenseCRFHIP, pb)
    for k in range(K):
        h.set_normalization(k, nc.SYMMETRIC)
    for bad_mode in (4, -1, 99):
        assert lib.lccrf_set_pairwise_normalization(h.h, 0, bad_mode) == E_INVALID
    mode = C.c_int(0)
    for bad_k in (-1, K, 99):
        assert lib.lccrf_set_pairwise_normalization(h.h, bad_k, nc.BEFORE) == E_INVALID
        assert lib.lccrf_get_pairwise_normalization(h.h, bad_k, C.byref(mode)) == E_INVALID
    assert lib.lccrf_get_pairwise_normalization(h.h, 0, None) == E_INVALID
    assert [h.get_normalization(k) for k in range(K)] == [nc.SYMMETRIC] * K
    h.inference(4, False, 0.7)
    before = h.probability()
    g = torch.zeros((500, 4), device="cuda")
    gu = torch.zeros((500, 4), device="cuda")
    gf = [torch.zeros((500, 2), device="cuda"), torch.zeros((500, 3), device="cuda")]
    ptrs = (C.c_void_p * 2)(*[C.c_void_p(t.data_ptr()) for t in gf])
    torch.cuda.synchronize()
    vp = C.c_void_p
    assert lib.lccrf_inference_backward_features(h.h, 4, 0.7, vp(g.data_ptr()), vp(gu.data_ptr()), None, ptrs) == E_STATE
    assert lib.lccrf_inference_backward_all(h.h, 4, 0.7, vp(g.data_ptr()), vp(gu.data_ptr()), None, ptrs, None) == E_STATE
    h.inference(4, False, 0.7)
    assert cc.same_bits(h.probability(), before)
    # without feature outputs lccrf_inference_backward_all is lccrf_inference_backward_compat: allowed
    assert lib.lccrf_inference_backward_all(h.h, 4, 0.7, vp(g.data_ptr()), vp(gu.data_ptr()), None, None, None) == 0
    h.synchronize()
    h.close()


# ---- GPU: torch -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layer_gradients_match_the_checker_and_sgd_lowers_the_loss(po, wl, golden):
    """MeanFieldCRF(normalization=SYMMETRIC) on L21:d3_d5: unary.grad and weights.grad against the float64 checker (identity
    matrices) on the bar of test_gradients_match_the_checker.  Then a student that starts at the case's weights learns from the
    Q of a teacher with half of them: plain SGD on the mean cross-entropy with a step of 1.0, chosen on the float64 checker -- there
    the loss falls 5.515 -> 4.148 -> 3.138 -> 2.682 (a step of 10 stalls after one)."""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb, U, nrm = _prepared("L21:d3_d5", golden, po, wl)
    K, L, N = 2, pb["L"], pb["N"]
    w0 = [float(w) for _, w in pb["kernels"]]
    layer = ag.MeanFieldCRF(N, L, nc.feats(pb), w0, n_iterations=5, relax=0.7, normalization=pkg.NORMALIZE_SYMMETRIC)
    assert [layer.crf.get_normalization(k) for k in range(K)] == [nc.SYMMETRIC] * K
    u = torch.from_numpy(U).cuda().requires_grad_(True)
    G = np.random.default_rng(2).standard_normal((N, L))
    q = layer(u)
    q.backward(torch.from_numpy(G.astype(np.float32)).cuda())
    torch.cuda.synchronize()
    o, lats, U64 = gs.checker(po, pb)
    o.close()
    eyes = [np.eye(L, dtype=np.float32)] * K
    at = gset.device_iterates(po, pb, 5, 0.7, None, [nc.SYMMETRIC] * K, [np.float32(x) for x in w0], nrm)
    r = gs.compat_reference(U64, np.array(w0), eyes, lats, 5, 0.7, G, "layer", [nc.SYMMETRIC] * K, at)
    r.check({"dL/dU": u.grad.cpu().numpy(), "dL/dw": layer.weights.grad.numpy()})
    layer.close()

    student = ag.MeanFieldCRF(N, L, nc.feats(pb), w0, n_iterations=5, normalization=[pkg.NORMALIZE_SYMMETRIC] * K)
    uu = torch.from_numpy(U).cuda()
    with torch.no_grad():
        target = ag.mean_field(student.crf, uu, 0.5 * student.weights.detach(), 5).clone()
    opt = torch.optim.SGD(student.parameters(), lr=1.0)

    def loss_of():
        return -(target * torch.log(student(uu).clamp_min(1e-12))).sum(1).mean()

    losses = []
    for _ in range(3):
        loss = loss_of()
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        losses.append(loss_of().item())
    student.close()
    print("cross-entropy over three SGD steps:", losses)
    assert losses[-1] < losses[0], losses

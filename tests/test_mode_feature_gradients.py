"""Feature gradients under every normalisation mode: lccrf_inference_backward_modes and lccrf_batch_inference_backward_modes
(include/lccrf.h sections 1m and 2i) and the torch layers on top (lc-crf-slam_amd/autograd.py: `normalization` of
mean_field_features, mean_field_learned, LearnedKernelCRF and LearnedCRF).

CPU: the symbols and methods; section 1m's sweep restated without autograd against the autograd reference
(tests/mode_feature_checker.py); every bar of every GPU setting under the cap; the bars reject a reference that holds the norm, or the
factor in front of the filter alone, constant.  GPU: the entry point against the reference under grad_support's bars, its bit
contracts against lccrf_inference_backward_all, routes, refusals and argument checks; a ragged batch frame by frame against handles;
a handle in locality mode; the torch layers."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import batch_learned_cases as bl
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import joint_checker as jc
import mode_feature_checker as mc
import normalization_checker as nc
from abi_support import assert_declared_exported_bound, dev, hip_malloc, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
NEW_SYMBOLS = ("lccrf_inference_backward_modes", "lccrf_batch_inference_backward_modes")
E_INVALID, E_STATE = -1, -5


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, NEW_SYMBOLS)
    assert lib.lccrf_abi_version() == 3                         # sections 1m and 2i came without a version step
    assert callable(getattr(pkg.DenseCRFHIP, "inference_backward_modes_device", None))
    assert callable(getattr(pkg.BatchCRF, "inference_backward_modes_device", None))


def test_entry_points_reject_a_null_handle(lib):
    assert lib.lccrf_inference_backward_modes(None, 1, 1.0, None, None, None, None, None) == E_INVALID
    assert lib.lccrf_batch_inference_backward_modes(None, 1, 1.0, None, None, None, None, None, None, None) == E_INVALID


def test_torch_layers_take_normalization():
    """the signatures of mean_field_features, mean_field_learned and the two layers are pinned
    (tests/test_fused_backward_features_resources.py), so `normalization` arrives as the functions' _modes twins and as an attribute
    of the layers, None after construction"""
    import inspect
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    p = list(inspect.signature(ag.mean_field_features_modes).parameters)
    assert p == ["unary", "features", "weights", "normalization", "n_iterations", "relax", "device", "fused_backward", "route_out"]
    p = list(inspect.signature(ag.mean_field_learned_modes).parameters)
    assert p == ["unary", "features", "weights", "compat", "normalization", "n_iterations", "relax", "device"]
    src = inspect.getsource(ag.LearnedKernelCRF.__init__)
    assert "self.normalization = None" in src and issubclass(ag.LearnedCRF, ag.LearnedKernelCRF)


RESTATED = [([nc.BEFORE, nc.SYMMETRIC], 1, 1.0), ([nc.SYMMETRIC, nc.NONE], 3, 0.7), ([nc.AFTER, nc.BEFORE], 3, 1.0),
            ([nc.SYMMETRIC, nc.SYMMETRIC], 0, 1.0)]


@pytest.mark.parametrize("modes,T,relax", RESTATED, ids=["%s-T%d-r%g" % ("+".join(nc.MODE_NAMES[m] for m in ms), T, r) for ms, T, r in RESTATED])
def test_the_restated_sweep_is_the_autograd_reference(po, wl, modes, T, relax):
    """Section 1m's sweep in float64 without autograd against autograd through the forward, 200 points, L = 4, d = 2 and 3, dense
    matrices, free and pinned iterates.  Measured: the largest relative L2 difference over every output and setting is 9.6e-15
    (dL/df of the d = 3 term under [AFTER, BEFORE], T = 3); asserted with a margin of about 200."""
    pb = wl.generic_problem(200, [2, 3], 4, seed=5, spread=1.5)
    o, lats, U = jc.checker(po, pb)
    nrm = [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    w = np.array([float(x) for x in nc.weights_f32(pb, nrm, modes)])
    G, mu = jc.grad_prob(pb), jc.checker_mu(jc.dense(2, 4), 4)
    for at in (None, gset.device_iterates(po, pb, T, relax, jc.dense(2, 4), modes, [np.float32(x) for x in w], nrm)):
        ref = mc.mode_gradients(U, w, mu, lats, modes, T, relax, G, at=at)
        got = mc.sweep_f64(U, w, mu, lats, modes, T, relax, G, at=at)
        for n, a, b in zip(mc.NAMES + ("dL/df0", "dL/df1"), got[:3] + tuple(got[3]), ref[:3] + tuple(ref[3])):
            e = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
            print("%s %s: restated sweep against autograd, relative L2 %.3g (|ref| %.3g)" % ("pinned" if at is not None else "free", n, e, np.linalg.norm(b)))
            assert e <= 2e-12, (n, e)
        if T == 0:
            assert all(np.all(a == 0) for a in got[3]) and all(np.all(a == 0) for a in ref[3])
        else:
            assert all(np.linalg.norm(a) > 0 for a in ref[3])


GROUPS = sorted({(n, ms, kind) for n, ms, T, r, kind in mc.SETTINGS}, key=str)
GROUP_IDS = ["%s-%s-%s" % (n, "+".join(nc.MODE_NAMES[m] for m in ms), kind) for n, ms, kind in GROUPS]


@pytest.mark.parametrize("name,ms,kind", GROUPS, ids=GROUP_IDS)
def test_every_bar_is_under_the_cap_and_held_factors_are_rejected(po, wl, golden, name, ms, kind):
    """Per (case, modes, matrices): every setting's bars <= BAR_CAP; and at T >= 1 the float64 reference with n held constant, and
    with the factor in front of the filter alone held constant, misses the L2 bar of dL/df of every BEFORE or SYMMETRIC term by more
    than a factor of 2 (a device within its bar can hide up to one bar of a fault)."""
    bad = []
    for T in mc.T_SET:
        for relax in mc.RELAX_SET:
            r = mc.reference_for(po, wl, golden, name, ms, T, relax, kind)
            bars = r["ref"].bars()
            for n, (bar, rbar, f, fr) in bars.items():
                if n == "dL/dmu" and not r["dense"]:
                    continue                                     # (not asked for on a Potts handle)
                print("%s %s: L2 bar %.3g%s" % (r["ref"].tag, n, bar, "" if rbar is None else ", row bar %.3g" % rbar))
                if bar > gs.BAR_CAP or (rbar is not None and rbar > gs.BAR_CAP):
                    bad.append((T, relax, n, bar, rbar))
            if T == 0:
                continue
            mu = jc.checker_mu(r["mats"], r["pb"]["L"])
            for what in ("n", "pre"):
                with mc.held(what):
                    got = mc.mode_gradients(r["U"], r["w64"], mu, r["lats"], r["modes"], T, relax, r["G"], at=r["at"])[3]
                for k, m in enumerate(r["modes"]):
                    if m in (nc.BEFORE, nc.SYMMETRIC):
                        n = "dL/df%d" % k
                        moved = gs.rel(got[k], r["ref"].ref[n], r["ref"].floors[n])
                        print("%s %s with %s held constant: moved by %.3g, bar %.3g" % (r["ref"].tag, n, what, moved, bars[n][0]))
                        assert moved > 2 * bars[n][0], (what, n, moved, bars[n][0])
    assert not bad, "bars beyond %g check nothing: %s" % (gs.BAR_CAP, bad)


# ---- GPU 1: against the reference ---------------------------------------------------------------------------------------------
def _handle(r):
    return mc.handle(r["pb"], r["w"], r["modes"], r["mats"])


def _check(got, r, T):
    assert all(np.isfinite(a).all() for a in got[:3 if r["dense"] else 2]) and all(np.isfinite(a).all() for a in got[3])
    named = gs._named(got[:3] if r["dense"] else got[:2], got[3])
    r["ref"].check(named)
    if T == 0:
        assert np.all(got[1] == 0) and all(np.all(a == 0) for a in got[3]) and (not r["dense"] or np.all(got[2] == 0))


@pytest.mark.gpu
@pytest.mark.parametrize("name,ms,T,relax,kind", mc.SETTINGS, ids=[mc.setting_id(s) for s in mc.SETTINGS])
def test_gradients_match_the_reference(po, wl, golden, name, ms, T, relax, kind):
    """Every output, pre-filled with NaN, against the float64 reference under grad_support's bars; T = 0: dL/df exactly 0.
    Measured on the MI355X: notes/normalization.md section 7."""
    r = mc.reference_for(po, wl, golden, name, ms, T, relax, kind)
    h = _handle(r)
    got = mc.backward(h, r["dims"], r["pb"]["L"], T, relax, r["G"], compat=r["dense"])
    h.close()
    if not r["dense"]:
        assert np.isnan(got[2]).all()                            # d_grad_compat == NULL: nothing written
    _check(got, r, T)


# ---- GPU 2: contracts -----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(cc.same_bits(x, y) for x, y in zip(a, b))


def _slam(po, wl, golden):
    pb, U, nrm = gset.norm_prepared("slam1001:s38", golden, po, wl)
    G = np.random.default_rng(9).standard_normal((pb["N"], 2))
    return pb, nrm, G


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_all_after_is_the_all_call_with_its_route(po, wl, golden, fused):
    pb, nrm, G = _slam(po, wl, golden)
    w = nc.weights_f32(pb, nrm, [nc.AFTER] * 2)
    for mats, compat in (([None, None], False), (jc.dense(2, 2), True)):
        h = mc.handle(pb, w, [nc.AFTER] * 2, mats)
        h.set_option(pkg.OPT_FUSED_BACKWARD_FEATURES, fused)
        a = mc.backward(h, [2, 2], 2, 5, 0.7, G, compat=compat, entry="all")
        route = h.backward_route()
        b = mc.backward(h, [2, 2], 2, 5, 0.7, G, compat=compat, entry="modes")
        assert h.backward_route() == route
        assert route == (pkg.BACKWARD_FUSED if fused and not compat else pkg.BACKWARD_STREAM)
        assert cc.same_bits(a[0], b[0]) and cc.same_bits(a[1], b[1]) and _same(a[3], b[3])
        assert cc.same_bits(a[2], b[2]) if compat else np.isnan(b[2]).all()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("modes", [[nc.SYMMETRIC, nc.BEFORE], [nc.NONE, nc.SYMMETRIC], [nc.BEFORE, nc.AFTER]],
                         ids=lambda ms: "+".join(nc.MODE_NAMES[m] for m in ms))
@pytest.mark.parametrize("dense", [False, True], ids=["potts", "dense"])
def test_bits_of_the_all_call_null_entries_determinism_route_and_refusals(po, wl, golden, lib, modes, dense):
    import torch
    pb, nrm, G = _slam(po, wl, golden)
    w = nc.weights_f32(pb, nrm, modes)
    mats = jc.dense(2, 2) if dense else [None, None]
    T, relax, dims = 5, 0.7, [2, 2]
    h = mc.handle(pb, w, modes, mats)
    e = mc.backward(h, dims, 2, T, relax, G, features=False, compat=dense, entry="all")     # the same handle, no features
    a = mc.backward(h, dims, 2, T, relax, G, compat=dense)
    assert h.backward_route() == pkg.BACKWARD_STREAM
    assert cc.same_bits(a[0], e[0]) and cc.same_bits(a[1], e[1]) and (cc.same_bits(a[2], e[2]) if dense else np.isnan(a[2]).all())
    assert all(np.isfinite(x).all() and np.linalg.norm(x) > 0 for x in a[3])
    q_after = h.probability()
    b = mc.backward(h, dims, 2, T, relax, G, compat=dense)                                  # run to run
    assert _same(a[:2], b[:2]) and _same(a[3], b[3]) and (not dense or cc.same_bits(a[2], b[2]))
    c = mc.backward(h, dims, 2, T, relax, G, features=False, compat=dense)                  # d_grad_features == NULL: the _all call
    assert _same(c[:2], e[:2]) and all(np.isnan(x).all() for x in c[3])
    for skip in range(2):                                                                   # a NULL entry
        c = mc.backward(h, dims, 2, T, relax, G, skip=(skip,), compat=dense)
        assert _same(c[:2], e[:2]) and c[3][skip] is None and cc.same_bits(c[3][1 - skip], a[3][1 - skip])
        assert not dense or cc.same_bits(c[2], e[2])
    c = mc.backward(h, dims, 2, T, relax, G, unary=False, weights=False, compat=dense)      # NULL dL/dU and dL/dw
    assert np.isnan(c[0]).all() and np.isnan(c[1]).all() and _same(c[3], a[3])
    for opt in (pkg.OPT_FUSED_BACKWARD, pkg.OPT_FUSED_BACKWARD_LEARNT, pkg.OPT_FUSED_BACKWARD_FEATURES):   # STREAM under each
        h.set_option(opt, 1)
        c = mc.backward(h, dims, 2, T, relax, G, compat=dense)
        assert h.backward_route() == pkg.BACKWARD_STREAM, opt
        assert _same(c[:2], a[:2]) and _same(c[3], a[3])
        h.set_option(opt, 0)
    # the entry points of sections 1d and 1f still refuse, and leave the handle as it was
    g, gu = dev(G.astype(np.float32)), torch.zeros((pb["N"], 2), device="cuda")
    gf = [torch.zeros((pb["N"], 2), device="cuda") for _ in range(2)]
    vp = C.c_void_p
    ptrs = (vp * 2)(*[vp(t.data_ptr()) for t in gf])
    torch.cuda.synchronize()
    if not dense:
        assert lib.lccrf_inference_backward_features(h.h, T, relax, vp(g.data_ptr()), vp(gu.data_ptr()), None, ptrs) == E_STATE
    assert lib.lccrf_inference_backward_all(h.h, T, relax, vp(g.data_ptr()), vp(gu.data_ptr()), None, ptrs, None) == E_STATE
    c = mc.backward(h, dims, 2, T, relax, G, compat=dense)
    assert _same(c[:2], a[:2]) and _same(c[3], a[3])
    assert cc.same_bits(h.probability(), q_after)
    h.inference(T, False, relax)                                                            # Q afterwards as lccrf_inference leaves it
    assert cc.same_bits(h.probability(), q_after)
    h2 = mc.handle(pb, w, modes, mats)                                                      # a fresh handle whose first call is this one
    d = mc.backward(h2, dims, 2, T, relax, G, compat=dense)
    assert _same(d[:2], a[:2]) and _same(d[3], a[3])
    z = mc.backward(h2, dims, 2, 0, relax, G, compat=dense)                                 # n_iterations = 0
    assert all(np.all(x == 0) for x in z[3]) and np.all(z[1] == 0)
    h.close(), h2.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_handle_as_it_was(po, wl):
    import torch
    pb = wl.generic_problem(500, [2, 3], 4, seed=17)
    N, L = 500, 4
    h = cc.setup(pkg.DenseCRFHIP, pb)
    jc.set_all(h, jc.dense(2, L))
    h.set_normalization(0, nc.SYMMETRIC), h.set_normalization(1, nc.BEFORE)
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
            assert lb.lccrf_inference_backward_modes(h.h, *args) == E_INVALID, args
        h0 = pkg.DenseCRFHIP(N, L)                               # no unary yet
        h0.add_pairwise(pb["kernels"][0][0], 1.0)
        h0.set_normalization(0, nc.SYMMETRIC)
        assert lb.lccrf_inference_backward_modes(h0.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, arr(vp(gf[0].data_ptr())), None) == E_STATE
        h0.close()
    finally:
        hl.hipFree(small)
    h.inference(4, False, 0.7)
    assert cc.same_bits(h.probability(), before)
    h.close()


# ---- GPU 3: a batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["potts", "dense"])
def test_every_frame_of_a_ragged_batch_has_the_bits_of_its_handle(golden, wl, dense):
    """frames of 300, 0, 1001 and 77 points in a batch of max_points 1008, modes [SYMMETRIC, BEFORE]"""
    Ns = (300, 0, 1001, 77)
    fr = bc.slam_frames(golden, wl, Ns=Ns)
    fr = bc.Frames(fr.probs, fr.w, max_points=max(Ns) + bl.SLACK)
    modes, mats = [nc.SYMMETRIC, nc.BEFORE], (jc.dense(2, 2) if dense else [None, None])
    b = fr.batch()
    bl.apply(b, modes, mats)
    handles = {f: bl.handle(fr, f, modes, mats, None) for f, n in enumerate(fr.N) if n}
    for T, relax in ((5, 0.7), (1, 1.0), (0, 1.0)):
        G = fr.grad_prob(100 * T + 3)
        out = mc.batch_backward(b, fr, T, relax, G)
        assert b.backward_route() == pkg.BACKWARD_STREAM
        ref = mc.batch_backward(b, fr, T, relax, G, features=False, entry="all")             # section 2h on the same batch
        assert cc.same_bits(out["model"], ref["model"]) and cc.same_bits(out["gu"], ref["gu"])
        assert cc.same_bits(out["gw"], ref["gw"]) and cc.same_bits(out["gm"], ref["gm"])
        assert cc.same_bits(out["model"], bl.model_of(out["gw"], out["gm"]))
        for f, n in enumerate(fr.N):
            where = "frame %d (N=%d) T=%d relax=%g" % (f, n, T, relax)
            assert np.all(out["gu"][f, n:] == 0) and all(np.all(a[f, n:] == 0) for a in out["gf"]), where
            if n == 0:
                assert np.all(out["gw"][f] == 0) and np.all(out["gm"][f] == 0), where
                continue
            hu, hw, hm, hf = mc.backward(handles[f], fr.dims, 2, T, relax, G[f, :n])
            assert cc.same_bits(out["gu"][f, :n], hu) and cc.same_bits(out["gw"][f], hw) and cc.same_bits(out["gm"][f], hm), where
            for k in range(2):
                assert cc.same_bits(out["gf"][k][f, :n], hf[k]), where + ": dL/df%d" % k
                assert T == 0 or np.linalg.norm(hf[k]) > 0, where
                assert T > 0 or np.all(hf[k] == 0), where
    # the batch entry points of sections 2d and 2h still refuse
    import torch
    vp = C.c_void_p
    g, gf = dev(np.nan_to_num(fr.grad_prob(1))), [torch.zeros((len(Ns), fr.maxN, 2), device="cuda") for _ in range(2)]
    ptrs = (vp * 2)(*[vp(t.data_ptr()) for t in gf])
    torch.cuda.synchronize()
    assert pkg.lib().lccrf_batch_inference_backward_all(b.h, 1, 1.0, vp(g.data_ptr()), None, None, ptrs, None, None, None) == E_STATE
    assert pkg.lib().lccrf_batch_inference_backward_features(b.h, 1, 1.0, vp(g.data_ptr()), None, None, ptrs, None) == E_STATE
    for h in handles.values():
        h.close()
    b.close()


# ---- GPU 4: locality mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_locality_mode_symmetric(po, wl):
    """8192 points (lccrf_inference runs in its internal point order), two labels, two 2-D terms, SYMMETRIC, T = 1: the handle is
    re-built the plain way and dL/df comes back in the caller's order, within its bars"""
    pb = wl.generic_problem(8192, [2, 2], 2, seed=31)
    modes = [nc.SYMMETRIC] * 2
    o, lats, U = jc.checker(po, pb)
    nrm = [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    w = nc.weights_f32(pb, nrm, modes)
    G = gset.grad_prob(pb)
    ref = mc.mode_reference(U, np.array([float(x) for x in w]), jc.checker_mu([None, None], 2), lats, modes, 1, 1.0, G, "locality symmetric")
    h = mc.handle(pb, w, modes)
    h.inference(1, True, 1.0)                                    # (locality mode first: the backward has something to re-build)
    got = mc.backward(h, [2, 2], 2, 1, 1.0, G, compat=False)
    h.close()
    ref.check(gs._named(got[:2], got[3]))


# ---- GPU 5: torch -------------------------------------------------------------------------------------------------------------------
def _torch_case(wl, po):
    pb = wl.generic_problem(257, [2, 3], 3, seed=11)
    o = cc.setup(po.OracleCRF, pb)
    U = o.unary()
    o.close()
    sd = [[1.5, 2.0], [1.2]]
    groups = [[[0], [1]], [[0, 1, 2]]]
    cols = [np.array([0, 1]), np.array([0, 0, 0])]
    raw = [np.ascontiguousarray(f * np.array(s, np.float32)[c], np.float32) for (f, _), s, c in zip(pb["kernels"], sd, cols)]
    return pb, U, raw, sd, groups, cols, [float(np.float32(w)) for _, w in pb["kernels"]]


def _assert_chain(layer, gf):
    """log_sd.grad of every term is the chain rule on dL/d features `gf`: f = raw * exp(-log_sd)[col], so d f / d log_sd = -f and
    dL/dlog_sd[j] = -sum over the rows and the columns c of group j of gf[i][c] * f[i][c].  The sum is torch's, in float32 and in
    an order of its own: it is held to the float64 sum of the same float32 terms within n eps sum |terms| (n terms, eps = 2^-24, the
    bound of any order of float32 additions) plus one rounding of each product."""
    for k, (f, col, g, p) in enumerate(zip(layer.features(), layer._col, gf, layer.log_sd)):
        terms = g.astype(np.float64) * f.detach().cpu().numpy().astype(np.float64)
        col = col.cpu().numpy()
        got = p.grad.cpu().numpy().astype(np.float64)
        for j in range(len(got)):
            t = terms[:, col == j]
            want, bound = -t.sum(), (t.size + 1) * 2.0 ** -24 * np.abs(t).sum()
            print("log_sd.grad[%d][%d] %.9g, chain rule %.9g, |difference| %.3g (bound %.3g)" % (k, j, got[j], want, abs(got[j] - want), bound))
            assert want != 0 and abs(got[j] - want) <= bound, (k, j, got[j], want, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["kernel", "learned"])
def test_layers_return_the_chain_rule_on_the_c_abi_bits(po, wl, which):
    """LearnedKernelCRF with normalization = SYMMETRIC and LearnedCRF with normalization = [SYMMETRIC, AFTER] on 257 points: log_sd.grad,
    weights.grad and compat.grad are the chain rule on the outputs of lccrf_inference_backward_modes; a second backward is refused"""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb, U, raw, sd, groups, cols, w = _torch_case(wl, po)
    N, L, T, relax = pb["N"], pb["L"], 5, 0.7
    if which == "kernel":
        layer = ag.LearnedKernelCRF(raw, sd, w, groups=groups, n_iterations=T, relax=relax)
        layer.normalization = pkg.NORMALIZE_SYMMETRIC
        modes, mats = [nc.SYMMETRIC] * 2, [None, None]
    else:
        layer = ag.LearnedCRF(raw, sd, w, groups=groups, n_labels=L, n_iterations=T, relax=relax)
        layer.normalization = [pkg.NORMALIZE_SYMMETRIC, pkg.NORMALIZE_AFTER]
        modes, mats = [nc.SYMMETRIC, nc.AFTER], jc.dense(2, L)
        with torch.no_grad():
            layer.compat.copy_(torch.tensor(np.stack(mats)))
    u = torch.from_numpy(U).cuda().requires_grad_(True)
    G = np.random.default_rng(2).standard_normal((N, L)).astype(np.float32)
    q = layer(u)
    q.backward(torch.from_numpy(G).cuda(), retain_graph=True)
    torch.cuda.synchronize()
    feats = [f.detach().cpu().numpy() for f in layer.features()]
    h = pkg.DenseCRFHIP(N, L)
    h.set_unary(U)
    for f, x in zip(feats, w):
        h.add_pairwise(f, x)
    for k, m in enumerate(modes):
        h.set_normalization(k, m)
    for k, m in enumerate(mats):
        if m is not None:
            h.set_pairwise_compatibility(k, m)
    ref = mc.backward(h, [2, 3], L, T, relax, G, compat=which == "learned")
    assert h.backward_route() == pkg.BACKWARD_STREAM
    h.inference(T, False, relax)
    assert cc.same_bits(q.detach().cpu().numpy(), h.probability())
    h.close()
    assert cc.same_bits(u.grad.cpu().numpy(), ref[0]) and cc.same_bits(layer.weights.grad.numpy(), ref[1])
    if which == "learned":
        assert cc.same_bits(layer.compat.grad.numpy(), ref[2])
    else:
        assert layer.backward_route == pkg.BACKWARD_STREAM
    _assert_chain(layer, ref[3])
    with pytest.raises(RuntimeError, match="backward a second time"):
        q.backward(torch.from_numpy(G).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_normalization_none_is_the_layer_as_it_was(po, wl, fused):
    """normalization=None and an explicit AFTER: the bits and the route of lccrf_inference_backward_all, the fused route included"""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.slam_problem(257, seed=4)
    o = cc.setup(po.OracleCRF, pb)
    U = o.unary()
    o.close()
    raw = [np.ascontiguousarray(f, np.float32) for f, _ in pb["kernels"]]
    w = [float(np.float32(x)) for _, x in pb["kernels"]]
    G = np.random.default_rng(3).standard_normal((257, 2)).astype(np.float32)
    h = pkg.DenseCRFHIP(257, 2)
    h.set_unary(U)
    for f, x in zip(raw, w):
        h.add_pairwise(f, x)
    h.set_option(pkg.OPT_FUSED_BACKWARD_FEATURES, int(fused))
    ref = mc.backward(h, [2, 2], 2, 5, 1.0, G, compat=False, entry="all")
    route = h.backward_route()
    h.close()
    assert route == (pkg.BACKWARD_FUSED if fused else pkg.BACKWARD_STREAM)
    for normalization in (None, pkg.NORMALIZE_AFTER):
        layer = ag.LearnedKernelCRF(raw, [[1.0, 1.0]] * 2, w, n_iterations=5, fused_backward=fused)
        assert layer.normalization is None
        layer.normalization = normalization
        u = torch.from_numpy(U).cuda().requires_grad_(True)
        layer(u).backward(torch.from_numpy(G).cuda())
        torch.cuda.synchronize()
        assert layer.backward_route == route
        assert cc.same_bits(u.grad.cpu().numpy(), ref[0]) and cc.same_bits(layer.weights.grad.numpy(), ref[1])
        _assert_chain(layer, ref[3])

"""The one-launch backward WITH feature gradients (include/lccrf.h section 1l, LCCRF_OPT_FUSED_BACKWARD_FEATURES;
csrc/fused_backward_features.hip) against the streaming sweep it replaces: every comparison is bit for bit, option on against option
off on the same object -- dL/dU with its zero rows, dL/dw, every dL/df_k with its zero rows and the Q left behind -- and the route is
asserted both ways.  Then the float64 checker under the existing bars, and the torch layers' keyword."""
import ctypes as C
import importlib

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
from abi_support import dev, hip_malloc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

OPT = pkg.OPT_FUSED_BACKWARD_FEATURES
STREAM, FUSED = pkg.BACKWARD_STREAM, pkg.BACKWARD_FUSED
# phantom points at each N % 4, wavefront and 256-point partial-block edges, 1 -> 2 points per lane, the plan's limit
HANDLE_NS = [1, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2000, 2047, 2048]
T_SET, RELAX_SET = [1, 2, 5, 10], [1.0, 0.7]
TERMS = {"both": slice(0, 2), "appearance": slice(0, 1), "smoothness": slice(1, 2)}


def _problem(wl, N, terms="both", seed=None):
    pb = wl.slam_problem(N, seed=300 + N if seed is None else seed)
    return dict(pb, kernels=pb["kernels"][TERMS[terms]])


def _dims(pb):
    return [int(f.shape[1]) for f, _ in pb["kernels"]]


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


def _call(h, on, T, relax, G, dims, **kw):
    """one backward with the option on / off: (dL/dU, dL/dw, [dL/df_k], Q left behind, route)"""
    h.set_option(OPT, 1 if on else 0)
    gu, gw, gf = _backward_features(h, dims, T, relax, G, **kw)
    return gu, gw, gf, h.probability(), h.backward_route()


def _same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and cc.same_bits(x, y))


def _assert_same(a, b, what):
    for name, x, y in zip(("dL/dU", "dL/dw"), a[:2], b[:2]):
        assert cc.same_bits(x, y), "%s: %s differs" % (what, name)       # (NaN-filled where the call was given NULL: the same bits too)
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert _same(x, y), "%s: dL/df%d differs (max |d| %g)" % (what, k, np.abs(x.astype(np.float64) - y).max())
        assert x is None or np.isfinite(x).all(), "%s: dL/df%d not finite" % (what, k)
    assert cc.same_bits(a[3], b[3]), "%s: Q differs" % what


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
        dims = _dims(pb)
        h = cc.setup(pkg.DenseCRFHIP, pb)
        assert h.backward_route() == pkg.BACKWARD_NONE
        for T in T_SET:
            for relax in RELAX_SET:
                what = "N=%d %s T=%d relax=%g" % (N, terms, T, relax)
                G = np.random.default_rng(1000 * T + int(10 * relax)).standard_normal((N, 2))
                off = _call(h, False, T, relax, G, dims)
                assert off[4] == STREAM, what
                on = _call(h, True, T, relax, G, dims)
                assert on[4] == FUSED, what
                _assert_same(on, off, what)
        h.close()


@pytest.mark.parametrize("N", [5, 257, 1025, 2048])
def test_null_arrays_leave_the_other_bits_unchanged(wl, N):
    """with two terms each single feature array left NULL: the other term's bits are unchanged (and the route is still this option's);
    NULL d_grad_unary / d_grad_weights change nothing else"""
    pb = _problem(wl, N)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    T, relax = 5, 0.7
    G = np.random.default_rng(N).standard_normal((N, 2))
    full = _call(h, True, T, relax, G, [2, 2])
    assert full[4] == FUSED
    for skip in (0, 1):
        what = "N=%d without dL/df%d" % (N, skip)
        off = _call(h, False, T, relax, G, [2, 2], skip=(skip,))
        on = _call(h, True, T, relax, G, [2, 2], skip=(skip,))
        assert off[4] == STREAM and on[4] == FUSED, what
        _assert_same(on, off, what)
        assert on[2][skip] is None and cc.same_bits(on[2][1 - skip], full[2][1 - skip]), what
        assert cc.same_bits(on[0], full[0]) and cc.same_bits(on[1], full[1]), what
    for kw in (dict(unary=False), dict(weights=False), dict(unary=False, weights=False)):
        on = _call(h, True, T, relax, G, [2, 2], **kw)
        off = _call(h, False, T, relax, G, [2, 2], **kw)
        assert on[4] == FUSED and off[4] == STREAM, kw
        _assert_same(on, off, "N=%d %r" % (N, kw))
        assert np.isnan(on[0]).all() == (not kw.get("unary", True)) and np.isnan(on[1]).all() == (not kw.get("weights", True))
        assert all(cc.same_bits(x, y) for x, y in zip(on[2], full[2])), kw
    h.close()


def test_short_rows_and_chain_rows_both_occur(wl):
    """which frames of the handle test ran the first term on chain rows (as tests/test_fused_backward.py finds: with both terms the
    large frames, the smoothness term alone never)"""
    chain = {}
    for terms in ("both", "smoothness"):
        for N in HANDLE_NS:
            pb = _problem(wl, N, terms)
            h = cc.setup(pkg.DenseCRFHIP, pb)
            on = _call(h, True, 1, 1.0, np.zeros((N, 2)), _dims(pb))
            assert on[4] == FUSED
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
    dims = _dims(pb)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(8).standard_normal((pb["N"], pb["L"]))
    for T, relax in ((5, 1.0), (2, 0.7)):
        off = _call(h, False, T, relax, G, dims)
        on = _call(h, True, T, relax, G, dims)
        assert off[4] == STREAM and on[4] == STREAM, (kind, off[4], on[4])
        _assert_same(on, off, kind)
    h.close()


def test_t0_gives_exact_zeros_on_either_route(wl):
    pb = _problem(wl, 700, seed=2)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(5).standard_normal((700, 2))
    off = _call(h, False, 0, 1.0, G, [2, 2])
    on = _call(h, True, 0, 1.0, G, [2, 2])
    assert off[4] == STREAM and on[4] in (STREAM, FUSED)
    _assert_same(on, off, "T=0")
    assert np.all(on[1] == 0) and all(np.all(a == 0) and not np.signbit(a).any() for a in on[2])
    h.close()


# ---- option interplay --------------------------------------------------------------------------------------------------------------
def test_each_option_selects_its_own_requests(wl):
    pb = _problem(wl, 2000, seed=4)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(3).standard_normal((2000, 2))
    ref = _call(h, False, 5, 0.7, G, [2, 2])
    # option 8 alone on a request without feature arrays: the sweep -- through section 1c's entry and through section 1d's with NULLs
    h.set_option(OPT, 1)
    ru, rw = gs.backward(h, 5, 0.7, G, 2)
    assert h.backward_route() == STREAM and cc.same_bits(ru, ref[0]) and cc.same_bits(rw, ref[1])
    none = _call(h, True, 5, 0.7, G, [2, 2], skip=(0, 1))
    assert none[4] == STREAM and cc.same_bits(none[0], ref[0]) and cc.same_bits(none[1], ref[1])
    h.set_option(OPT, 0)
    # options 6 and 7 alone on a request with feature arrays: the sweep; without feature arrays option 6 keeps its route
    for other in (pkg.OPT_FUSED_BACKWARD, pkg.OPT_FUSED_BACKWARD_LEARNT):
        h.set_option(other, 1)
        got = _call(h, False, 5, 0.7, G, [2, 2])
        assert got[4] == STREAM, other
        _assert_same(got, ref, "option %d alone" % other)
        h.set_option(other, 0)
    for other in (pkg.OPT_FUSED_BACKWARD, pkg.OPT_FUSED_BACKWARD_LEARNT):
        h.set_option(other, 1)
    both = _call(h, True, 5, 0.7, G, [2, 2])                  # all three set: the feature request is option 8's ...
    assert both[4] == FUSED
    _assert_same(both, ref, "options 6, 7 and 8")
    ru, rw = gs.backward(h, 5, 0.7, G, 2)                      # ... and the plain one option 6's
    assert h.backward_route() == FUSED and cc.same_bits(ru, ref[0]) and cc.same_bits(rw, ref[1])
    h.close()


def _backward_all(h, T, relax, G, K):
    """lccrf_inference_backward_all with feature arrays and dL/dmu: (dL/dU, dL/dw, [dL/df_k], dL/dmu, route)"""
    import torch
    N = G.shape[0]
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((K,), float("nan"), device="cuda")
    gf = [torch.full((N, 2), float("nan"), device="cuda") for _ in range(K)]
    gm = torch.full((K, 2, 2), float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_all_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [t.data_ptr() for t in gf], gm.data_ptr())
    h.synchronize()
    return gu.cpu().numpy(), gw.cpu().numpy(), [t.cpu().numpy() for t in gf], gm.cpu().numpy(), h.backward_route()


def test_a_matrix_or_a_mode_keeps_its_behaviour(wl):
    """a handle with a label-compatibility matrix: section 1d's entry refuses it either way, section 1f's call streams with the same
    bits; a handle with a mode other than AFTER: feature gradients are refused either way; back on Potts / AFTER the route is taken"""
    import torch
    pb = _problem(wl, 1500, seed=8)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(6).standard_normal((1500, 2))
    L = pkg.lib()
    g = dev(G.astype(np.float32))
    gu = torch.zeros((1500, 2), device="cuda")
    gf = [torch.zeros((1500, 2), device="cuda") for _ in range(2)]
    arr = (C.c_void_p * 2)(C.c_void_p(gf[0].data_ptr()), C.c_void_p(gf[1].data_ptr()))
    torch.cuda.synchronize()

    def features_entry():
        return L.lccrf_inference_backward_features(h.h, 5, 1.0, C.c_void_p(g.data_ptr()), C.c_void_p(gu.data_ptr()), None, arr)

    h.set_pairwise_compatibility(0, np.array([[1.0, 0.25], [0.5, 1.0]], np.float32))
    out = {}
    for on in (False, True):
        h.set_option(OPT, 1 if on else 0)
        assert features_entry() == -5, on
        out[on] = _backward_all(h, 5, 0.7, G, 2)
        assert out[on][4] == STREAM, on
    for x, y in zip(out[True][:2] + tuple(out[True][2]) + (out[True][3],), out[False][:2] + tuple(out[False][2]) + (out[False][3],)):
        assert cc.same_bits(x, y)
    h.set_pairwise_compatibility(0, None)
    h.set_normalization(1, pkg.NORMALIZE_SYMMETRIC)
    for on in (False, True):
        h.set_option(OPT, 1 if on else 0)
        assert features_entry() == -5, on
    h.set_normalization(1, pkg.NORMALIZE_AFTER)
    off = _call(h, False, 5, 0.7, G, [2, 2])
    on = _call(h, True, 5, 0.7, G, [2, 2])
    assert off[4] == STREAM and on[4] == FUSED
    _assert_same(on, off, "Potts / AFTER again")
    # section 1f's call that reduces to section 1d's request (what mean_field_features calls) is this option's too
    gm = None
    torch.cuda.synchronize()
    h.inference_backward_all_device(5, 0.7, g.data_ptr(), gu.data_ptr(), None, [t.data_ptr() for t in gf], gm)
    h.synchronize()
    assert h.backward_route() == FUSED
    assert cc.same_bits(gu.cpu().numpy(), on[0]) and all(cc.same_bits(t.cpu().numpy(), x) for t, x in zip(gf, on[2]))
    h.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------
RAGGED = (0, 5, 7, 257, 1000, 1001, 2000, 2048)


def _batch_call(b, fr, on, T, relax, G, skip=(), stream=None, all_entry=False):
    """(dL/dU, dL/dw, [dL/df_k], Q, route) of a batch; every output pre-filled with NaN"""
    import torch
    b.set_option(OPT, 1 if on else 0)
    F = len(fr.probs)
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((F, fr.K), float("nan"), device="cuda")
    gf = [None if k in skip else torch.full((F, fr.maxN, d), float("nan"), device="cuda") for k, d in enumerate(fr.dims)]
    ptrs = [t.data_ptr() if t is not None else None for t in gf]
    torch.cuda.synchronize()
    if all_entry:
        b.inference_backward_all_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), ptrs, None, None, stream=stream)
    else:
        b.inference_backward_features_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), ptrs, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return (gu.cpu().numpy(), gw.cpu().numpy(), [t.cpu().numpy() if t is not None else None for t in gf], b.probability(),
            b.backward_route())


def _assert_same_frames(a, b, N, what):
    assert cc.same_bits(a[0], b[0]), what + ": dL/dU differs"
    assert cc.same_bits(a[1], b[1]), what + ": dL/dw differs"
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert _same(x, y), "%s: dL/df%d differs" % (what, k)
    for f, n in enumerate(N):
        assert cc.same_bits(a[3][f, :n], b[3][f, :n]), "%s: Q of frame %d differs" % (what, f)


def _assert_handle_bits(fr, handles, got, T, relax, G):
    gu, gw, gf = got[:3]
    for f, n in enumerate(fr.N):
        for a in [gu] + gf:
            assert np.all(a[f, n:] == 0) and not np.signbit(a[f, n:]).any(), "frame %d: rows beyond n_points not +0" % f
        if n == 0:
            assert np.all(gw[f] == 0), "frame %d (0 points): weight gradient not 0" % f
            continue
        handles[f].set_option(OPT, 0)
        hu, hw, hf = _backward_features(handles[f], fr.dims, T, relax, G[f, :n])
        what = "frame %d (N=%d) T=%d relax=%g" % (f, n, T, relax)
        assert cc.same_bits(gu[f, :n], hu) and cc.same_bits(gw[f], hw), what
        assert all(cc.same_bits(gf[k][f, :n], hf[k]) for k in range(fr.K)), what


def test_ragged_batch_has_the_bits_of_the_sweep_and_of_its_handles(wl, golden):
    fr = bc.slam_frames(golden, wl, Ns=RAGGED)
    b = fr.batch()
    assert b.backward_route() == pkg.BACKWARD_NONE
    handles = {f: fr.handle(f) for f, n in enumerate(fr.N) if n}
    for T, relax in ((1, 0.7), (5, 1.0), (10, 0.7)):
        what = "T=%d relax=%g" % (T, relax)
        G = fr.grad_prob(7 + T)
        off = _batch_call(b, fr, False, T, relax, G)
        assert off[4] == STREAM
        on = _batch_call(b, fr, True, T, relax, G)
        assert on[4] == FUSED, what
        _assert_same_frames(on, off, fr.N, what)
        _assert_handle_bits(fr, handles, on, T, relax, G)
    # a NULL entry, and section 2h's entry when it reduces to section 2d's request
    G = fr.grad_prob(3)
    full = _batch_call(b, fr, True, 5, 0.7, G)
    part = _batch_call(b, fr, True, 5, 0.7, G, skip=(0,))
    assert part[4] == FUSED and part[2][0] is None and cc.same_bits(part[2][1], full[2][1]) and cc.same_bits(part[0], full[0])
    alle = _batch_call(b, fr, True, 5, 0.7, G, all_entry=True)
    assert alle[4] == FUSED
    _assert_same_frames(alle, full, fr.N, "lccrf_batch_inference_backward_all")
    alle_off = _batch_call(b, fr, False, 5, 0.7, G, all_entry=True)
    assert alle_off[4] == STREAM
    _assert_same_frames(alle, alle_off, fr.N, "lccrf_batch_inference_backward_all, option off")
    for h in handles.values():
        h.close()
    b.close()


def test_one_frame_beyond_the_plan_streams_the_whole_batch(wl, golden):
    fr = bc.slam_frames(golden, wl, Ns=RAGGED + (3000,))
    b = fr.batch()
    G = fr.grad_prob(3)
    off = _batch_call(b, fr, False, 5, 0.7, G)
    on = _batch_call(b, fr, True, 5, 0.7, G)
    assert off[4] == STREAM and on[4] == STREAM
    _assert_same_frames(on, off, fr.N, "with a 3000-point frame")
    b.close()


def test_rebound_batch_carries_no_stale_rows_or_accumulators(wl, golden):
    big = bc.slam_frames(golden, wl, Ns=(2002, 2002, 1500))
    b = big.batch()
    a1 = _batch_call(b, big, True, 5, 1.0, big.grad_prob(11))
    assert a1[4] == FUSED
    small = bc.slam_frames(golden, wl, Ns=(1001, 5))
    small = bc.Frames(small.probs, small.w, max_points=2002)
    b.set_inputs_host(small.N, small.feats, unary=small.U)
    b.build()
    handles = {f: small.handle(f) for f in range(2)}
    for T, relax in ((5, 1.0), (10, 0.7), (1, 1.0)):
        G = small.grad_prob(T)
        on = _batch_call(b, small, True, T, relax, G)
        assert on[4] == FUSED
        _assert_handle_bits(small, handles, on, T, relax, G)
        off = _batch_call(b, small, False, T, relax, G)
        _assert_same_frames(on, off, small.N, "rebound T=%d" % T)
    for h in handles.values():
        h.close()
    b.close()
    assert all(np.isfinite(a).all() for a in a1[2])


def test_a_user_stream_is_honoured(wl, golden):
    import torch
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000, 0, 2000))
    b = fr.batch()
    G = fr.grad_prob(4)
    off = _batch_call(b, fr, False, 5, 0.7, G)
    s = torch.cuda.Stream()
    on = _batch_call(b, fr, True, 5, 0.7, G, stream=s.cuda_stream)
    assert on[4] == FUSED
    _assert_same_frames(on, off, fr.N, "user stream")
    b.close()


# ---- state and determinism -----------------------------------------------------------------------------------------------------
def test_toggling_the_option_and_repeating_the_call(wl):
    pb = _problem(wl, 2000, seed=12)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(9).standard_normal((2000, 2))
    runs = [_call(h, on, 5, 0.7, G, [2, 2]) for on in (True, False, True, True, False)]
    assert [r[4] for r in runs] == [FUSED, STREAM, FUSED, FUSED, STREAM]
    for r in runs[1:]:
        _assert_same(r, runs[0], "toggled")
    h.inference(5, True, 0.7)                                   # the next inference is unchanged
    assert cc.same_bits(h.probability(), runs[0][3])
    h.close()


def test_argument_checks_with_the_option_on(po, wl, golden):
    """the cases of test_argument_checks_leave_the_handle_usable (tests/test_feature_gradients.py), with the same codes"""
    import torch
    pb = wl.slam_problem(2000, seed=4)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    h.set_option(OPT, 1)
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
        h0.set_option(OPT, 1)
        assert L.lccrf_inference_backward_features(h0.h, 1, 1.0, vp(g.data_ptr()), vp(gu.data_ptr()), None, None) == -5
        assert h0.backward_route() == pkg.BACKWARD_NONE
        h0.close()
    finally:
        hl.hipFree(small)
    assert h.backward_route() == pkg.BACKWARD_NONE               # no call has succeeded yet
    o = cc.setup(po.OracleCRF, pb)                               # still usable
    h.inference(5, True)
    o.inference_native(5, True)
    assert cc.same_bits(h.probability(), o.probability())
    torch.cuda.synchronize()
    h.inference_backward_features_device(5, 1.0, g.data_ptr(), gu.data_ptr(), None, [t.data_ptr() for t in gf])
    h.synchronize()
    assert h.backward_route() == FUSED
    assert np.all(gu.cpu().numpy() == 0) and all(np.all(t.cpu().numpy() == 0) for t in gf)      # dL/dQ = 0
    assert cc.same_bits(h.probability(), o.probability())
    h.close()
    # the batch entry point: the same checks
    fr = bc.slam_frames(golden, wl, Ns=(5, 1000))
    b = fr.batch()
    b.set_option(OPT, 1)
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
    assert b.backward_route() == pkg.BACKWARD_NONE
    nb = fr.batch(build=False)
    nb.set_option(OPT, 1)
    assert L.lccrf_batch_inference_backward_features(nb.h, 5, 1.0, vp(G.data_ptr()), vp(gub.data_ptr()), None, goodb, None) == -5
    nb.close()
    b.inference_backward_features_device(5, 1.0, G.data_ptr(), gub.data_ptr(), None, [t.data_ptr() for t in gfb])
    b.synchronize()
    assert b.backward_route() == FUSED
    assert all(np.all(t.cpu().numpy() == 0) for t in gfb)
    b.close()


# ---- the float64 checker ---------------------------------------------------------------------------------------------------------
CHECKED = [(n, T, r) for n, T, r in gset.FEATURE_SETTINGS if n in ("slam:N5", "slam:N1001", "c2") and T == 5]
CHECKED_TIES = [(n, T, r) for n, T, r in gset.TIES if n in ("ties:slam256", "ties:slam2047")]


@pytest.mark.parametrize("name,T,relax", CHECKED, ids=["%s-%d-%r" % s for s in CHECKED])
def test_feature_gradients_match_the_checker(po, wl, golden, name, T, relax):
    """under the bars and the cap of test_feature_gradients_match_the_checker (tests/test_feature_gradients.py), no new bar"""
    s = gset.features(po, wl, golden, name, T, relax)
    h, keep = gs.gpu_handle(s["pb"], s["image"])
    on = _call(h, True, T, relax, s["G"], _dims(s["pb"]))
    h.close()
    assert on[4] == FUSED
    s["ref"].check({"dL/df%d" % k: a for k, a in enumerate(on[2])})
    s["ref_1c"].check({"dL/dU": on[0], "dL/dw": on[1]})


@pytest.mark.parametrize("name,T,relax", CHECKED_TIES, ids=["%s-%d-%r" % s for s in CHECKED_TIES])
def test_feature_gradients_at_exact_lattice_ties(po, wl, golden, name, T, relax):
    """the kernel recomputes the simplex itself (lattice_simplex, as k_corner_to_feature does): frames whose points sit on the build's
    rounding and rank ties, under the bars of the list"""
    s = gset.ties(po, wl, golden, name, T, relax)
    h, keep = gs.gpu_handle(s["pb"], None)
    on = _call(h, True, T, relax, s["G"], _dims(s["pb"]))
    h.close()
    assert on[4] == FUSED
    s["ref"].check({"dL/df%d" % k: a for k, a in enumerate(on[2])})
    s["ref_1c"].check({"dL/dU": on[0], "dL/dw": on[1]})


# ---- the torch layers ---------------------------------------------------------------------------------------------------------------
def test_mean_field_features_keyword(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = wl.slam_problem(1500, seed=6)
    U = torch.from_numpy(cc.raw_unary(pb)).cuda()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((1500, 2)).astype(np.float32)).cuda()
    out, routes = {}, []
    for fused in (False, True):
        u = U.clone().requires_grad_(True)
        w = torch.tensor([float(x) for _, x in pb["kernels"]], dtype=torch.float32, requires_grad=True)
        fs = [torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda().requires_grad_(True) for f, _ in pb["kernels"]]
        q = ag.mean_field_features(u, fs, w, 5, 0.7, route_out=routes, **({"fused_backward": True} if fused else {}))
        q.backward(G)
        torch.cuda.synchronize()
        out[fused] = [u.grad.cpu().numpy(), w.grad.numpy(), q.detach().cpu().numpy()] + [f.grad.cpu().numpy() for f in fs]
    assert routes == [STREAM, FUSED]
    for x, y in zip(out[True], out[False]):
        assert cc.same_bits(x, y)


def test_learned_kernel_crf_keyword(wl):
    """one optimiser step of LearnedKernelCRF(fused_backward=True) gives the bits of the streaming layer's step"""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    p = wl.TUM3
    pb = wl.slam_problem(2000, seed=31)
    fr = pb["frame"]
    raw = [np.stack([fr["obs"], fr["err"]], 1).astype(np.float32), fr["uv"].astype(np.float32)]
    U = torch.from_numpy(cc.raw_unary(pb)).cuda()
    target = torch.from_numpy(np.random.default_rng(4).random((2000, 2)).astype(np.float32)).cuda()
    out = {}
    for fused in (False, True):
        layer = ag.LearnedKernelCRF(raw, [[2.5, 1.0], [30.0]], [p["w1"] / 10, p["w2"] / 10], groups=[None, [[0, 1]]], n_iterations=5,
                                    **({"fused_backward": True} if fused else {}))
        assert layer.backward_route == pkg.BACKWARD_NONE
        opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
        loss = ((layer(U) - target) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        out[fused] = ([x.detach().cpu().numpy() for x in layer.log_sd] + [layer.weights.detach().cpu().numpy()] +
                      [x.grad.cpu().numpy() for x in layer.log_sd], layer.backward_route)
    assert out[False][1] == STREAM and out[True][1] == FUSED
    for x, y in zip(out[True][0], out[False][0]):
        assert cc.same_bits(x, y)

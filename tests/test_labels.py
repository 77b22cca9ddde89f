"""Every label count, term count and feature dimension include/lccrf.h accepts: L = 1 .. LCCRF_MAX_LABELS (64), up to
LCCRF_MAX_KERNELS (8) terms, features of up to LCCRF_MAX_DIMS (8) dimensions.

CPU: the oracle against tests/golden/labels.npz (vectors from the reference build itself, make_golden_labels.py), bit for bit; the
float64 checker's forward on those cases; the closed form of one label; the limits rejected before any device is touched.
GPU: the HIP forward against the fixture and the oracle at every L from 1 to 64 (the streaming engine's softmax rows, its per-point
softmax, the four-label splat / blur chunks and their partial last chunk), its long-row, locality-mode and ragged-batch paths at
L = 9, 33 and 64 with eight terms, the bare filter at every value size, apply(); the backward's five lane groups (1, 2, 4, 8, 16 lanes
per row: L <= 4, <= 8, <= 16, <= 32, <= 64) on both sides of each boundary, with 0, 1 and 8 terms, against the float64 checker; its
determinism at 64 labels; and the torch layers at L = 64, K = 8."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import meanfield_f64 as mf
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
LABELS_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labels.npz")
FILTER_SIZES = (1, 3, 4, 7, 31, 33, 63, 64)
EIGHT = list(range(1, 9))                                   # eight terms, d = 1 .. 8


def _fixture():
    return np.load(LABELS_NPZ)


CASES = [str(c) for c in _fixture()["cases"]]


def _check_fixture_case(c, z, name):
    """lattice internals of every term, the Q trace and the labels of one labels.npz case, bit for bit"""
    p = name + "_"
    for k in range(int(z[p + "K"])):
        kv = c.kernel(k)
        assert kv["V"] == int(z[p + "V%d" % k]), (name, k)
        for a in ("norm", "offset", "bary", "nbr"):
            assert cc.same_bits(kv[a], z[p + "%s%d" % (a, k)]), (name, k, a)
    trace = c.run_trace(int(z["iters"]), relax=float(z["relax"]))
    want = z[p + "trace"]
    for t in range(len(want)):
        assert cc.same_bits(trace[t], want[t]), "%s: Q differs after %d iterations (max %g)" % (
            name, t, np.abs(trace[t] - want[t]).max())
    c.build_map()
    assert np.array_equal(c.map(), z[p + "map"]), name


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_every_label_group_term_count_and_dimension():
    z = _fixture()
    Ls = {int(z[c + "_L"]) for c in CASES}
    assert Ls >= {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 21, 22, 31, 32, 33, 63, 64}
    assert max(int(z[c + "_K"]) for c in CASES) == 8
    dims = {int(z[c + "_feat%d" % k].shape[1]) for c in CASES for k in range(int(z[c + "_K"]))}
    assert dims == set(EIGHT)
    assert any(c + "_label" in z.files for c in CASES) and any(c + "_unary" in z.files for c in CASES)
    ties = [c for c in CASES if c + "_unary" in z.files and int(z[c + "_L"]) >= 2]
    assert all(cc.same_bits(z[c + "_trace"][..., 0], z[c + "_trace"][..., -1]) for c in ties)   # exact ties for the argmax


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_labels_fixture(po, name):
    z = _fixture()
    o = cc.setup(po.OracleCRF, cc.case_problem(z, name))
    _check_fixture_case(o, z, name)
    o.close()


@pytest.mark.parametrize("vs", FILTER_SIZES)
def test_oracle_lattice_filter_reproduces_the_labels_fixture(po, vs):
    z, p = _fixture(), "filter%d_" % vs
    y, V = po.oracle_lattice_filter(z[p + "features"], z[p + "x"])
    assert V == int(z[p + "V"]) and cc.same_bits(y, z[p + "y"])


@pytest.mark.parametrize("name", CASES)
def test_checker_forward_matches_the_labels_fixture(po, name):
    """The float64 checker (tests/meanfield_f64.py) at every iteration of the reference's trace, at the tolerance of
    test_checker_forward_matches_the_oracle: 1e-5, and 5e-5 with several terms on one CRF."""
    import torch
    z = _fixture()
    pb = cc.case_problem(z, name)
    o, lats, U = gs.checker(po, pb)
    tol = 5e-5 if len(pb["kernels"]) > 1 else 1e-5
    trace = z[name + "_trace"]
    for t in range(1, len(trace)):
        q = mf.forward(torch.as_tensor(U), torch.as_tensor(gs.weights(pb)), lats, t, float(z["relax"])).numpy()
        assert np.abs(q - trace[t]).max() <= tol, (name, t, np.abs(q - trace[t]).max())
    o.close()


def test_one_label_is_the_closed_form(po):
    """L = 1: every softmax row is exp(0) / exp(0) -- Q is 1 and the label 0 from the start, whatever the terms."""
    z = _fixture()
    assert np.all(z["L1_trace"] == 1.0) and np.all(z["L1_map"] == 0)
    pb = cc.label_problem(300, 1, EIGHT, seed=4)
    o = cc.setup(po.OracleCRF, pb)
    o.inference_native(5, True, 0.8)
    assert np.all(o.probability() == 1.0) and np.all(o.map() == 0)
    o.close()


def test_limits_are_rejected_before_the_device_is_touched(lib):
    """L = 0 and 65, a ninth term and d = 9: LCCRF_E_INVALID from the handle, the batch descriptor, BatchCRF and the bare filter,
    before any device is looked at (so also where there is none)."""
    h = C.c_void_p()
    for L in (0, 65, -1):
        assert lib.lccrf_create(C.byref(h), 0, 16, L) == -1 and not h.value, L
        with pytest.raises(pkg.LccrfError) as e:
            pkg.DenseCRFHIP(16, L)
        assert e.value.code == -1
    desc = pkg.BatchDesc()
    desc.max_frames, desc.max_points, desc.n_labels, desc.n_kernels = 2, 16, 64, 8
    for k in range(8):
        desc.feat_dims[k], desc.weights[k] = k + 1, 1.0
    for field, value in (("n_labels", 0), ("n_labels", 65), ("n_kernels", 9), ("n_kernels", -1)):
        bad = pkg.BatchDesc.from_buffer_copy(desc)
        setattr(bad, field, value)
        assert lib.lccrf_batch_create(C.byref(h), 0, C.byref(bad)) == -1 and not h.value, (field, value)
    for k, d in ((0, 9), (7, 9), (3, 0)):
        bad = pkg.BatchDesc.from_buffer_copy(desc)
        bad.feat_dims[k] = d
        assert lib.lccrf_batch_create(C.byref(h), 0, C.byref(bad)) == -1 and not h.value, (k, d)
    for L, dims in ((0, [2]), (65, [2]), (64, EIGHT + [3]), (64, [2, 9])):
        with pytest.raises(pkg.LccrfError) as e:
            pkg.BatchCRF(2, 16, L, dims, [1.0] * len(dims))
        assert e.value.code == -1, (L, dims)
    f = np.zeros((16, 9), np.float32)
    x = np.zeros((16, 4), np.float32)
    out = np.zeros_like(x)
    f32p = C.POINTER(C.c_float)
    for d, vs in ((9, 4), (0, 4), (2, 0), (2, 65)):
        assert lib.lccrf_lattice_filter(0, f.ctypes.data_as(f32p), 16, d, x.ctypes.data_as(f32p), vs, out.ctypes.data_as(f32p),
                                        None) == -1, (d, vs)


# ---- GPU: forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_reproduces_the_labels_fixture(name):
    z = _fixture()
    h = cc.setup(pkg.DenseCRFHIP, cc.case_problem(z, name))
    _check_fixture_case(h, z, name)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", range(1, 65))
def test_hip_matches_the_oracle_at_every_label_count(po, L):
    """One generic frame of 1500 points, one 3-D term: raw unaries with exact ties between labels 0 and L - 1, and labels (L >= 2).
    The Q trace and the labels, bit for bit."""
    for label in ((False, True) if L >= 2 else (False,)):
        pb = cc.label_problem(1500, L, [3], seed=L, label=label)
        h, o = cc.setup(pkg.DenseCRFHIP, pb), cc.setup(po.OracleCRF, pb)
        th, to = h.run_trace(3, relax=0.75), o.run_trace(3, relax=0.75)
        for t in range(4):
            assert cc.same_bits(th[t], to[t]), "L=%d label=%s: Q differs after %d iterations (max %g)" % (
                L, label, t, np.abs(th[t] - to[t]).max())
        h.build_map(), o.build_map()
        assert np.array_equal(h.map(), o.map()), (L, label)
        if not label and L >= 2:
            assert np.any(to[3][:, 0] == to[3].max(1)), "no tied row"
        h.close(), o.close()


def _oracle_frames(po, b, probs, sizes, n_iter, relax):
    """every frame of a batch against the oracle on its own points: lattice sizes, Q and labels"""
    Q, M = b.probability(), b.map()
    for f, n in enumerate(sizes):
        if n == 0:
            continue
        pb = probs[f]
        o = cc.setup(po.OracleCRF, pb)
        o.inference_native(n_iter, True, relax)
        assert all(int(b.lattice_sizes(k)[f]) == o.kernel(k)["V"] for k in range(len(pb["kernels"]))), f
        assert cc.same_bits(Q[f, :n], o.probability()), "frame %d (N=%d): Q differs (max %g)" % (
            f, n, np.abs(Q[f, :n] - o.probability()).max())
        assert np.array_equal(M[f, :n], o.map()), f
        o.close()


def _batch_inputs(probs, maxN, L):
    F = len(probs)
    U = np.zeros((F, maxN, L), np.float32)
    feats = [np.zeros((F, maxN, f.shape[1]), np.float32) for f, _ in probs[0]["kernels"]]
    for i, pb in enumerate(probs):
        U[i, :pb["N"]] = pb["unary"]
        for k, (f, _) in enumerate(pb["kernels"]):
            feats[k][i, :pb["N"]] = f
    return U, feats


def _crop(pb, n):
    return dict(pb, N=n, unary=pb["unary"][:n], kernels=[(f[:n], w) for f, w in pb["kernels"]])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [9, 33, 64])
def test_streaming_long_rows_at_large_label_counts(po, L):
    """A term whose points all lie in one lattice cell (3 vertices, rows of N products: k_splat_long) beside one with a giant
    vertex and many shared cells, two ragged frames, the hash and the sorted vertex order: the oracle's bits."""
    N = 6000
    pb = cc.label_problem(N, L, [2, 3], seed=70 + L)
    f0, f1 = pb["kernels"][0][0], pb["kernels"][1][0]
    f0[:] = f0[0]
    f1[: N // 3] = f1[5]
    f1[N // 3: N // 2] = np.round(f1[N // 3: N // 2])
    sizes = [N, N - 211]
    probs = [_crop(pb, n) for n in sizes]
    U, feats = _batch_inputs(probs, N, L)
    for order in (0, 2):
        b = pkg.BatchCRF(2, N, L, [2, 3], [float(w) for _, w in pb["kernels"]])
        b.set_engine(1)
        b.set_option(pkg.OPT_VERTEX_ORDER, order)
        b.set_inputs_host(sizes, feats, unary=U)
        b.build()
        b.inference(3, True, relax=0.75)
        assert int(b.lattice_sizes(0)[0]) <= 3
        _oracle_frames(po, b, probs, sizes, 3, 0.75)
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [9, 33, 64])
def test_locality_mode_at_large_label_counts(po, L):
    """A frame above the locality-mode threshold (internal point order, sorted build) through the object API and a batch, labels as
    input on the handle: the oracle's bits."""
    N = 9000
    pb = cc.label_problem(N, L, [3, 2], seed=90 + L, spread=2.5)
    pl = cc.label_problem(N, L, [3, 2], seed=90 + L, spread=2.5, label=True)
    for p in (pb, pl):
        h, o = cc.setup(pkg.DenseCRFHIP, p), cc.setup(po.OracleCRF, p)
        h.inference(3, True, 0.75)
        o.inference_native(3, True, 0.75)
        assert cc.same_bits(h.probability(), o.probability()) and np.array_equal(h.map(), o.map())
        h.close(), o.close()
    sizes = [N, 1200]
    probs = [pb, _crop(pb, 1200)]
    U, feats = _batch_inputs(probs, N, L)
    b = pkg.BatchCRF(2, N, L, [3, 2], [float(w) for _, w in pb["kernels"]])
    b.set_inputs_host(sizes, feats, unary=U)
    b.build()
    b.inference(3, True, relax=0.75)
    assert b.locality_mode()[0], "the 9000-point frame should be in locality mode"
    _oracle_frames(po, b, probs, sizes, 3, 0.75)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [9, 33, 64])
def test_ragged_batch_with_eight_terms_at_large_label_counts(po, L):
    sizes = [700, 0, 1500, 77, 1201]
    fr = bc.label_frames(L, sizes, seed=300 + L)
    probs = fr.probs
    b = fr.batch()
    b.inference(3, True, relax=0.75)
    _oracle_frames(po, b, probs, sizes, 3, 0.75)
    b.run(3, True, 0.75)
    _oracle_frames(po, b, probs, sizes, 3, 0.75)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vs", FILTER_SIZES)
def test_hip_lattice_filter_reproduces_the_labels_fixture(vs):
    z, p = _fixture(), "filter%d_" % vs
    y, V = pkg.lattice_filter(z[p + "features"], z[p + "x"])
    assert V == int(z[p + "V"]) and cc.same_bits(y, z[p + "y"])


@pytest.mark.gpu
def test_hip_lattice_filter_at_every_value_size(po):
    rng = np.random.default_rng(12)
    f = rng.normal(0, 2.5, (700, 3)).astype(np.float32)
    f[rng.random(700) < 0.3] = np.float32(0.5)
    for vs in range(1, 65):
        x = rng.normal(0, 1, (700, vs)).astype(np.float32)
        (yh, Vh), (yo, Vo) = pkg.lattice_filter(f, x), po.oracle_lattice_filter(f, x)
        assert Vh == Vo and cc.same_bits(yh, yo), "value_size %d (max %g)" % (vs, np.abs(yh - yo).max())


@pytest.mark.gpu
def test_apply_at_64_labels_and_eight_terms(po):
    pb = cc.label_problem(1300, 64, EIGHT, seed=13)
    h, o = cc.setup(pkg.DenseCRFHIP, pb), cc.setup(po.OracleCRF, pb)
    rng = np.random.default_rng(14)
    for k in range(8):
        out = rng.normal(0, 1, (1300, 64)).astype(np.float32)
        x = rng.random((1300, 64)).astype(np.float32)
        assert cc.same_bits(h.apply(k, out, x), o.apply(k, out, x)), k
    h.close(), o.close()


@pytest.mark.gpu
def test_ninth_term_and_ninth_dimension_are_rejected_and_the_handle_stays_usable(po):
    pb = cc.label_problem(500, 64, EIGHT, seed=15)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    with pytest.raises(pkg.LccrfError) as e:
        h.add_pairwise(pb["kernels"][0][0], 1.0)
    assert e.value.code == -6                                  # LCCRF_E_CAPACITY
    h2 = pkg.DenseCRFHIP(500, 64)
    with pytest.raises(pkg.LccrfError) as e:
        h2.add_pairwise(np.zeros((500, 9), np.float32), 1.0)
    assert e.value.code == -1
    h2.close()
    o = cc.setup(po.OracleCRF, pb)
    h.inference(3, True, 0.75)
    o.inference_native(3, True, 0.75)
    assert cc.same_bits(h.probability(), o.probability()) and np.array_equal(h.map(), o.map())
    h.close(), o.close()


# ---- GPU: backward --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", gset.LANE_LABELS)
@pytest.mark.parametrize("K", gset.LANE_TERMS)
@pytest.mark.parametrize("T", gset.T_SHORT)
@pytest.mark.parametrize("relax", gset.RELAX_SET)
def test_gradients_match_the_checker_in_every_lane_group(po, L, K, T, relax):
    """lccrf_inference_backward at the edges of its lane groups (bwd_lanes: 1, 2, 4, 8, 16 lanes per row), one and eight terms, at
    the bar of test_gradients_match_the_checker.  The weights of label_problem keep the rows unsaturated, so the gradients compared
    are far above that test's floor."""
    s = gset.lane_group(po, L, K, T, relax)
    h = cc.setup(pkg.DenseCRFHIP, s["pb"])
    gu, gw = gs.backward(h, T, relax, s["G"], K)
    h.close()
    s["ref"].check({"dL/dU": gu, "dL/dw": gw})
    if T == 0:
        assert np.all(gw == 0)
    assert np.linalg.norm(s["ref"].ref["dL/dU"]) > 1e-3 * np.linalg.norm(s["G"])


@pytest.mark.gpu
@pytest.mark.parametrize("L", gset.TERMLESS_LABELS)
def test_gradients_without_terms_in_every_lane_group(po, L):
    h = None
    for T in gset.T_SHORT:
        for relax in gset.RELAX_SET:
            s = gset.termless(L, T, relax)
            h = h or cc.setup(pkg.DenseCRFHIP, s["pb"])
            gu, _ = gs.backward(h, T, relax, s["G"], 0)
            s["ref"].check({"dL/dU": gu})
    h.close()


_k8_frames = gset.k8_frames


@pytest.mark.gpu
@pytest.mark.parametrize("L", gset.K8_BATCH_LABELS)
def test_batch_gradients_with_eight_terms_match_the_checker(po, L):
    fr = _k8_frames(L)
    b = fr.batch()
    G = fr.grad_prob(L)
    for T, relax in gset.K8_BATCH_SETTINGS:
        gu, gw = gs.batch_backward(b, T, relax, G, fr.K)
        for f, n in enumerate(fr.N):
            if n == 0:
                assert np.all(gu[f] == 0) and np.all(gw[f] == 0)
                continue
            gset.batch_frame(po, fr, G, f, T, relax, "frame %d L=%d" % (f, L))["ref"].check({"dL/dU": gu[f, :n], "dL/dw": gw[f]})
    b.close()


@pytest.mark.gpu
def test_torch_layers_at_64_labels_and_eight_terms_give_the_bits_of_the_c_abi():
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    T, relax = 5, 0.7
    pb = cc.label_problem(900, 64, EIGHT, seed=800)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    G = np.random.default_rng(8).standard_normal((900, 64)).astype(np.float32)
    ref_u, ref_w = gs.backward(h, T, relax, G, 8)
    h.inference(T, False, relax)
    ref_q = h.probability()
    u = torch.from_numpy(h.unary()).cuda().requires_grad_(True)
    w = torch.tensor(gs.weights(pb).astype(np.float32), requires_grad=True)
    q = ag.mean_field(h, u, w, T, relax)
    q.backward(torch.from_numpy(G).cuda())
    torch.cuda.synchronize()
    assert cc.same_bits(q.detach().cpu().numpy(), ref_q)
    assert cc.same_bits(u.grad.cpu().numpy(), ref_u) and cc.same_bits(w.grad.numpy(), ref_w.astype(np.float32))
    h.close()
    # the batched layer over ragged frames
    fr = _k8_frames(64)
    ref = fr.batch()
    ref.inference(T, False, relax)
    q_ref = ref.probability()
    Gb = np.nan_to_num(fr.grad_prob(9), nan=0.0)
    bu, bw = gs.batch_backward(ref, T, relax, Gb, 8)
    ref.close()
    b = fr.batch()
    u = torch.from_numpy(fr.U).cuda().requires_grad_(True)
    w = torch.tensor(fr.w, requires_grad=True)
    q = ag.mean_field_batch(b, u, w, T, relax)
    q.backward(torch.from_numpy(Gb).cuda())
    torch.cuda.synchronize()
    qn = q.detach().cpu().numpy()
    assert all(cc.same_bits(qn[f, :n], q_ref[f, :n]) and np.all(qn[f, n:] == 0) for f, n in enumerate(fr.N))
    assert cc.same_bits(u.grad.cpu().numpy(), bu)
    want = bw.astype(np.float64).sum(0)
    assert np.all(np.abs(w.grad.numpy() - want) <= 1e-6 * np.abs(want)), (w.grad, want)
    b.close()

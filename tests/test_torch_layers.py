"""The contract of the torch layer (lc-crf-slam_amd/autograd.py) and of the binding it drives (DenseCRFHIP, BatchCRF): what its six
functions and six modules refuse and in which words, where a gradient lands, which features get one, that a backward runs under the
model of ITS forward, and that Q and every gradient have the bits of the binding's setters, inference and backward entry point called
by hand.  notes/torch_layers.md says which entry point stands behind which function.

Shapes are the smallest at which these paths can go wrong: 64 points, L = 2 and 3, K = 0, 1 and 2 two-dimensional terms, T = 2,
relax 0.7; batches of three frames of (64, 17, 0) points at max_points 64.  Features and unaries are wl.slam_problem's."""
import importlib

import numpy as np
import pytest
import torch

import crf_cases as cc

pkg = importlib.import_module("lc-crf-slam_amd")
ag = importlib.import_module("lc-crf-slam_amd.autograd")
F32 = np.float32
N, T, RELAX = 64, 2, 0.7
COUNTS = (64, 17, 0)
# function -> (what it is bound to, does it take `compat`)
KINDS = {"mean_field": ("handle", False), "mean_field_compat": ("handle", True),
         "mean_field_batch": ("batch", False), "mean_field_batch_compat": ("batch", True),
         "mean_field_features": ("own", False), "mean_field_learned": ("own", True)}
HANDLE_KINDS, BATCH_KINDS, OWN_KINDS = ([k for k, (b, _) in KINDS.items() if b == bound] for bound in ("handle", "batch", "own"))
SECOND = "%s: backward a second time (the handle is closed by the first)"
DEVICE_COUNTS = "the batch's point counts are on the device only (bind_inputs_device): set its inputs from the host"


class Case:
    """inputs of one handle (counts None: [N, .] arrays) or of one batch ([F, N, .] arrays, rows beyond a frame's points 0), and dL/dQ"""

    def __init__(self, wl, L, K, counts=None):
        self.L, self.K, self.counts = L, K, counts
        ns = [N] if counts is None else list(counts)
        U, feats = np.zeros((len(ns), N, L), F32), [np.zeros((len(ns), N, 2), F32) for _ in range(K)]
        for f, n in enumerate(ns):
            if n:
                pb, third = wl.slam_problem(n, seed=300 + f), wl.slam_problem(n, seed=400 + f)
                u = cc.raw_unary(pb)
                U[f, :n] = u if L == 2 else np.concatenate([u, cc.raw_unary(third)[:, :1]], 1)
                for k in range(K):
                    feats[k][f, :n] = pb["kernels"][k][0]
        self.U, self.feats = (U[0], [x[0] for x in feats]) if counts is None else (U, feats)
        self.G = np.random.default_rng(500 + 10 * L + K).standard_normal(self.U.shape).astype(F32)      # (finite in every row)


_cases = {}


def _case(wl, L, K, counts=None):
    key = (L, K, counts)
    if key not in _cases:
        _cases[key] = Case(wl, L, K, counts)
    return _cases[key]


def _model(c, which):
    """(weights [K], matrices [K, L, L]) A (which = 0) or B (1): neither the weights the targets are created with nor identities"""
    m = np.eye(c.L, dtype=F32) + np.random.default_rng(600 + which).standard_normal((2, c.L, c.L)).astype(F32) * F32(0.25)
    return [[3.0, 5.0], [1.5, 7.0]][which][:c.K], np.ascontiguousarray(m[:c.K], F32)


def _handle(c):
    h = pkg.DenseCRFHIP(N, c.L)
    for f in c.feats:
        h.add_pairwise(f, 1.0)
    return h


def _batch(c):
    b = pkg.BatchCRF(len(c.counts), N, c.L, [2] * c.K, [1.0] * c.K)
    b.set_inputs_host(c.counts, c.feats, unary=np.zeros_like(c.U))
    b.build()
    return b


def _target(kind, c):
    return {"handle": _handle, "batch": _batch, "own": lambda c: None}[KINDS[kind][0]](c)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _same(a, b):
    """two results (dicts of tensors, arrays, None or lists of them) with the same bits"""
    def one(x, y):
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(one(p, q) for p, q in zip(x, y))
        if x is None or y is None:
            return x is None and y is None
        return cc.same_bits(_np(x) if isinstance(x, torch.Tensor) else x, _np(y) if isinstance(y, torch.Tensor) else y)
    return a.keys() == b.keys() and all(one(a[k], b[k]) for k in a)


class Run:
    """one forward of a layer function on leaf tensors of its own"""

    def __init__(self, kind, c, model, target=None, w_dev="cpu", m_dev="cpu", f_grad=(True, True)):
        bound, compat = KINDS[kind]
        w, m = model
        self.u = _cuda(c.U).requires_grad_(True)
        self.w = torch.tensor(w, dtype=torch.float32, device=w_dev).requires_grad_(True)
        self.m = torch.tensor(m, device=m_dev).requires_grad_(True) if compat else None
        self.fs = [_cuda(f).requires_grad_(need) for f, need in zip(c.feats, f_grad)] if bound == "own" else []
        args = [self.u] + ([self.fs] if bound == "own" else []) + [self.w] + ([self.m] if compat else [])
        self.q = getattr(ag, kind)(*(([] if bound == "own" else [target]) + args), T, RELAX)

    def backward(self, G, retain=False):
        """the leaves' gradients (tensors, where they landed) of one backward from dL/dQ = G"""
        for t in [self.u, self.w, self.m] + self.fs:
            if t is not None:
                t.grad = None
        self.q.backward(_cuda(G), retain_graph=retain)
        torch.cuda.synchronize()
        out = dict(gu=self.u.grad, gw=self.w.grad, gf=[f.grad for f in self.fs])
        if self.m is not None:
            out["gm"] = self.m.grad
        return out


def _layer(kind, c, model, **kw):
    """(Q, gradients) of one forward and backward on a fresh target"""
    t = _target(kind, c)
    r = Run(kind, c, model, t, **kw)
    out = r.backward(c.G)
    if t is not None:
        t.close()
    return r.q.detach(), out


def _arm(t, w, m):
    for k, x in enumerate(w):
        t.set_pairwise_weight(k, x)
    for k in range(0 if m is None else len(m)):
        t.set_pairwise_compatibility(k, m[k])


def _by_hand(kind, c, model):
    """(Q, gradients) of the same setters, inference() and the backward entry point of `kind`, called on the binding directly"""
    bound, compat = KINDS[kind]
    w, m = model[0], model[1] if compat else None
    K, L = c.K, c.L
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    u, g, gu = _cuda(c.U), _cuda(c.G), nan(*c.U.shape)
    fs = [_cuda(f) for f in c.feats]
    gf = [nan(N, 2) for _ in fs]
    out = dict(gf=[])
    if bound == "batch":
        F = len(c.counts)
        per_frame, sums = nan(F, K), nan(K * (1 + L * L))
        t = _batch(c)
        torch.cuda.synchronize()
        _arm(t, w, m)
        t.set_unary_device(u.data_ptr())
        t.inference(T, False, RELAX)
        t.synchronize()
        q = t.probability()
        for f, n in enumerate(c.counts):
            q[f, n:] = 0
        if compat:                                                # section 2h: the call's own ordered sums
            t.inference_backward_all_device(T, RELAX, g.data_ptr(), gu.data_ptr(), d_grad_model=sums.data_ptr())
            t.synchronize()
            out.update(gw=sums[:K], gm=sums[K:].reshape(K, L, L))
        else:                                                     # section 2c: torch's sum of the [F, K] output
            t.inference_backward_device(T, RELAX, g.data_ptr(), gu.data_ptr(), per_frame.data_ptr())
            t.synchronize()
            out.update(gw=torch.sum(per_frame[:, :K], 0))
    else:
        gw, gm = nan(max(K, 1)), nan(max(K, 1), L, L)
        t = _handle(c) if bound == "handle" else pkg.DenseCRFHIP(N, L)
        torch.cuda.synchronize()
        if bound == "handle":
            _arm(t, w, m)
            t.set_unary_device(u.data_ptr())
        else:
            t.set_unary_device(u.data_ptr())
            for f, x in zip(fs, w):
                t.add_pairwise_device(f.data_ptr(), 2, x)
            _arm(t, [], m)
        t.inference(T, False, RELAX)
        t.synchronize()
        q = t.probability()
        args = (T, RELAX, g.data_ptr(), gu.data_ptr(), gw.data_ptr() if K else None)
        gf_ptr = [x.data_ptr() for x in gf]
        if kind == "mean_field":
            t.inference_backward_device(*args)
        elif kind == "mean_field_compat":
            t.inference_backward_compat_device(*args, gm.data_ptr())
        elif kind == "mean_field_features":
            t.inference_backward_features_device(*args, gf_ptr)
        else:
            t.inference_backward_all_device(*args, gf_ptr, gm.data_ptr())
        t.synchronize()
        out.update(gw=gw[:K], gf=gf if bound == "own" else [])
        if compat:
            out["gm"] = gm[:K]
    t.close()
    out["gu"] = gu
    return q, out


SHAPES = [(kind, L, K) for kind in KINDS for L in (2, 3) for K in ((1, 2) if KINDS[kind][0] == "batch" else (0, 1, 2))]


# ---- the bits of the binding called by hand ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,L,K", SHAPES)
def test_q_and_every_gradient_have_the_bits_of_the_binding_called_by_hand(wl, kind, L, K):
    c = _case(wl, L, K, COUNTS if kind in BATCH_KINDS else None)
    model = _model(c, 0)
    q, got = _layer(kind, c, model)
    q_want, want = _by_hand(kind, c, model)
    assert cc.same_bits(_np(q), q_want)
    assert _same(got, want), (got, want)
    assert tuple(got["gw"].shape) == (K,) and ("gm" not in got or tuple(got["gm"].shape) == (K, L, L))      # K = 0: empty, not absent
    assert all(np.isfinite(_np(x)).all() for x in [q, got["gu"], got["gw"]] + got["gf"])
    if kind in BATCH_KINDS:                                       # rows at and beyond a frame's count, the empty frame included
        for f, n in enumerate(COUNTS):
            assert float(q[f, n:].abs().sum()) == 0.0 and float(got["gu"][f, n:].abs().sum()) == 0.0, f
        assert float(q[0].abs().min()) > 0.0


# ---- where results land ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_model_gradients_land_where_the_model_came_from(wl, kind):
    c = _case(wl, 2, 2, COUNTS if kind in BATCH_KINDS else None)
    model = _model(c, 0)
    _, ref = _layer(kind, c, model)
    for w_dev, m_dev in (("cpu", "cuda"), ("cuda", "cpu")):
        _, got = _layer(kind, c, model, w_dev=w_dev, m_dev=m_dev)
        assert got["gw"].device.type == w_dev and got["gu"].is_cuda
        assert "gm" not in got or got["gm"].device.type == m_dev
        assert _same(got, ref)


# ---- which features get a gradient -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", OWN_KINDS)
def test_only_the_features_that_ask_get_a_gradient(wl, kind):
    c = _case(wl, 3, 2)
    model = _model(c, 0)
    _, both = _layer(kind, c, model)
    _, second = _layer(kind, c, model, f_grad=(False, True))
    assert second["gf"][0] is None and both["gf"][0] is not None
    assert cc.same_bits(_np(second["gf"][1]), _np(both["gf"][1]))
    assert _same(dict(second, gf=[]), dict(both, gf=[]))


# ---- re-arming ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", HANDLE_KINDS + BATCH_KINDS)
def test_a_backward_runs_under_the_model_of_its_own_forward(wl, kind):
    c = _case(wl, 3, 2, COUNTS if kind in BATCH_KINDS else None)
    a, b = _model(c, 0), _model(c, 1)
    q_alone, alone = _layer(kind, c, a)
    t = _target(kind, c)
    first = Run(kind, c, a, t)
    other = Run(kind, c, b, t)
    assert cc.same_bits(_np(first.q), _np(q_alone)) and not cc.same_bits(_np(other.q), _np(q_alone))
    got = first.backward(c.G, retain=True)
    assert _same(got, alone), (got, alone)
    assert not _same(other.backward(c.G), alone)                  # (the other model's gradients are others)
    again = first.backward(c.G, retain=True)                      # ... and a second time through the same graph
    assert _same(again, alone)
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OWN_KINDS)
def test_an_own_handle_takes_one_backward(wl, kind):
    c = _case(wl, 2, 2)
    r = Run(kind, c, _model(c, 0))
    r.backward(c.G, retain=True)
    with pytest.raises(RuntimeError) as e:
        r.backward(c.G)
    assert str(e.value) == SECOND % kind


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(text, f, *args, exc=ValueError, **kw):
    with pytest.raises(exc) as e:
        f(*args, **kw)
    assert str(e.value) == text, (str(e.value), text)


@pytest.mark.gpu
def test_the_functions_refuse_bad_inputs_in_their_own_words(wl):
    c, cb = _case(wl, 2, 2), _case(wl, 2, 2, COUNTS)
    h, b = _handle(c), _batch(cb)
    u, ub, fs = _cuda(c.U), _cuda(cb.U), [_cuda(f) for f in c.feats]
    w, m = torch.tensor([3.0, 5.0]), torch.eye(2).repeat(2, 1, 1)
    call = {"mean_field": lambda u_, w_, m_, f_, t_: ag.mean_field(h, u_, w_, t_, RELAX),
            "mean_field_compat": lambda u_, w_, m_, f_, t_: ag.mean_field_compat(h, u_, w_, m_, t_, RELAX),
            "mean_field_batch": lambda u_, w_, m_, f_, t_: ag.mean_field_batch(b, u_, w_, t_, RELAX),
            "mean_field_batch_compat": lambda u_, w_, m_, f_, t_: ag.mean_field_batch_compat(b, u_, w_, m_, t_, RELAX),
            "mean_field_features": lambda u_, w_, m_, f_, t_: ag.mean_field_features(u_, f_, w_, t_, RELAX),
            "mean_field_learned": lambda u_, w_, m_, f_, t_: ag.mean_field_learned(u_, f_, w_, m_, t_, RELAX)}
    for kind, (bound, compat) in KINDS.items():
        good = ub if bound == "batch" else u
        shape = {"handle": "64, 2", "batch": "3, 64, 2", "own": "N, L"}[bound]
        for bad in (good.cpu(), good.double(), good[None] if bound == "own" else good[:-1]):
            _refused("unary must be a float32 GPU tensor of shape [%s]" % shape, call[kind], bad, w, m, fs, T)
        for bad in (w.double(), torch.ones(3), torch.ones(2, 1)):
            _refused("weights must be a float32 tensor of shape [2]", call[kind], good, bad, m, fs, T)
        if compat:
            for bad in (m.double(), torch.eye(3).repeat(2, 1, 1), m[:1]):
                _refused("compat must be a float32 tensor of shape [2, 2, 2]", call[kind], good, w, bad, fs, T)
        if bound == "own":
            for bad in (fs[0].cpu(), fs[0].double(), fs[0][:-1], fs[0].reshape(-1)):
                _refused("every feature array must be a float32 GPU tensor of shape [64, d_k]", call[kind], good, w, m, [fs[1], bad], T)
        _refused("n_iterations must be >= 0", call[kind], good, w, m, fs, -1)
    # a batch whose point counts are on the device only
    bd = pkg.BatchCRF(3, N, 2, [2, 2], [1.0, 1.0])
    counts, fb = torch.tensor(COUNTS, dtype=torch.int32, device="cuda"), [_cuda(f) for f in cb.feats]
    torch.cuda.synchronize()
    bd.bind_inputs_device(3, counts.data_ptr(), [f.data_ptr() for f in fb], ub.data_ptr())
    _refused(DEVICE_COUNTS, ag.mean_field_batch, bd, ub, w, T, RELAX)
    _refused(DEVICE_COUNTS, ag.mean_field_batch_compat, bd, ub, w, m, T, RELAX)
    bd.close()
    # required addresses of the batch's calls: None is no address
    with pytest.raises(TypeError):
        b.set_unary_device(None)
    with pytest.raises(TypeError):
        b.inference_backward_device(T, RELAX, d_grad_prob=None, d_grad_unary=ub.data_ptr())
    # ... and both targets still run
    assert _same(Run("mean_field", c, _model(c, 0), h).backward(c.G), _layer("mean_field", c, _model(c, 0))[1])
    assert _same(Run("mean_field_batch", cb, _model(cb, 0), b).backward(cb.G), _layer("mean_field_batch", cb, _model(cb, 0))[1])
    h.close()
    b.close()


@pytest.mark.gpu
def test_the_modules_refuse_bad_models_in_their_own_words(wl):
    c, cb = _case(wl, 2, 2), _case(wl, 2, 2, COUNTS)
    for cls in (ag.MeanFieldCRF, ag.CompatMeanFieldCRF):
        _refused("one weight per feature array", cls, N, 2, c.feats, [1.0])
    for cls in (ag.BatchMeanFieldCRF, ag.BatchCompatMeanFieldCRF):
        _refused("one weight per feature array", cls, COUNTS, cb.feats, [1.0])
    for cls in (ag.LearnedKernelCRF, ag.LearnedCRF):
        _refused("one list of standard deviations and one weight per feature array", cls, c.feats, [[1.0, 1.0]] * 2, [1.0])
        _refused("one list of standard deviations and one weight per feature array", cls, c.feats, [[1.0, 1.0]], [1.0, 1.0])
        for groups in ([[0], [0]], [[0]], [[0, 1], [1]]):
            _refused("the groups of a term must partition its 2 columns", cls, c.feats[:1], [1.0], [1.0], groups=[groups])


# ---- the modules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_module_is_its_function_over_parameters(wl, kind):
    """every module builds its target from the features, holds float32 CPU parameters -- the weights it was given, identities -- and
    its forward is the function's on them"""
    L = 2
    c = _case(wl, L, 2, COUNTS if kind in BATCH_KINDS else None)
    w, m = _model(c, 0)
    SYM = pkg.NORMALIZE_SYMMETRIC
    layer = {"mean_field": lambda: ag.MeanFieldCRF(N, L, c.feats, w, T, RELAX, normalization=[SYM, pkg.NORMALIZE_AFTER]),
             "mean_field_compat": lambda: ag.CompatMeanFieldCRF(N, L, [_cuda(f) for f in c.feats], w, T, RELAX, normalization=SYM),
             "mean_field_batch": lambda: ag.BatchMeanFieldCRF(COUNTS, c.feats, w, T, RELAX, n_labels=L),
             "mean_field_batch_compat": lambda: ag.BatchCompatMeanFieldCRF(COUNTS, [_cuda(f) for f in c.feats], w, T, RELAX, n_labels=L,
                                                                           normalization=[SYM, pkg.NORMALIZE_AFTER]),
             "mean_field_features": lambda: ag.LearnedKernelCRF(c.feats, [[1.0, 1.0]] * 2, w, n_iterations=T, relax=RELAX),
             "mean_field_learned": lambda: ag.LearnedCRF(c.feats, [[1.0, 1.0]] * 2, w, n_labels=L, n_iterations=T, relax=RELAX)}[kind]()
    bound, compat = KINDS[kind]
    assert layer.weights.dtype == torch.float32 and not layer.weights.is_cuda and layer.weights.tolist() == w
    assert not compat or torch.equal(layer.compat.detach(), torch.eye(L).repeat(2, 1, 1))
    want_modes = {"mean_field": [SYM, 0], "mean_field_compat": [SYM, SYM], "mean_field_batch": [0, 0], "mean_field_batch_compat": [SYM, 0]}
    if bound == "handle":
        assert [layer.crf.get_normalization(k) for k in range(2)] == want_modes[kind] and (layer.crf.N, layer.crf.L) == (N, L)
    if bound == "batch":
        t = layer.batch
        assert [t.normalization(k) for k in range(2)] == want_modes[kind]
        assert (t.n_frames, t.maxN, t.L, t.dims) == (3, N, L, [2, 2]) and tuple(t.n_points) == COUNTS
    if compat:
        layer.compat.data.copy_(torch.from_numpy(m))
    u = _cuda(c.U).requires_grad_(True)
    q = layer(u)
    q.backward(_cuda(c.G))
    torch.cuda.synchronize()
    got = dict(gu=u.grad, gw=layer.weights.grad, gm=layer.compat.grad if compat else None)
    # the function on a target made by hand under the same modes (exp(-log(1)) = 1: the learnt kernels see the features themselves)
    t = _target(kind, c)
    if t is not None:
        for k, mode in enumerate(want_modes[kind]):
            t.set_normalization(k, mode)
    r = Run(kind, c, (w, m), t)
    ref = r.backward(c.G)
    want = dict(gu=ref["gu"], gw=ref["gw"], gm=ref.get("gm"))
    assert cc.same_bits(_np(q), _np(r.q)) and _same(got, want), (got, want)
    if t is not None:
        t.close()
    if bound != "own":
        layer.close()

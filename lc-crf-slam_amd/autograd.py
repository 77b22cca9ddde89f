"""torch autograd through DenseCRF::inference on the HIP path (include/lccrf.h sections 1c - 1g, 1m, 2c, 2i - 2l).

    Q = mean_field(crf, unary, weights, n_iterations=5, relax=1.0)
    Q.backward(g)      # -> unary.grad = dL/dU, weights.grad = dL/dw

    Q = mean_field_batch(batch, unary, weights, n_iterations=5, relax=1.0)     # every frame of a BatchCRF at once
    Q.backward(g)      # -> unary.grad [F, max_points, L], weights.grad = sum over the frames of dL/dw

    Q = mean_field_batch_compat(batch, unary, weights, compat, n_iterations=5, relax=1.0)    # ... with a [K, L, L] compatibility
    Q.backward(g)      # -> also compat.grad; both sums over the frames come from the batch's own call (section 2h)

    Q, t = mean_field_converged(crf, unary, weights, max_iterations=12)         # "until converged, at most 12" (section 1h)
    Q.backward(g)      # -> the gradients at the reported count t (section 1h's recipe)

    Q, t = mean_field_batch_converged(batch, unary, weights, max_iterations=12)   # every frame stops on its own; t [F] int32
    Q.backward(g)      # -> every frame differentiated at ITS count, in one call (section 2j)

    Q, t = mean_field_batch_compat_converged(batch, unary, weights, compat, max_iterations=12)   # ... under a learnt model
    Q.backward(g)      # -> also compat.grad; the sums over the frames at every frame's own count (section 2k)

    Q = mean_field_batch_features(batch, n_points, unary, [f_0, ..], weights, n_iterations=5)   # a batch, the features inputs too
    Q.backward(g)      # -> also f_k.grad [F, max_points, d_k] (sections 2d / 2i); the lattices are built by the forward

    Q, t = mean_field_batch_features_converged(batch, n_points, unary, [f_0, ..], weights, max_iterations=12)   # ... under the stop rule
    Q.backward(g)      # -> every frame at ITS count, dL/d features included (section 2l); BatchLearnedKernelCRF fits bandwidths with both

    Q = mean_field_features(unary, [f_0, f_1, ..], weights, n_iterations=5, relax=1.0)        # the features are inputs too
    Q.backward(g)      # -> also f_k.grad = dL/d features [N, d_k] (section 1d); LearnedKernelCRF fits kernel bandwidths with it

    Q = mean_field_compat(crf, unary, weights, compat, n_iterations=5, relax=1.0)             # a [K, L, L] label compatibility
    Q.backward(g)      # -> also compat.grad = dL/dmu (section 1e); CompatMeanFieldCRF learns it, starting from the Potts model

    Q = mean_field_learned(unary, [f_0, f_1, ..], weights, compat, n_iterations=5, relax=1.0)   # features and matrices together
    Q.backward(g)      # -> unary.grad, weights.grad, f_k.grad and compat.grad from one sweep (section 1f); LearnedCRF learns both

    Q = mean_field_features_modes(unary, [f_0, ..], weights, NORMALIZE_SYMMETRIC, n_iterations=5)   # ... under a normalisation mode
    Q.backward(g)      # -> f_k.grad through the norm's factors too (section 1m); mean_field_learned_modes: with matrices

`crf` is a DenseCRFHIP whose pairwise terms are already added (their features fix the lattices; only the weights are
inputs here).  Forward: lccrf_set_pairwise_weight + lccrf_set_unary_device + lccrf_inference.  Backward:
lccrf_inference_backward, which replays the forward itself, so nothing but the inputs is kept between the two.

Three autograd Functions stand behind them all: one bound to a caller's handle, one to a caller's batch, one to a handle of its own
with the features as inputs; each takes `compat` or None (Potts terms), and the first two a stop rule or None (a fixed count).  notes/torch_layers.md has the entry point each one calls.

Streams (the pattern of section 1b): on entry the handle's stream waits for torch's current stream (the inputs and the
incoming gradient are produced there); on exit torch's current stream waits for the handle's stream.  inference()
results are complete behind lccrf_synchronize, so the forward synchronises the handle before it copies Q out.  The batch
layer follows the same pattern on the batch's own stream (lccrf_batch_inference leaves nothing to settle).
"""
import contextlib
import importlib

import numpy as np
import torch

_pkg = importlib.import_module("lc-crf-slam_amd")


def _device_view(ptr, shape, device, typestr="<f4"):
    """A tensor over handle-owned device memory (no copy)."""
    class _View:
        __cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)
    return torch.as_tensor(_View(), device=device)


def _check_unary_weights(unary, shape, weights, K):
    """unary: float32, on the GPU, of `shape` (None: any [N, L]); weights: float32 [K]"""
    shape_ok = unary.dim() == 2 if shape is None else tuple(unary.shape) == tuple(shape)
    if not unary.is_cuda or unary.dtype != torch.float32 or not shape_ok:
        wanted = "N, L" if shape is None else ", ".join("%d" % n for n in shape)
        raise ValueError("unary must be a float32 GPU tensor of shape [%s]" % wanted)
    if weights.dtype != torch.float32 or tuple(weights.shape) != (K,):
        raise ValueError("weights must be a float32 tensor of shape [%d]" % K)


def _check_compat_iterations(compat, K, L, n_iterations):
    """compat: None (Potts terms) or float32 [K, L, L]"""
    if compat is not None and (compat.dtype != torch.float32 or tuple(compat.shape) != (K, L, L)):
        raise ValueError("compat must be a float32 tensor of shape [%d, %d, %d]" % (K, L, L))
    if n_iterations < 0:
        raise ValueError("n_iterations must be >= 0")


@contextlib.contextmanager
def _on_stream(raw_stream, device):
    """The stream hand-off around calls on a handle's (or batch's) stream: it waits for torch's current stream on entry, and
    torch's current stream waits for it on exit.  Yields (the stream as a torch stream, torch's current stream)."""
    cur = torch.cuda.current_stream(device)
    ext = torch.cuda.ExternalStream(raw_stream, device=device)
    ext.wait_stream(cur)
    yield ext, cur
    cur.wait_stream(ext)


def _clone_q(ptr, shape, device, ext, cur):
    """Q out of the handle's own buffer, copied on the handle's stream `ext` (inside _on_stream)"""
    with torch.cuda.stream(ext):
        q = _device_view(ptr, shape, device).clone()
    q.record_stream(cur)
    return q


def _forward_q(crf, u, n_iterations, relax, ext, cur):
    """run inference on the handle (its unaries `u` and terms are set), clone Q out (inside _on_stream)"""
    crf.inference(int(n_iterations), False, float(relax))
    crf.synchronize()                                         # the completion rule of inference() results
    return _clone_q(crf.device_buffers()["current"], tuple(u.shape), u.device, ext, cur)


def _check_stop(stop, compat, batch=False):
    """stop: None (a fixed count) or (criterion, tol) of "until converged, at most n_iterations" -- on a handle for Potts terms only; a
    batch takes matrices too (include/lccrf.h section 2k)"""
    if stop is not None and compat is not None and not batch:
        raise ValueError("the converged handle layer takes Potts terms only (include/lccrf.h section 1h)")


def _model(weights, compat):
    """what a Function keeps of a forward's model: detached clones (never the caller's live parameters); compat may be None"""
    return weights.detach().clone(), None if compat is None else compat.detach().clone().contiguous()


def _set_matrices(crf, compat):
    """the label-compatibility matrices of a forward (None: none), uploaded on the handle's or batch's stream (inside _on_stream)"""
    if compat is not None:
        for k, m in enumerate(compat.detach().cpu().numpy()):
            crf.set_pairwise_compatibility(k, m)


def _arm(crf, weights, compat):
    """the term weights and matrices of a forward, set on the handle or batch (inside _on_stream)"""
    for k, w in enumerate(weights.tolist()):
        crf.set_pairwise_weight(k, w)
    _set_matrices(crf, compat)


def _remember(ctx, target, n_iterations, relax, weights, compat):
    ctx.target, ctx.n_iterations, ctx.relax = target, int(n_iterations), float(relax)
    ctx.weights_device, ctx.compat_device = weights.device, None if compat is None else compat.device


def _grad_buffers(K, L, device, compat):
    """(dL/dw buffer [max(K, 1)], the address to pass: NULL for K = 0, dL/dmu buffer [max(K, 1), L, L] or None without matrices)"""
    grad_w = torch.empty(max(K, 1), dtype=torch.float32, device=device)
    grad_m = torch.zeros((max(K, 1), L, L), dtype=torch.float32, device=device) if compat else None
    return grad_w, (grad_w.data_ptr() if K else None), grad_m


def _model_grads(ctx, grad_w, grad_m, K):
    """(dL/dw [K], dL/dmu [K, L, L] or None) of a handle from its buffers, each on the device its input came from"""
    if K == 0:
        grad_w = torch.zeros(0, dtype=torch.float32, device=grad_w.device)
    return grad_w[:K].to(ctx.weights_device), None if grad_m is None else grad_m[:K].to(ctx.compat_device)


def _grad_in(grad_q, device):
    return grad_q.detach().to(device=device, dtype=torch.float32).contiguous()


def _modes(normalization, K):
    """None (every term AFTER, the reference's form), one NORMALIZE_* mode for every term, or one per term -> the modes to set"""
    return [] if normalization is None else np.broadcast_to(np.asarray(normalization, np.int64), (K,)).tolist()


def _host_f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32)


def _weights_parameter(weights):
    return torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))


def _identities(K, L):
    """the Potts model as a [K, L, L] parameter"""
    return torch.nn.Parameter(torch.eye(int(L), dtype=torch.float32).repeat(K, 1, 1))


# ---- a caller's handle -----------------------------------------------------------------------------------------------------------
class _MeanField(torch.autograd.Function):
    """mean_field (compat None), mean_field_compat and -- with a stop rule -- mean_field_converged on a caller's DenseCRFHIP"""

    @staticmethod
    def forward(ctx, crf, unary, weights, compat, n_iterations, relax, stop):
        _check_unary_weights(unary, (crf.N, crf.L), weights, len(crf._d))
        _check_compat_iterations(compat, len(crf._d), crf.L, n_iterations)
        _check_stop(stop, compat)
        u = unary.detach().contiguous()
        w, m = _model(weights, compat)
        with _on_stream(crf.stream(), u.device) as (ext, cur):
            _arm(crf, w, m)
            crf.set_unary_device(u.data_ptr())
            if stop is None:
                q = _forward_q(crf, u, n_iterations, relax, ext, cur)
            else:                                             # (section 1h: the backward is the fixed-count one at the reported count)
                n_iterations = crf.inference_converged(int(n_iterations), int(stop[0]), float(stop[1]), False, float(relax))["iterations"]
                crf.synchronize()
                q = _clone_q(crf.device_buffers()["current"], tuple(u.shape), u.device, ext, cur)
        _remember(ctx, crf, n_iterations, relax, weights, compat)
        ctx.save_for_backward(u, w, m)
        if stop is None:
            return q
        it = torch.tensor(n_iterations, dtype=torch.int32, device=u.device)
        ctx.mark_non_differentiable(it)
        return q, it

    @staticmethod
    def backward(ctx, grad_q, *_):
        u, w, m = ctx.saved_tensors
        crf, dev, K = ctx.target, u.device, int(w.numel())
        g = _grad_in(grad_q, dev)
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr, grad_m = _grad_buffers(K, crf.L, dev, m is not None)
        with _on_stream(crf.stream(), dev):
            _arm(crf, w, m)                                   # the inputs of this forward (the handle may have run others since)
            crf.set_unary_device(u.data_ptr())
            # (without d_grad_compat the call is lccrf_inference_backward, section 1c)
            crf.inference_backward_compat_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr,
                                                 None if grad_m is None else grad_m.data_ptr())
        return (None, grad_u) + _model_grads(ctx, grad_w, grad_m, K) + (None, None, None)


def mean_field(crf, unary, weights, n_iterations=5, relax=1.0):
    """Q_T of DenseCRF::inference(n_iterations, relax) with unary energies `unary` [N, L] (float32, GPU) and pairwise
    weights `weights` [K] (float32, any device) on the terms of `crf`; differentiable in both."""
    return _MeanField.apply(crf, unary, weights, None, n_iterations, relax, None)


def mean_field_compat(crf, unary, weights, compat, n_iterations=5, relax=1.0):
    """mean_field with a label-compatibility matrix per term (include/lccrf.h section 1e): `compat` [K, L, L] (float32, any
    device), term k adding w_k * norm_k * (Phi_k(Q) @ compat[k].T); differentiable in unary, weights and compat.  The matrices
    are left set on `crf`."""
    return _MeanField.apply(crf, unary, weights, compat, n_iterations, relax, None)


def mean_field_converged(crf, unary, weights, max_iterations, criterion=_pkg.STOP_LABELS, tol=0.0, relax=1.0):
    """mean_field "until converged, at most max_iterations" (include/lccrf.h section 1h: criterion a STOP_* bit set, tol for STOP_DELTA):
    returns (Q_t, t) -- t the reported iteration count, an int32 scalar tensor, not differentiable -- and the backward is mean_field's
    at t, section 1h's recipe for the gradient of the converged result."""
    return _MeanField.apply(crf, unary, weights, None, max_iterations, relax, (criterion, tol))


def _option_attribute(owner):
    """the layers' fused_multilabel: a bool attribute whose assignment puts OPT_FUSED_MULTILABEL on the handle or batch the layer owns
    (`owner`: the attribute holding it); takes effect with the next forward"""
    def get(self):
        return self.__dict__.get("_fused_multilabel", False)

    def put(self, value):
        getattr(self, owner).set_option(_pkg.OPT_FUSED_MULTILABEL, 1 if value else 0)
        self.__dict__["_fused_multilabel"] = bool(value)
    return property(get, put)


def _route_attribute(owner):
    """the layers' fused_multilabel_learnt, after _option_attribute's pattern: a bool attribute whose assignment sets or clears
    MULTILABEL_LEARNT among the multilabel routes of the handle or batch the layer owns (the other route bits stay as they are);
    takes effect with the next forward"""
    def get(self):                                            # (the handle's own bit: it cannot drift from a direct set_multilabel_routes)
        return bool(getattr(self, owner).multilabel_routes() & _pkg.MULTILABEL_LEARNT)

    def put(self, value):
        crf = getattr(self, owner)
        routes = crf.multilabel_routes() & ~_pkg.MULTILABEL_LEARNT
        crf.set_multilabel_routes(routes | (_pkg.MULTILABEL_LEARNT if value else 0))
    return property(get, put)


class _HandleCRF(torch.nn.Module):
    """what MeanFieldCRF and CompatMeanFieldCRF share: a DenseCRFHIP handle over fixed features, the term weights an nn.Parameter"""

    def __init__(self, n_points, n_labels, features, weights, n_iterations, relax, device, normalization=None):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        self.crf = _pkg.DenseCRFHIP(n_points, n_labels, device=device)
        for f, w in zip(features, weights):
            self.crf.add_pairwise(_host_f32(f), float(w))
        for k, mode in enumerate(_modes(normalization, len(features))):      # (include/lccrf.h section 1g)
            self.crf.set_normalization(k, mode)
        self.weights = _weights_parameter(weights)
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def close(self):
        self.crf.close()


class MeanFieldCRF(_HandleCRF):
    """A dense CRF layer: a DenseCRFHIP handle over fixed features, its term weights an nn.Parameter.

    features: list of [N, d_k] arrays (already divided by the kernel's standard deviation, as lccrf_add_pairwise takes
    them); weights: their initial weights; normalization: None (the reference's form), or one of the package's NORMALIZE_* modes
    for every term, or one per term (include/lccrf.h section 1g); fused_backward: sets OPT_FUSED_BACKWARD on the handle -- the
    gradients of a frame the one-launch backward takes are then formed in one launch, the same bits (section 1j);
    the attribute fused_multilabel (False; the constructor's parameter list is kept as it was): set to True, it puts
    OPT_FUSED_MULTILABEL on the handle -- the forward of a frame of three to eight labels the fused plan takes then runs in one
    launch, the same bits; the backward is unchanged.  The attribute fused_multilabel_learnt (False) does the same with
    MULTILABEL_LEARNT for a layer with a `normalization` other than AFTER (engine 6).
    forward(unary [N, L]) -> Q [N, L]."""

    def __init__(self, n_points, n_labels, features, weights, n_iterations=5, relax=1.0, device=0, normalization=None,
                 fused_backward=False):
        super().__init__(n_points, n_labels, features, weights, n_iterations, relax, device, normalization)
        if fused_backward:
            self.crf.set_option(_pkg.OPT_FUSED_BACKWARD, 1)

    fused_multilabel = _option_attribute("crf")
    fused_multilabel_learnt = _route_attribute("crf")

    def forward(self, unary):
        return mean_field(self.crf, unary, self.weights, self.n_iterations, self.relax)


class CompatMeanFieldCRF(_HandleCRF):
    """MeanFieldCRF whose terms carry a learnt label-compatibility matrix: parameters `weights` [K] and `compat` [K, L, L], the
    latter initialised to identities (the Potts model); normalization as MeanFieldCRF takes it; fused_backward: sets OPT_FUSED_BACKWARD
    and OPT_FUSED_BACKWARD_LEARNT on the handle -- the gradients of frames the fused plan takes run in one launch (include/lccrf.h
    sections 1j and 1k; the same bits); the attribute fused_multilabel_learnt (False; not a constructor argument): set to True, it puts
    MULTILABEL_LEARNT on the handle -- the forward of a frame of three to eight labels the plan takes then runs in one launch (engine
    6), the same bits; the backward is unchanged.  forward(unary [N, L]) -> Q [N, L]."""

    def __init__(self, n_points, n_labels, features, weights, n_iterations=5, relax=1.0, device=0, normalization=None,
                 fused_backward=False):
        super().__init__(n_points, n_labels, features, weights, n_iterations, relax, device, normalization)
        if fused_backward:
            self.crf.set_option(_pkg.OPT_FUSED_BACKWARD, 1)
            self.crf.set_option(_pkg.OPT_FUSED_BACKWARD_LEARNT, 1)
        self.compat = _identities(len(weights), n_labels)

    fused_multilabel_learnt = _route_attribute("crf")

    def forward(self, unary):
        return mean_field_compat(self.crf, unary, self.weights, self.compat, self.n_iterations, self.relax)


# ---- a caller's batch ------------------------------------------------------------------------------------------------------------
class _MeanFieldBatch(torch.autograd.Function):
    """mean_field_batch (compat None), mean_field_batch_compat and -- with a stop rule -- mean_field_batch_converged and
    mean_field_batch_compat_converged on a caller's BatchCRF.  The backwards are different calls: without matrices section 2c, which
    refuses a batch that carries matrices or modes, and torch's sum of its [F, K] output (under a stop rule section 2j, section 2c at
    every frame's own count); with them section 2h, whose model gradients are the batch's own ordered sums over the frames (under a
    stop rule section 2k, section 2h at every frame's own count).
    With `bind` and the K feature tensors behind it: mean_field_batch_features and mean_field_batch_features_converged -- the forward
    binds its own inputs to the batch and builds the lattices, the backward is section 2i's call (under a stop rule section 2l's) with
    a feature array for every tensor that needs a gradient."""

    @staticmethod
    def forward(ctx, batch, unary, weights, compat, n_iterations, relax, n_points, stop, bind=False, *features):
        F, N, L = len(n_points) if bind else batch.n_frames, batch.maxN, batch.L
        _check_unary_weights(unary, (F, N, L), weights, len(batch.dims))
        _check_compat_iterations(compat, len(batch.dims), L, n_iterations)
        _check_stop(stop, compat, batch=True)
        dev = unary.device
        u = unary.detach().contiguous()
        w, m = _model(weights, compat)
        it = None
        fs = _check_batch_features(features, batch.dims, F, N) if bind else []
        with _on_stream(batch.own_stream(), dev) as (ext, cur):
            if bind:
                ctx.n_points = np.ascontiguousarray(n_points, np.int32)
                ctx.serial = _bind_and_build(batch, ctx.n_points, u, fs)
            _arm(batch, w, m)
            batch.set_unary_device(u.data_ptr())
            if stop is None:
                batch.inference(int(n_iterations), False, float(relax))      # (leaves nothing to settle)
            else:
                batch.inference_converged(int(n_iterations), int(stop[0]), float(stop[1]), False, float(relax))
                # the counts, CLONED on the batch's stream: the backward re-arms the batch and sets the unaries again, which may
                # invalidate the stored report
                with torch.cuda.stream(ext):
                    it = _device_view(batch.device_convergence()["iterations"], (F,), dev, "<i4").clone()
                it.record_stream(cur)
            q = _clone_q(batch.device_buffers()[1], (F, N, L), dev, ext, cur)
        live = torch.arange(N, device=dev)[None, :] < torch.as_tensor(n_points, device=dev)[:, None]
        q = torch.where(live[:, :, None], q, torch.zeros((), device=dev))    # rows beyond a frame's points: 0
        _remember(ctx, batch, n_iterations, relax, weights, compat)
        ctx.bind = bool(bind)
        ctx.save_for_backward(u, w, m, it, *fs)
        if it is None:
            return q
        ctx.mark_non_differentiable(it)
        return q, it

    @staticmethod
    def backward(ctx, grad_q, *_):
        u, w, m, it = ctx.saved_tensors[:4]
        batch, dev = ctx.target, u.device
        K, L = int(w.numel()), batch.L
        g = _grad_in(grad_q, dev)
        grad_u = torch.empty_like(u)
        if ctx.bind:
            return _MeanFieldBatch._backward_features(ctx, g, grad_u, u, w, m, it, list(ctx.saved_tensors[4:]))
        if m is None:
            grad_w = torch.empty((batch.n_frames, max(K, 1)), dtype=torch.float32, device=dev)
        else:
            model = torch.zeros(max(K * (1 + L * L), 1), dtype=torch.float32, device=dev)
        with _on_stream(batch.own_stream(), dev):
            _arm(batch, w, m)                                 # the inputs of this forward (the batch may have run others since)
            batch.set_unary_device(u.data_ptr())
            if it is not None and m is not None:              # (section 2k: section 2h's sums, every frame at its own count)
                batch.inference_backward_all_converged_device(ctx.n_iterations, ctx.relax, it.data_ptr(), g.data_ptr(), grad_u.data_ptr(),
                                                              d_grad_model=model.data_ptr() if K else None)
            elif it is not None:                              # (section 2j: the cap, and every frame's own count from the device)
                batch.inference_backward_converged_device(ctx.n_iterations, ctx.relax, it.data_ptr(), g.data_ptr(), grad_u.data_ptr(),
                                                          grad_w.data_ptr() if K else None)
            elif m is None:
                batch.inference_backward_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(),
                                                grad_w.data_ptr() if K else None)
            else:
                batch.inference_backward_all_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(),
                                                    d_grad_model=model.data_ptr() if K else None)
        if m is None:
            return None, grad_u, grad_w[:, :K].sum(0).to(ctx.weights_device), None, None, None, None, None
        return (None, grad_u, model[:K].to(ctx.weights_device), model[K:K * (1 + L * L)].reshape(K, L, L).to(ctx.compat_device),
                None, None, None, None)

    @staticmethod
    def _backward_features(ctx, g, grad_u, u, w, m, it, fs):
        """the backward of the functions that take the features: section 2i's call, under a stop rule section 2l's.  With matrices the
        model's gradients are the batch's own ordered sums (d_grad_model, no torch reduction); without them the request stays in the
        plain form -- per-frame dL/dw, summed by torch as mean_field_batch does -- which is the form OPT_FUSED_BACKWARD_FEATURES takes
        in one launch (include/lccrf.h section 1l)."""
        batch, dev = ctx.target, u.device
        K, L, F = int(w.numel()), batch.L, int(u.shape[0])
        grad_f = [torch.empty_like(f) if ctx.needs_input_grad[9 + k] else None for k, f in enumerate(fs)]
        ptrs = [t.data_ptr() if t is not None else None for t in grad_f]
        model = torch.zeros(max(K * (1 + L * L), 1), dtype=torch.float32, device=dev) if m is not None else None
        grad_w = torch.empty((F, max(K, 1)), dtype=torch.float32, device=dev) if m is None else None
        gw_ptr, md_ptr = (grad_w.data_ptr() if K else None, None) if m is None else (None, model.data_ptr() if K else None)
        with _on_stream(batch.own_stream(), dev):
            if batch.inputs_serial != ctx.serial:             # the batch has been given other inputs since: this forward's again
                ctx.serial = _bind_and_build(batch, ctx.n_points, u, fs)
            _arm(batch, w, m)                                 # (the weights, matrices and unaries may be another forward's too)
            batch.set_unary_device(u.data_ptr())
            if it is not None:
                batch.inference_backward_modes_converged_device(ctx.n_iterations, ctx.relax, it.data_ptr(), g.data_ptr(), grad_u.data_ptr(),
                                                                gw_ptr, ptrs, None, md_ptr)
            else:
                batch.inference_backward_modes_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), gw_ptr, ptrs, None,
                                                      md_ptr)
        if m is None:
            gw, gm = grad_w[:, :K].sum(0).to(ctx.weights_device), None
        else:
            gw, gm = model[:K].to(ctx.weights_device), model[K:K * (1 + L * L)].reshape(K, L, L).to(ctx.compat_device)
        return (None, grad_u, gw, gm, None, None, None, None, None) + tuple(grad_f)


def _check_batch_features(features, dims, F, N):
    """the K feature tensors of a batch function: float32, on the GPU, [F, max_points, d_k] -> detached and contiguous"""
    if len(features) != len(dims):
        raise ValueError("one feature tensor per term of the batch (%d)" % len(dims))
    for f, d in zip(features, dims):
        if not f.is_cuda or f.dtype != torch.float32 or tuple(f.shape) != (F, N, d):
            raise ValueError("every feature tensor must be a float32 GPU tensor of shape [%d, %d, d_k]" % (F, N))
    return [f.detach().contiguous() for f in features]


def _bind_and_build(batch, n_points, u, fs):
    """bind one forward's unaries and features to the batch (lccrf_batch_bind_inputs_device: bound, not copied -- the batch keeps
    them alive) and build the lattices (inside _on_stream); returns the batch's inputs_serial, by which a backward tells whether the
    batch still holds them.  The point counts go to the device from the host's and are complete before the call, as it demands."""
    d_np = torch.as_tensor(n_points, dtype=torch.int32).to(u.device)
    torch.cuda.current_stream(u.device).synchronize()
    batch.bind_inputs_device(int(n_points.size), d_np.data_ptr(), [f.data_ptr() for f in fs], d_unary=u.data_ptr())
    batch.n_points = n_points.copy()                          # (known here, although they were bound from the device)
    batch._bound = (d_np, u, fs)
    batch.build()
    return batch.inputs_serial


def _apply_batch(batch, unary, weights, compat, n_iterations, relax, stop=None):
    if batch.n_points is None:
        raise ValueError("the batch's point counts are on the device only (bind_inputs_device): set its inputs from the host")
    return _MeanFieldBatch.apply(batch, unary, weights, compat, n_iterations, relax, batch.n_points, stop)


def mean_field_batch(batch, unary, weights, n_iterations=5, relax=1.0):
    """Q_T [F, max_points, L] of every frame's DenseCRF::inference(n_iterations, relax) on a built BatchCRF (inputs set with host
    point counts, lattices built: build() or run()), with unary energies `unary` [F, max_points, L] (float32, GPU) and the batch's
    term weights `weights` [K] (float32, any device); differentiable in both.  Rows beyond a frame's points are 0 in Q and in
    unary.grad; weights.grad is the sum over the frames of their dL/dw."""
    return _apply_batch(batch, unary, weights, None, n_iterations, relax)


def mean_field_batch_compat(batch, unary, weights, compat, n_iterations=5, relax=1.0):
    """mean_field_batch with a label-compatibility matrix per term (include/lccrf.h sections 2g and 2h): `compat` [K, L, L] (float32,
    any device), shared by every frame; differentiable in unary, weights and compat.  weights.grad and compat.grad are the sums over
    the frames of dL/dw and dL/dmu, formed by the batch's own call in ascending frame order (no torch reduction).  The matrices are left
    set on `batch`; its normalisation modes are honoured."""
    return _apply_batch(batch, unary, weights, compat, n_iterations, relax)


def mean_field_batch_converged(batch, unary, weights, max_iterations, criterion=_pkg.STOP_LABELS, tol=0.0, relax=1.0):
    """mean_field_batch "until converged, at most max_iterations": every frame stops on its own (include/lccrf.h section 2e; criterion
    a STOP_* bit set, tol for STOP_DELTA).  Returns (Q [F, max_points, L], iterations [F] int32 on the GPU, not differentiable): frame
    f's rows are Q_{t_f}, t_f = iterations[f], a clone of the batch's device report.  The backward differentiates every frame at its
    own t_f in one call on those counts, which never visit the host (section 2j); unary.grad and weights.grad as mean_field_batch.
    Potts terms normalised AFTER only."""
    return _apply_batch(batch, unary, weights, None, max_iterations, relax, (criterion, tol))


def mean_field_batch_compat_converged(batch, unary, weights, compat, max_iterations, criterion=_pkg.STOP_LABELS, tol=0.0, relax=1.0):
    """mean_field_batch_compat "until converged, at most max_iterations": the learnt model under the stop rule it is deployed with
    (include/lccrf.h sections 2e and 2k).  Returns (Q [F, max_points, L], iterations [F] int32 on the GPU, not differentiable) as
    mean_field_batch_converged does.  The backward differentiates every frame at its own t_f in one call on the cloned device counts;
    weights.grad and compat.grad are the batch's own ordered sums over the frames (no torch reduction).  The matrices are left set on
    `batch`; its normalisation modes are honoured."""
    return _apply_batch(batch, unary, weights, compat, max_iterations, relax, (criterion, tol))


def mean_field_batch_features(batch, n_points, unary, features, weights, n_iterations=5, relax=1.0, compat=None):
    """mean_field_batch with the features as inputs: `features` a list of K [F, max_points, d_k] float32 GPU tensors (already divided
    by the kernels' standard deviations), `n_points` [F] host integers, `unary` [F, max_points, L].  The forward binds the tensors to
    `batch` (BatchCRF.bind_inputs_device), builds every frame's lattices, sets weights and -- with `compat` [K, L, L] -- matrices, and
    runs inference(n_iterations, relax); the batch's normalisation modes are honoured.  Differentiable in unary, every features[k],
    weights and compat: one lccrf_batch_inference_backward_modes call (include/lccrf.h section 2i) with a feature array per tensor
    that needs a gradient.  With compat, weights.grad and compat.grad are the batch's own ordered sums over the frames (d_grad_model);
    without, weights.grad is torch's sum of the per-frame dL/dw, and the request is one OPT_FUSED_BACKWARD_FEATURES takes in one
    launch.  A backward behind another forward on the same batch binds and builds its own inputs again."""
    return _MeanFieldBatch.apply(batch, unary, weights, compat, n_iterations, relax, n_points, None, True, *features)


def mean_field_batch_features_converged(batch, n_points, unary, features, weights, max_iterations, criterion=_pkg.STOP_LABELS, tol=0.0,
                                        relax=1.0, compat=None):
    """mean_field_batch_features "until converged, at most max_iterations": every frame stops on its own (include/lccrf.h section 2e).
    Returns (Q [F, max_points, L], iterations [F] int32 on the GPU, not differentiable), the counts a clone of the batch's device report
    taken on the batch's stream.  The backward differentiates every frame at its own count, dL/d features included, in one
    lccrf_batch_inference_backward_modes_converged call on those counts (section 2l); everything else as mean_field_batch_features."""
    return _MeanFieldBatch.apply(batch, unary, weights, compat, max_iterations, relax, n_points, (criterion, tol), True, *features)


class _BatchCRF(torch.nn.Module):
    """what BatchMeanFieldCRF and BatchCompatMeanFieldCRF share: one BatchCRF over fixed per-frame features, uploaded and its lattices
    built once, here; the term weights (shared by every frame) an nn.Parameter"""

    def __init__(self, n_points, features, weights, n_iterations, relax, device, n_labels, normalization=None):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        feats = [_host_f32(f) for f in features]
        n_points = np.ascontiguousarray(n_points, np.int32)
        F = int(n_points.size)
        N = int(feats[0].shape[1]) if feats else int(n_points.max(initial=0))
        self.batch = _pkg.BatchCRF(F, N, n_labels, [f.shape[2] for f in feats], [float(w) for w in weights], device=device)
        for k, mode in enumerate(_modes(normalization, len(feats))):      # (include/lccrf.h section 2g)
            self.batch.set_normalization(k, mode)
        self.batch.set_inputs_host(n_points, feats, unary=np.zeros((F, N, n_labels), np.float32))
        self.batch.build()
        self.weights = _weights_parameter(weights)
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def close(self):
        self.batch.close()


class BatchMeanFieldCRF(_BatchCRF):
    """A dense CRF layer over many frames: one BatchCRF over fixed per-frame features, the term weights (shared by every frame) an
    nn.Parameter.  The features are uploaded and the lattices built once, here; forward() only sets weights and unaries.

    n_points: [F] points per frame; features: list of [F, max_points, d_k] arrays (already divided by the kernel's standard
    deviation); weights: their initial weights; fused_backward: sets OPT_FUSED_BACKWARD on the batch (include/lccrf.h section 1j: the
    same gradients, in one launch where the frames fit); the attribute fused_multilabel (False; the constructor's parameter list is
    kept as it was): set to True, it puts OPT_FUSED_MULTILABEL on the batch (the forward of frames of three to eight labels in one
    launch where the plan fits, the same bits; the backward is unchanged); the attribute fused_multilabel_learnt (False) is the
    batch's MULTILABEL_LEARNT route, as on BatchCompatMeanFieldCRF.
    forward(unary [F, max_points, L]) -> Q [F, max_points, L]."""

    def __init__(self, n_points, features, weights, n_iterations=5, relax=1.0, device=0, n_labels=2, fused_backward=False):
        super().__init__(n_points, features, weights, n_iterations, relax, device, n_labels)
        if fused_backward:
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD, 1)

    fused_multilabel = _option_attribute("batch")
    fused_multilabel_learnt = _route_attribute("batch")

    def forward(self, unary):
        return mean_field_batch(self.batch, unary, self.weights, self.n_iterations, self.relax)


class BatchConvergedMeanFieldCRF(_BatchCRF):
    """BatchMeanFieldCRF under the stop rule the model is deployed with: forward(unary [F, max_points, L]) -> (Q [F, max_points, L],
    iterations [F] int32) through mean_field_batch_converged -- every frame inferred until ITS criterion holds, at most max_iterations,
    and differentiated at its own count (include/lccrf.h sections 2e and 2j).  criterion, tol: as BatchCRF.inference_converged takes
    them; fused_backward: sets OPT_FUSED_BACKWARD on the batch (section 1j: the same gradients, in one launch where the frames fit)."""

    def __init__(self, n_points, features, weights, max_iterations=12, criterion=_pkg.STOP_LABELS, tol=0.0, relax=1.0, device=0,
                 n_labels=2, fused_backward=False):
        super().__init__(n_points, features, weights, max_iterations, relax, device, n_labels)
        self.criterion, self.tol = int(criterion), float(tol)
        if fused_backward:
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD, 1)

    def forward(self, unary):
        return mean_field_batch_converged(self.batch, unary, self.weights, self.n_iterations, self.criterion, self.tol, self.relax)


class BatchCompatMeanFieldCRF(_BatchCRF):
    """BatchMeanFieldCRF whose terms carry a learnt label-compatibility matrix: parameters `weights` [K] and `compat` [K, L, L], the
    latter initialised to identities (the Potts model), both shared by every frame; normalization: None (the reference's form), one of
    the package's NORMALIZE_* modes for every term, or one per term, set once; fused_backward: sets OPT_FUSED_BACKWARD and
    OPT_FUSED_BACKWARD_LEARNT on the batch (include/lccrf.h sections 1j and 1k: the same bits in one launch plus the two of the sums
    over the frames); the attribute fused_multilabel_learnt (False; not a constructor argument): set to True, it puts
    MULTILABEL_LEARNT on the batch -- the forward of frames of three to eight labels the plan takes in one launch (engine 6), the same
    bits; the backward is unchanged.  The features are uploaded and the lattices built once, here.
    forward(unary [F, max_points, L]) -> Q [F, max_points, L]."""

    def __init__(self, n_points, features, weights, n_iterations=5, relax=1.0, device=0, n_labels=2, normalization=None,
                 fused_backward=False):
        super().__init__(n_points, features, weights, n_iterations, relax, device, n_labels, normalization)
        if fused_backward:
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD, 1)
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD_LEARNT, 1)
        self.compat = _identities(len(weights), n_labels)

    fused_multilabel_learnt = _route_attribute("batch")

    def forward(self, unary):
        return mean_field_batch_compat(self.batch, unary, self.weights, self.compat, self.n_iterations, self.relax)


class BatchCompatConvergedMeanFieldCRF(_BatchCRF):
    """BatchCompatMeanFieldCRF under the stop rule the model is deployed with: forward(unary [F, max_points, L]) -> (Q [F, max_points,
    L], iterations [F] int32) through mean_field_batch_compat_converged -- every frame inferred until ITS criterion holds, at most
    max_iterations, and differentiated at its own count (include/lccrf.h sections 2e and 2k).  Parameters `weights` [K] and `compat`
    [K, L, L] (identities at first) and normalization as BatchCompatMeanFieldCRF; criterion, tol as BatchCRF.inference_converged takes
    them; fused_backward: sets OPT_FUSED_BACKWARD and OPT_FUSED_BACKWARD_LEARNT on the batch (the same bits, in one launch where the
    frames fit, plus the two of the sums over the frames)."""

    def __init__(self, n_points, features, weights, max_iterations=12, criterion=_pkg.STOP_LABELS, tol=0.0, relax=1.0, device=0,
                 n_labels=2, normalization=None, fused_backward=False):
        super().__init__(n_points, features, weights, max_iterations, relax, device, n_labels, normalization)
        self.criterion, self.tol = int(criterion), float(tol)
        if fused_backward:
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD, 1)
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD_LEARNT, 1)
        self.compat = _identities(len(weights), n_labels)

    def forward(self, unary):
        return mean_field_batch_compat_converged(self.batch, unary, self.weights, self.compat, self.n_iterations, self.criterion,
                                                 self.tol, self.relax)


# ---- a handle of its own: the features are inputs --------------------------------------------------------------------------------
class _MeanFieldFeatures(torch.autograd.Function):
    """mean_field_features (compat None) and mean_field_learned: the lattices depend on the features, so a handle per forward
    (lccrf_create re-uses parked handles), which the backward closes"""

    @staticmethod
    def forward(ctx, unary, weights, compat, n_iterations, relax, device, fused_backward, route_out, normalization, *features):
        _check_unary_weights(unary, None, weights, len(features))
        N, L = (int(x) for x in unary.shape)
        for f in features:
            if not f.is_cuda or f.dtype != torch.float32 or f.dim() != 2 or int(f.shape[0]) != N:
                raise ValueError("every feature array must be a float32 GPU tensor of shape [%d, d_k]" % N)
        _check_compat_iterations(compat, len(features), L, n_iterations)
        u = unary.detach().contiguous()
        fs = [f.detach().contiguous() for f in features]
        crf = _pkg.DenseCRFHIP(N, L, device=device)
        if fused_backward:                                    # (lccrf_create hands out handles with fresh options: nothing leaks)
            crf.set_option(_pkg.OPT_FUSED_BACKWARD_FEATURES, 1)
        ctx.route_out = route_out
        # (include/lccrf.h sections 1g and 1m: a term that is not AFTER sends the backward to lccrf_inference_backward_modes)
        modes = _modes(normalization, len(features))
        ctx.any_mode = any(mode != _pkg.NORMALIZE_AFTER for mode in modes)
        with _on_stream(crf.stream(), u.device) as (ext, cur):
            crf.set_unary_device(u.data_ptr())
            for f, w in zip(fs, weights.detach().cpu().tolist()):
                crf.add_pairwise_device(f.data_ptr(), int(f.shape[1]), w)
            for k, mode in enumerate(modes if ctx.any_mode else []):
                crf.set_normalization(k, mode)
            _set_matrices(crf, compat)
            q = _forward_q(crf, u, n_iterations, relax, ext, cur)
        _remember(ctx, crf, n_iterations, relax, weights, compat)
        ctx.name = "mean_field_features" if compat is None else "mean_field_learned"
        ctx.save_for_backward(u, *fs)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, fs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        crf = ctx.target
        if crf is None:
            raise RuntimeError("%s: backward a second time (the handle is closed by the first)" % ctx.name)
        dev, K = u.device, len(fs)
        g = _grad_in(grad_q, dev)
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr, grad_m = _grad_buffers(K, int(u.shape[1]), dev, ctx.compat_device is not None)
        grad_f = [torch.empty_like(f) if ctx.needs_input_grad[9 + k] else None for k, f in enumerate(fs)]
        with _on_stream(crf.stream(), dev):                   # (the handle still holds this forward's unary, weights, matrices and modes)
            # (without d_grad_compat, on a handle without matrices, the request is lccrf_inference_backward_features', section 1d)
            call = crf.inference_backward_modes_device if ctx.any_mode else crf.inference_backward_all_device
            call(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr,
                 [t.data_ptr() if t is not None else None for t in grad_f], None if grad_m is None else grad_m.data_ptr())
        crf.synchronize()                                     # (the handle goes back to the cache: nothing of this call may be in flight)
        if isinstance(ctx.route_out, list):
            ctx.route_out.append(crf.backward_route())
        crf.close()
        ctx.target = None
        return (grad_u,) + _model_grads(ctx, grad_w, grad_m, K) + (None, None, None, None, None, None) + tuple(grad_f)


def mean_field_features(unary, features, weights, n_iterations=5, relax=1.0, device=0, fused_backward=False, route_out=None):
    """Q_T of DenseCRF::inference(n_iterations, relax) with unary energies `unary` [N, L] (float32, GPU), pairwise terms over
    `features` (a list of [N, d_k] float32 GPU tensors, already divided by the kernels' standard deviations) and their weights
    `weights` [K] (float32, any device); differentiable in all three.  The feature gradient is the exact derivative of the lattice
    filter inside the simplices the points sit in (include/lccrf.h section 1d).  Every forward builds the lattices afresh on a
    handle of its own, which its backward closes: one backward per forward.  fused_backward: sets OPT_FUSED_BACKWARD_FEATURES on that
    handle -- the gradients of a frame the fused plan takes, dL/d features included, run in one launch with the same bits
    (include/lccrf.h section 1l).  route_out: a list to which the backward appends the handle's backward_route() before it closes it."""
    return _MeanFieldFeatures.apply(unary, weights, None, n_iterations, relax, device, fused_backward, route_out, None, *features)


def mean_field_features_modes(unary, features, weights, normalization, n_iterations=5, relax=1.0, device=0, fused_backward=False,
                              route_out=None):
    """mean_field_features under normalisation modes (include/lccrf.h sections 1g and 1m).  normalization: None (every term AFTER,
    the reference's form), one of the package's NORMALIZE_* modes for every term, or one per term.  With a term that is not AFTER the
    modes are set on the function's own handle before the forward and the backward is lccrf_inference_backward_modes: the norm's
    factors are differentiated in the features too, on the streaming sweep.  With None or every term AFTER the call is
    mean_field_features, bit for bit and route for route."""
    return _MeanFieldFeatures.apply(unary, weights, None, n_iterations, relax, device, fused_backward, route_out, normalization,
                                    *features)


def mean_field_learned(unary, features, weights, compat, n_iterations=5, relax=1.0, device=0):
    """mean_field_features with a label-compatibility matrix per term (include/lccrf.h section 1f): `compat` [K, L, L] (float32,
    any device), term k adding w_k * norm_k * (Phi_k(Q) @ compat[k].T); differentiable in unary, features, weights and compat, all
    four from one reverse sweep.  Every forward builds the lattices afresh on a handle of its own, which its backward closes: one
    backward per forward."""
    return _MeanFieldFeatures.apply(unary, weights, compat, n_iterations, relax, device, False, None, None, *features)


def mean_field_learned_modes(unary, features, weights, compat, normalization, n_iterations=5, relax=1.0, device=0):
    """mean_field_learned under normalisation modes: `normalization` as mean_field_features_modes takes it (include/lccrf.h sections
    1g and 1m); with None or every term AFTER the call is mean_field_learned."""
    return _MeanFieldFeatures.apply(unary, weights, compat, n_iterations, relax, device, False, None, normalization, *features)


def _bandwidth_parameter(d, s, g, dev):
    """one term's bandwidth parameterisation: (log_sd, one value per group, an nn.Parameter; the group of every one of the d columns)"""
    g = [[c] for c in range(d)] if g is None else [list(x) for x in g]
    if sorted(c for x in g for c in x) != list(range(d)):
        raise ValueError("the groups of a term must partition its %d columns" % d)
    s = np.broadcast_to(np.asarray(s, np.float64), (len(g),))
    col = np.empty(d, np.int64)
    for j, x in enumerate(g):
        col[x] = j
    return torch.nn.Parameter(torch.tensor(np.log(s), dtype=torch.float32, device=dev)), torch.as_tensor(col, device=dev)


class LearnedKernelCRF(torch.nn.Module):
    """A dense CRF layer whose kernel standard deviations are learned with the term weights.

    raw_features: list of [N, d_k] arrays or tensors, NOT divided by any standard deviation; sd: per term, the initial standard
    deviations -- one value per feature column, or one per group with `groups` (per term a list of column-index lists, e.g.
    [[0, 1], [2, 3, 4]] so that (x, y) share posdev and (r, g, b) share featuredev; None: every column its own).  The parameters
    are log_sd[k] (one value per group) and weights; forward(unary [N, L]) forms raw * exp(-log_sd) and calls mean_field_features,
    so autograd carries dL/d features to the bandwidths.  fused_backward: passed on to mean_field_features (include/lccrf.h section
    1l: the same bits in one launch); backward_route is the route of the last backward (BACKWARD_NONE before any).
    The attribute `normalization` (None after construction: the reference's form) may be set to one NORMALIZE_* mode for every term,
    or to one per term, with the meaning it has in MeanFieldCRF: the next forward runs under those modes and the bandwidths are learnt
    through the norm's factors too (mean_field_features_modes; include/lccrf.h section 1m)."""

    def __init__(self, raw_features, sd, weights, groups=None, n_iterations=5, relax=1.0, device=0, fused_backward=False):
        super().__init__()
        if not (len(raw_features) == len(sd) == len(weights)):
            raise ValueError("one list of standard deviations and one weight per feature array")
        dev = torch.device("cuda", device)
        self.raw = [torch.as_tensor(_host_f32(f), device=dev) for f in raw_features]
        groups = groups if groups is not None else [None] * len(self.raw)
        self.log_sd = torch.nn.ParameterList()
        self._col = []                                        # per term: group of every column
        for f, s, g in zip(self.raw, sd, groups):
            log_sd, col = _bandwidth_parameter(int(f.shape[1]), s, g, dev)
            self._col.append(col)
            self.log_sd.append(log_sd)
        self.weights = _weights_parameter(weights)
        self.n_iterations, self.relax, self.device = int(n_iterations), float(relax), int(device)
        self.fused_backward = bool(fused_backward)
        self.normalization = None                             # None, one NORMALIZE_* mode for every term, or one per term (section 1m)
        self._routes = []                                     # what the backwards of this layer's forwards reported

    @property
    def backward_route(self):
        return self._routes[-1] if self._routes else _pkg.BACKWARD_NONE

    def features(self):
        """the features the CRF sees: raw / sd, column by column"""
        return [f * torch.exp(-ls)[col] for f, ls, col in zip(self.raw, self.log_sd, self._col)]

    def sd(self):
        return [torch.exp(ls.detach()).cpu().numpy() for ls in self.log_sd]

    def forward(self, unary):
        del self._routes[:-1]
        return mean_field_features_modes(unary, self.features(), self.weights, self.normalization, self.n_iterations, self.relax,
                                         self.device, fused_backward=self.fused_backward, route_out=self._routes)


class LearnedCRF(LearnedKernelCRF):
    """LearnedKernelCRF whose terms also carry a learnt label-compatibility matrix: parameters log_sd[k], `weights` [K] and `compat`
    [K, n_labels, n_labels], the latter initialised to identities (the Potts model).  sd and groups as LearnedKernelCRF takes them.
    The attribute `normalization` as in LearnedKernelCRF.  forward(unary [N, n_labels]) -> Q [N, n_labels] through
    mean_field_learned_modes (mean_field_learned while `normalization` is None)."""

    def __init__(self, raw_features, sd, weights, groups=None, n_labels=2, n_iterations=5, relax=1.0, device=0):
        super().__init__(raw_features, sd, weights, groups, n_iterations, relax, device)
        self.compat = _identities(len(weights), n_labels)

    def forward(self, unary):
        return mean_field_learned_modes(unary, self.features(), self.weights, self.compat, self.normalization, self.n_iterations,
                                        self.relax, self.device)


class BatchLearnedKernelCRF(torch.nn.Module):
    """LearnedKernelCRF over the frames of a batch: the kernel standard deviations (shared by every frame) are learned with the term
    weights, at a fixed count or under the stop rule the model is deployed with.

    n_points: [F] points per frame; raw_features: list of [F, max_points, d_k] arrays or tensors, NOT divided by any standard deviation;
    sd, groups and weights as LearnedKernelCRF takes them.  The parameters are log_sd[k] (one value per group) and weights; forward(unary
    [F, max_points, L]) forms raw * exp(-log_sd) and calls, on a BatchCRF the layer owns, mean_field_batch_features_converged when
    max_iterations is given -- it then returns (Q, iterations [F] int32) -- and mean_field_batch_features at n_iterations otherwise (it
    returns Q): every forward builds the lattices afresh, autograd carries dL/d features to the bandwidths (include/lccrf.h sections 2i
    and 2l).  normalization: None (the reference's form), one NORMALIZE_* mode for every term, or one per term, set once;
    fused_backward: sets OPT_FUSED_BACKWARD_FEATURES on the batch (section 1l: the same bits in one launch where the frames fit and
    every term is normalised AFTER); batch.backward_route() is the route of the last backward."""

    def __init__(self, n_points, raw_features, sd, weights, groups=None, max_iterations=None, n_iterations=5, criterion=_pkg.STOP_LABELS,
                 tol=0.0, relax=1.0, device=0, n_labels=2, normalization=None, fused_backward=False):
        super().__init__()
        if not (len(raw_features) == len(sd) == len(weights)):
            raise ValueError("one list of standard deviations and one weight per feature array")
        dev = torch.device("cuda", device)
        self.raw = [torch.as_tensor(_host_f32(f), device=dev) for f in raw_features]
        self.n_points = np.ascontiguousarray(n_points, np.int32)
        if any(f.dim() != 3 or int(f.shape[0]) != self.n_points.size for f in self.raw):
            raise ValueError("every feature array must be of shape [%d, max_points, d_k]" % self.n_points.size)
        groups = groups if groups is not None else [None] * len(self.raw)
        self.log_sd = torch.nn.ParameterList()
        self._col = []                                        # per term: group of every column
        for f, s, g in zip(self.raw, sd, groups):
            log_sd, col = _bandwidth_parameter(int(f.shape[2]), s, g, dev)
            self._col.append(col)
            self.log_sd.append(log_sd)
        self.weights = _weights_parameter(weights)
        F = int(self.n_points.size)
        N = int(self.raw[0].shape[1]) if self.raw else int(self.n_points.max(initial=0))
        self.batch = _pkg.BatchCRF(F, N, n_labels, [int(f.shape[2]) for f in self.raw], [float(w) for w in weights], device=device)
        for k, mode in enumerate(_modes(normalization, len(self.raw))):      # (include/lccrf.h section 2g)
            self.batch.set_normalization(k, mode)
        if fused_backward:
            self.batch.set_option(_pkg.OPT_FUSED_BACKWARD_FEATURES, 1)
        self.max_iterations = None if max_iterations is None else int(max_iterations)
        self.n_iterations, self.relax = int(n_iterations), float(relax)
        self.criterion, self.tol = int(criterion), float(tol)

    def features(self):
        """the features the CRF sees: raw / sd, column by column, [F, max_points, d_k]"""
        return [f * torch.exp(-ls)[col] for f, ls, col in zip(self.raw, self.log_sd, self._col)]

    def sd(self):
        return [torch.exp(ls.detach()).cpu().numpy() for ls in self.log_sd]

    def forward(self, unary):
        if self.max_iterations is None:
            return mean_field_batch_features(self.batch, self.n_points, unary, self.features(), self.weights, self.n_iterations, self.relax)
        return mean_field_batch_features_converged(self.batch, self.n_points, unary, self.features(), self.weights, self.max_iterations,
                                                   self.criterion, self.tol, self.relax)

    def close(self):
        self.batch.close()

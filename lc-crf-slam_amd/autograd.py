"""torch autograd through DenseCRF::inference on the HIP path (include/lccrf.h sections 1c - 1f and 2c).

    Q = mean_field(crf, unary, weights, n_iterations=5, relax=1.0)
    Q.backward(g)      # -> unary.grad = dL/dU, weights.grad = dL/dw

    Q = mean_field_batch(batch, unary, weights, n_iterations=5, relax=1.0)     # every frame of a BatchCRF at once
    Q.backward(g)      # -> unary.grad [F, max_points, L], weights.grad = sum over the frames of dL/dw

    Q = mean_field_batch_compat(batch, unary, weights, compat, n_iterations=5, relax=1.0)    # ... with a [K, L, L] compatibility
    Q.backward(g)      # -> also compat.grad; both sums over the frames come from the batch's own call (section 2h)

    Q = mean_field_features(unary, [f_0, f_1, ..], weights, n_iterations=5, relax=1.0)        # the features are inputs too
    Q.backward(g)      # -> also f_k.grad = dL/d features [N, d_k] (section 1d); LearnedKernelCRF fits kernel bandwidths with it

    Q = mean_field_compat(crf, unary, weights, compat, n_iterations=5, relax=1.0)             # a [K, L, L] label compatibility
    Q.backward(g)      # -> also compat.grad = dL/dmu (section 1e); CompatMeanFieldCRF learns it, starting from the Potts model

    Q = mean_field_learned(unary, [f_0, f_1, ..], weights, compat, n_iterations=5, relax=1.0)   # features and matrices together
    Q.backward(g)      # -> unary.grad, weights.grad, f_k.grad and compat.grad from one sweep (section 1f); LearnedCRF learns both

`crf` is a DenseCRFHIP whose pairwise terms are already added (their features fix the lattices; only the weights are
inputs here).  Forward: lccrf_set_pairwise_weight + lccrf_set_unary_device + lccrf_inference.  Backward:
lccrf_inference_backward, which replays the forward itself, so nothing but the inputs is kept between the two.

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


def _device_view(ptr, shape, device):
    """A tensor over handle-owned device memory (no copy)."""
    class _View:
        __cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f4", data=(int(ptr), False), version=2)
    return torch.as_tensor(_View(), device=device)


def _check_unary_weights(unary, shape, weights, K):
    """unary: float32, on the GPU, of `shape` (None: any [N, L]); weights: float32 [K]"""
    shape_ok = unary.dim() == 2 if shape is None else tuple(unary.shape) == tuple(shape)
    if not unary.is_cuda or unary.dtype != torch.float32 or not shape_ok:
        wanted = "N, L" if shape is None else ", ".join("%d" % n for n in shape)
        raise ValueError("unary must be a float32 GPU tensor of shape [%s]" % wanted)
    if weights.dtype != torch.float32 or tuple(weights.shape) != (K,):
        raise ValueError("weights must be a float32 tensor of shape [%d]" % K)


def _check_iterations(n_iterations):
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


def _arm(crf, weights, compat=None):
    """the term weights (and label-compatibility matrices) of a forward, set on the handle or batch"""
    for k, w in enumerate(weights.detach().cpu().tolist()):
        crf.set_pairwise_weight(k, w)
    if compat is not None:
        m = compat.cpu().numpy()
        for k in range(m.shape[0]):
            crf.set_pairwise_compatibility(k, m[k])


def _grad_w_buffer(K, device, frames=None):
    """(buffer, the address to pass) for dL/dw: [K], or [frames, K] for a batch; K = 0: a dummy row and NULL"""
    shape = (max(K, 1),) if frames is None else (frames, max(K, 1))
    buf = torch.empty(shape, dtype=torch.float32, device=device)
    return buf, (buf.data_ptr() if K else None)


def _grad_w_result(buf, K, device):
    """dL/dw [K] of a handle from its buffer (K = 0: an empty tensor), on the device the weights came from"""
    if K == 0:
        buf = torch.zeros(0, dtype=torch.float32, device=buf.device)
    return buf[:K].to(device)


def _grad_in(grad_q, device):
    return grad_q.detach().to(device=device, dtype=torch.float32).contiguous()


class _MeanField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, crf, unary, weights, n_iterations, relax):
        _check_unary_weights(unary, (crf.N, crf.L), weights, len(crf._d))
        _check_iterations(n_iterations)
        u = unary.detach().contiguous()
        _arm(crf, weights)
        with _on_stream(crf.stream(), u.device) as (ext, cur):
            crf.set_unary_device(u.data_ptr())
            q = _forward_q(crf, u, n_iterations, relax, ext, cur)
        ctx.crf, ctx.n_iterations, ctx.relax = crf, int(n_iterations), float(relax)
        ctx.weights_device = weights.device
        ctx.save_for_backward(u, weights.detach().clone())
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, w = ctx.saved_tensors
        crf, dev, K = ctx.crf, u.device, int(w.numel())
        g = _grad_in(grad_q, dev)
        _arm(crf, w)                                          # the inputs of this forward (the handle may have run others since)
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr = _grad_w_buffer(K, dev)
        with _on_stream(crf.stream(), dev):
            crf.set_unary_device(u.data_ptr())
            crf.inference_backward_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr)
        return None, grad_u, _grad_w_result(grad_w, K, ctx.weights_device), None, None


def mean_field(crf, unary, weights, n_iterations=5, relax=1.0):
    """Q_T of DenseCRF::inference(n_iterations, relax) with unary energies `unary` [N, L] (float32, GPU) and pairwise
    weights `weights` [K] (float32, any device) on the terms of `crf`; differentiable in both."""
    return _MeanField.apply(crf, unary, weights, n_iterations, relax)


class _HandleCRF(torch.nn.Module):
    """what MeanFieldCRF and CompatMeanFieldCRF share: a DenseCRFHIP handle over fixed features, the term weights an nn.Parameter"""

    def __init__(self, n_points, n_labels, features, weights, n_iterations, relax, device, normalization=None):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        modes = [] if normalization is None else np.broadcast_to(np.asarray(normalization, np.int64), (len(features),)).tolist()
        self.crf = _pkg.DenseCRFHIP(n_points, n_labels, device=device)
        for f, w in zip(features, weights):
            f = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
            self.crf.add_pairwise(np.ascontiguousarray(f, np.float32), float(w))
        for k, mode in enumerate(modes):                      # (include/lccrf.h section 1g; None: every term AFTER, the reference's form)
            self.crf.set_normalization(k, mode)
        self.weights = torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def close(self):
        self.crf.close()


class MeanFieldCRF(_HandleCRF):
    """A dense CRF layer: a DenseCRFHIP handle over fixed features, its term weights an nn.Parameter.

    features: list of [N, d_k] arrays (already divided by the kernel's standard deviation, as lccrf_add_pairwise takes
    them); weights: their initial weights; normalization: None (the reference's form), or one of the package's NORMALIZE_* modes
    for every term, or one per term (include/lccrf.h section 1g).  forward(unary [N, L]) -> Q [N, L]."""

    def __init__(self, n_points, n_labels, features, weights, n_iterations=5, relax=1.0, device=0, normalization=None):
        super().__init__(n_points, n_labels, features, weights, n_iterations, relax, device, normalization)

    def forward(self, unary):
        return mean_field(self.crf, unary, self.weights, self.n_iterations, self.relax)


class _MeanFieldBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, unary, weights, n_iterations, relax, n_points):
        F, N, L = batch.n_frames, batch.maxN, batch.L
        _check_unary_weights(unary, (F, N, L), weights, len(batch.dims))
        _check_iterations(n_iterations)
        dev = unary.device
        u = unary.detach().contiguous()
        _arm(batch, weights)
        with _on_stream(batch.own_stream(), dev) as (ext, cur):
            batch.set_unary_device(u.data_ptr())
            batch.inference(int(n_iterations), False, float(relax))      # (leaves nothing to settle)
            q = _clone_q(batch.device_buffers()[1], (F, N, L), dev, ext, cur)
        live = torch.arange(N, device=dev)[None, :] < torch.as_tensor(n_points, device=dev)[:, None]
        q = torch.where(live[:, :, None], q, torch.zeros((), device=dev))    # rows beyond a frame's points: 0
        ctx.batch, ctx.n_iterations, ctx.relax = batch, int(n_iterations), float(relax)
        ctx.weights_device = weights.device
        ctx.save_for_backward(u, weights.detach().clone())
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, w = ctx.saved_tensors
        batch, dev, K = ctx.batch, u.device, int(w.numel())
        g = _grad_in(grad_q, dev)
        _arm(batch, w)                                        # the inputs of this forward (the batch may have run others since)
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr = _grad_w_buffer(K, dev, batch.n_frames)
        with _on_stream(batch.own_stream(), dev):
            batch.set_unary_device(u.data_ptr())
            batch.inference_backward_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr)
        return None, grad_u, grad_w[:, :K].sum(0).to(ctx.weights_device), None, None, None


def mean_field_batch(batch, unary, weights, n_iterations=5, relax=1.0):
    """Q_T [F, max_points, L] of every frame's DenseCRF::inference(n_iterations, relax) on a built BatchCRF (inputs set with host
    point counts, lattices built: build() or run()), with unary energies `unary` [F, max_points, L] (float32, GPU) and the batch's
    term weights `weights` [K] (float32, any device); differentiable in both.  Rows beyond a frame's points are 0 in Q and in
    unary.grad; weights.grad is the sum over the frames of their dL/dw."""
    if batch.n_points is None:
        raise ValueError("the batch's point counts are on the device only (bind_inputs_device): set its inputs from the host")
    return _MeanFieldBatch.apply(batch, unary, weights, n_iterations, relax, batch.n_points)


class BatchMeanFieldCRF(torch.nn.Module):
    """A dense CRF layer over many frames: one BatchCRF over fixed per-frame features, the term weights (shared by every frame) an
    nn.Parameter.  The features are uploaded and the lattices built once, here; forward() only sets weights and unaries.

    n_points: [F] points per frame; features: list of [F, max_points, d_k] arrays (already divided by the kernel's standard
    deviation); weights: their initial weights.  forward(unary [F, max_points, L]) -> Q [F, max_points, L]."""

    def __init__(self, n_points, features, weights, n_iterations=5, relax=1.0, device=0, n_labels=2):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        feats = [np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f, np.float32) for f in features]
        n_points = np.ascontiguousarray(n_points, np.int32)
        F = int(n_points.size)
        N = int(feats[0].shape[1]) if feats else int(n_points.max(initial=0))
        self.batch = _pkg.BatchCRF(F, N, n_labels, [f.shape[2] for f in feats], [float(w) for w in weights], device=device)
        self.batch.set_inputs_host(n_points, feats, unary=np.zeros((F, N, n_labels), np.float32))
        self.batch.build()
        self.weights = torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def forward(self, unary):
        return mean_field_batch(self.batch, unary, self.weights, self.n_iterations, self.relax)

    def close(self):
        self.batch.close()


class _MeanFieldBatchCompat(torch.autograd.Function):
    """_MeanFieldCompat for a batch: the model's gradients are the batch's own ordered sums over the frames (section 2h)"""

    @staticmethod
    def forward(ctx, batch, unary, weights, compat, n_iterations, relax, n_points):
        F, N, L, K = batch.n_frames, batch.maxN, batch.L, len(batch.dims)
        _check_unary_weights(unary, (F, N, L), weights, K)
        if compat.dtype != torch.float32 or tuple(compat.shape) != (K, L, L):
            raise ValueError("compat must be a float32 tensor of shape [%d, %d, %d]" % (K, L, L))
        _check_iterations(n_iterations)
        dev = unary.device
        u = unary.detach().contiguous()
        w, m = weights.detach().clone(), compat.detach().clone().contiguous()
        with _on_stream(batch.own_stream(), dev) as (ext, cur):
            _arm(batch, w, m)
            batch.set_unary_device(u.data_ptr())
            batch.inference(int(n_iterations), False, float(relax))      # (leaves nothing to settle)
            q = _clone_q(batch.device_buffers()[1], (F, N, L), dev, ext, cur)
        live = torch.arange(N, device=dev)[None, :] < torch.as_tensor(n_points, device=dev)[:, None]
        q = torch.where(live[:, :, None], q, torch.zeros((), device=dev))    # rows beyond a frame's points: 0
        ctx.batch, ctx.n_iterations, ctx.relax = batch, int(n_iterations), float(relax)
        ctx.weights_device, ctx.compat_device = weights.device, compat.device
        ctx.save_for_backward(u, w, m)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, w, m = ctx.saved_tensors
        batch, dev = ctx.batch, u.device
        K, L = int(w.numel()), batch.L
        g = _grad_in(grad_q, dev)
        grad_u = torch.empty_like(u)
        model = torch.zeros(max(K * (1 + L * L), 1), dtype=torch.float32, device=dev)
        with _on_stream(batch.own_stream(), dev):
            _arm(batch, w, m)                                 # the inputs of this forward (the batch may have run others since)
            batch.set_unary_device(u.data_ptr())
            batch.inference_backward_all_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(),
                                                d_grad_model=model.data_ptr() if K else None)
        return (None, grad_u, model[:K].to(ctx.weights_device), model[K:K * (1 + L * L)].reshape(K, L, L).to(ctx.compat_device),
                None, None, None)


def mean_field_batch_compat(batch, unary, weights, compat, n_iterations=5, relax=1.0):
    """mean_field_batch with a label-compatibility matrix per term (include/lccrf.h sections 2g and 2h): `compat` [K, L, L] (float32,
    any device), shared by every frame; differentiable in unary, weights and compat.  weights.grad and compat.grad are the sums over
    the frames of dL/dw and dL/dmu, formed by the batch's own call in ascending frame order (no torch reduction).  The matrices are left
    set on `batch`; its normalisation modes are honoured."""
    if batch.n_points is None:
        raise ValueError("the batch's point counts are on the device only (bind_inputs_device): set its inputs from the host")
    return _MeanFieldBatchCompat.apply(batch, unary, weights, compat, n_iterations, relax, batch.n_points)


class BatchCompatMeanFieldCRF(torch.nn.Module):
    """BatchMeanFieldCRF whose terms carry a learnt label-compatibility matrix: parameters `weights` [K] and `compat` [K, L, L], the
    latter initialised to identities (the Potts model), both shared by every frame; normalization: None (the reference's form), one of
    the package's NORMALIZE_* modes for every term, or one per term, set once.  The features are uploaded and the lattices built once,
    here.  forward(unary [F, max_points, L]) -> Q [F, max_points, L]."""

    def __init__(self, n_points, features, weights, n_iterations=5, relax=1.0, device=0, n_labels=2, normalization=None):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        feats = [np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f, np.float32) for f in features]
        n_points = np.ascontiguousarray(n_points, np.int32)
        modes = [] if normalization is None else np.broadcast_to(np.asarray(normalization, np.int64), (len(feats),)).tolist()
        F = int(n_points.size)
        N = int(feats[0].shape[1]) if feats else int(n_points.max(initial=0))
        self.batch = _pkg.BatchCRF(F, N, n_labels, [f.shape[2] for f in feats], [float(w) for w in weights], device=device)
        for k, mode in enumerate(modes):                      # (include/lccrf.h section 2g; None: every term AFTER)
            self.batch.set_normalization(k, mode)
        self.batch.set_inputs_host(n_points, feats, unary=np.zeros((F, N, n_labels), np.float32))
        self.batch.build()
        self.weights = torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))
        self.compat = torch.nn.Parameter(torch.eye(int(n_labels), dtype=torch.float32).repeat(len(weights), 1, 1))
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def forward(self, unary):
        return mean_field_batch_compat(self.batch, unary, self.weights, self.compat, self.n_iterations, self.relax)

    def close(self):
        self.batch.close()


def _forward_on_own_handle(unary, features, weights, compat, n_iterations, relax, device):
    """The forward of mean_field_features and mean_field_learned: the lattices depend on the features, so a handle per forward
    (lccrf_create re-uses parked handles), which the backward closes.  compat: [K, L, L] or None (Potts terms).
    Returns (handle, Q, the detached unary, the detached features)."""
    _check_unary_weights(unary, None, weights, len(features))
    N, L = (int(x) for x in unary.shape)
    for f in features:
        if not f.is_cuda or f.dtype != torch.float32 or f.dim() != 2 or int(f.shape[0]) != N:
            raise ValueError("every feature array must be a float32 GPU tensor of shape [%d, d_k]" % N)
    if compat is not None and (compat.dtype != torch.float32 or tuple(compat.shape) != (len(features), L, L)):
        raise ValueError("compat must be a float32 tensor of shape [%d, %d, %d]" % (len(features), L, L))
    _check_iterations(n_iterations)
    u = unary.detach().contiguous()
    fs = [f.detach().contiguous() for f in features]
    crf = _pkg.DenseCRFHIP(N, L, device=device)
    with _on_stream(crf.stream(), u.device) as (ext, cur):
        crf.set_unary_device(u.data_ptr())
        for f, w in zip(fs, weights.detach().cpu().tolist()):
            crf.add_pairwise_device(f.data_ptr(), int(f.shape[1]), w)
        if compat is not None:
            for k, m in enumerate(compat.detach().cpu().numpy()):
                crf.set_pairwise_compatibility(k, m)
        q = _forward_q(crf, u, n_iterations, relax, ext, cur)
    return crf, q, u, fs


class _MeanFieldFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unary, weights, n_iterations, relax, device, *features):
        crf, q, u, fs = _forward_on_own_handle(unary, features, weights, None, n_iterations, relax, device)
        ctx.crf, ctx.n_iterations, ctx.relax = crf, int(n_iterations), float(relax)
        ctx.weights_device = weights.device
        ctx.save_for_backward(u, *fs)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, fs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        crf = ctx.crf
        if crf is None:
            raise RuntimeError("mean_field_features: backward a second time (the handle is closed by the first)")
        dev, K = u.device, len(fs)
        g = _grad_in(grad_q, dev)
        need = ctx.needs_input_grad
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr = _grad_w_buffer(K, dev)
        grad_f = [torch.empty_like(f) if need[5 + k] else None for k, f in enumerate(fs)]
        with _on_stream(crf.stream(), dev):
            crf.inference_backward_features_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr,
                                                   [t.data_ptr() if t is not None else None for t in grad_f])
        crf.synchronize()                                     # (the handle goes back to the cache: nothing of this call may be in flight)
        crf.close()
        ctx.crf = None
        return (grad_u, _grad_w_result(grad_w, K, ctx.weights_device), None, None, None) + tuple(grad_f)


def mean_field_features(unary, features, weights, n_iterations=5, relax=1.0, device=0):
    """Q_T of DenseCRF::inference(n_iterations, relax) with unary energies `unary` [N, L] (float32, GPU), pairwise terms over
    `features` (a list of [N, d_k] float32 GPU tensors, already divided by the kernels' standard deviations) and their weights
    `weights` [K] (float32, any device); differentiable in all three.  The feature gradient is the exact derivative of the lattice
    filter inside the simplices the points sit in (include/lccrf.h section 1d).  Every forward builds the lattices afresh on a
    handle of its own, which its backward closes: one backward per forward."""
    return _MeanFieldFeatures.apply(unary, weights, n_iterations, relax, device, *features)


class LearnedKernelCRF(torch.nn.Module):
    """A dense CRF layer whose kernel standard deviations are learned with the term weights.

    raw_features: list of [N, d_k] arrays or tensors, NOT divided by any standard deviation; sd: per term, the initial standard
    deviations -- one value per feature column, or one per group with `groups` (per term a list of column-index lists, e.g.
    [[0, 1], [2, 3, 4]] so that (x, y) share posdev and (r, g, b) share featuredev; None: every column its own).  The parameters
    are log_sd[k] (one value per group) and weights; forward(unary [N, L]) forms raw * exp(-log_sd) and calls mean_field_features,
    so autograd carries dL/d features to the bandwidths."""

    def __init__(self, raw_features, sd, weights, groups=None, n_iterations=5, relax=1.0, device=0):
        super().__init__()
        if not (len(raw_features) == len(sd) == len(weights)):
            raise ValueError("one list of standard deviations and one weight per feature array")
        dev = torch.device("cuda", device)
        self.raw = [torch.as_tensor(np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f, np.float32),
                                    device=dev) for f in raw_features]
        groups = groups if groups is not None else [None] * len(self.raw)
        self.log_sd = torch.nn.ParameterList()
        self._col = []                                        # per term: group of every column
        for f, s, g in zip(self.raw, sd, groups):
            d = int(f.shape[1])
            g = [[c] for c in range(d)] if g is None else [list(x) for x in g]
            if sorted(c for x in g for c in x) != list(range(d)):
                raise ValueError("the groups of a term must partition its %d columns" % d)
            s = np.broadcast_to(np.asarray(s, np.float64), (len(g),))
            col = np.empty(d, np.int64)
            for j, x in enumerate(g):
                col[x] = j
            self._col.append(torch.as_tensor(col, device=dev))
            self.log_sd.append(torch.nn.Parameter(torch.tensor(np.log(s), dtype=torch.float32, device=dev)))
        self.weights = torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))
        self.n_iterations, self.relax, self.device = int(n_iterations), float(relax), int(device)

    def features(self):
        """the features the CRF sees: raw / sd, column by column"""
        return [f * torch.exp(-ls)[col] for f, ls, col in zip(self.raw, self.log_sd, self._col)]

    def sd(self):
        return [torch.exp(ls.detach()).cpu().numpy() for ls in self.log_sd]

    def forward(self, unary):
        return mean_field_features(unary, self.features(), self.weights, self.n_iterations, self.relax, self.device)


class _MeanFieldLearned(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unary, weights, compat, n_iterations, relax, device, *features):
        crf, q, u, fs = _forward_on_own_handle(unary, features, weights, compat, n_iterations, relax, device)
        ctx.crf, ctx.n_iterations, ctx.relax = crf, int(n_iterations), float(relax)
        ctx.weights_device, ctx.compat_device = weights.device, compat.device
        ctx.save_for_backward(u, *fs)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, fs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        crf = ctx.crf
        if crf is None:
            raise RuntimeError("mean_field_learned: backward a second time (the handle is closed by the first)")
        dev, K, L = u.device, len(fs), int(u.shape[1])
        g = _grad_in(grad_q, dev)
        need = ctx.needs_input_grad
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr = _grad_w_buffer(K, dev)
        grad_m = torch.zeros((max(K, 1), L, L), dtype=torch.float32, device=dev)
        grad_f = [torch.empty_like(f) if need[6 + k] else None for k, f in enumerate(fs)]
        with _on_stream(crf.stream(), dev):                   # (the handle still holds this forward's unary, weights and matrices)
            crf.inference_backward_all_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr,
                                              [t.data_ptr() if t is not None else None for t in grad_f], grad_m.data_ptr())
        crf.synchronize()                                     # (the handle goes back to the cache: nothing of this call may be in flight)
        crf.close()
        ctx.crf = None
        return (grad_u, _grad_w_result(grad_w, K, ctx.weights_device), grad_m[:K].to(ctx.compat_device), None, None, None) + tuple(grad_f)


def mean_field_learned(unary, features, weights, compat, n_iterations=5, relax=1.0, device=0):
    """mean_field_features with a label-compatibility matrix per term (include/lccrf.h section 1f): `compat` [K, L, L] (float32,
    any device), term k adding w_k * norm_k * (Phi_k(Q) @ compat[k].T); differentiable in unary, features, weights and compat, all
    four from one reverse sweep.  Every forward builds the lattices afresh on a handle of its own, which its backward closes: one
    backward per forward."""
    return _MeanFieldLearned.apply(unary, weights, compat, n_iterations, relax, device, *features)


class LearnedCRF(LearnedKernelCRF):
    """LearnedKernelCRF whose terms also carry a learnt label-compatibility matrix: parameters log_sd[k], `weights` [K] and `compat`
    [K, n_labels, n_labels], the latter initialised to identities (the Potts model).  sd and groups as LearnedKernelCRF takes them.
    forward(unary [N, n_labels]) -> Q [N, n_labels] through mean_field_learned."""

    def __init__(self, raw_features, sd, weights, groups=None, n_labels=2, n_iterations=5, relax=1.0, device=0):
        super().__init__(raw_features, sd, weights, groups, n_iterations, relax, device)
        self.compat = torch.nn.Parameter(torch.eye(int(n_labels), dtype=torch.float32).repeat(len(weights), 1, 1))

    def forward(self, unary):
        return mean_field_learned(unary, self.features(), self.weights, self.compat, self.n_iterations, self.relax, self.device)


class _MeanFieldCompat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, crf, unary, weights, compat, n_iterations, relax):
        K = len(crf._d)
        _check_unary_weights(unary, (crf.N, crf.L), weights, K)
        if compat.dtype != torch.float32 or tuple(compat.shape) != (K, crf.L, crf.L):
            raise ValueError("compat must be a float32 tensor of shape [%d, %d, %d]" % (K, crf.L, crf.L))
        _check_iterations(n_iterations)
        u = unary.detach().contiguous()
        w, m = weights.detach().clone(), compat.detach().clone().contiguous()
        with _on_stream(crf.stream(), u.device) as (ext, cur):
            _arm(crf, w, m)
            crf.set_unary_device(u.data_ptr())
            q = _forward_q(crf, u, n_iterations, relax, ext, cur)
        ctx.crf, ctx.n_iterations, ctx.relax = crf, int(n_iterations), float(relax)
        ctx.weights_device, ctx.compat_device = weights.device, compat.device
        ctx.save_for_backward(u, w, m)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, w, m = ctx.saved_tensors
        crf, dev = ctx.crf, u.device
        g = _grad_in(grad_q, dev)
        K, L = int(w.numel()), crf.L
        grad_u = torch.empty_like(u)
        grad_w, grad_w_ptr = _grad_w_buffer(K, dev)
        grad_m = torch.zeros((max(K, 1), L, L), dtype=torch.float32, device=dev)
        with _on_stream(crf.stream(), dev):
            _arm(crf, w, m)                                   # the inputs of this forward (the handle may have run others since)
            crf.set_unary_device(u.data_ptr())
            crf.inference_backward_compat_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(), grad_w_ptr,
                                                 grad_m.data_ptr())
        return None, grad_u, _grad_w_result(grad_w, K, ctx.weights_device), grad_m[:K].to(ctx.compat_device), None, None


def mean_field_compat(crf, unary, weights, compat, n_iterations=5, relax=1.0):
    """mean_field with a label-compatibility matrix per term (include/lccrf.h section 1e): `compat` [K, L, L] (float32, any
    device), term k adding w_k * norm_k * (Phi_k(Q) @ compat[k].T); differentiable in unary, weights and compat.  The matrices
    are left set on `crf`."""
    return _MeanFieldCompat.apply(crf, unary, weights, compat, n_iterations, relax)


class CompatMeanFieldCRF(_HandleCRF):
    """MeanFieldCRF whose terms carry a learnt label-compatibility matrix: parameters `weights` [K] and `compat` [K, L, L], the
    latter initialised to identities (the Potts model); normalization as MeanFieldCRF takes it.  forward(unary [N, L]) -> Q [N, L]."""

    def __init__(self, n_points, n_labels, features, weights, n_iterations=5, relax=1.0, device=0, normalization=None):
        super().__init__(n_points, n_labels, features, weights, n_iterations, relax, device, normalization)
        self.compat = torch.nn.Parameter(torch.eye(n_labels, dtype=torch.float32).repeat(len(weights), 1, 1))

    def forward(self, unary):
        return mean_field_compat(self.crf, unary, self.weights, self.compat, self.n_iterations, self.relax)

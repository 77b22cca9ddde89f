"""torch autograd through DenseCRF::inference on the HIP path (include/lccrf.h section 1c).

    Q = mean_field(crf, unary, weights, n_iterations=5, relax=1.0)
    Q.backward(g)      # -> unary.grad = dL/dU, weights.grad = dL/dw

`crf` is a DenseCRFHIP whose pairwise terms are already added (their features fix the lattices; only the weights are
inputs here).  Forward: lccrf_set_pairwise_weight + lccrf_set_unary_device + lccrf_inference.  Backward:
lccrf_inference_backward, which replays the forward itself, so nothing but the inputs is kept between the two.

Streams (the pattern of section 1b): on entry the handle's stream waits for torch's current stream (the inputs and the
incoming gradient are produced there); on exit torch's current stream waits for the handle's stream.  inference()
results are complete behind lccrf_synchronize, so the forward synchronises the handle before it copies Q out.
"""
import importlib

import numpy as np
import torch

_pkg = importlib.import_module("lc-crf-slam_amd")


def _device_view(ptr, shape, device):
    """A tensor over handle-owned device memory (no copy)."""
    class _View:
        __cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f4", data=(int(ptr), False), version=2)
    return torch.as_tensor(_View(), device=device)


def _handle_stream(crf, device):
    return torch.cuda.ExternalStream(crf.stream(), device=device)


class _MeanField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, crf, unary, weights, n_iterations, relax):
        if not unary.is_cuda or unary.dtype != torch.float32 or tuple(unary.shape) != (crf.N, crf.L):
            raise ValueError("unary must be a float32 GPU tensor of shape [%d, %d]" % (crf.N, crf.L))
        K = len(crf._d)
        if weights.dtype != torch.float32 or tuple(weights.shape) != (K,):
            raise ValueError("weights must be a float32 tensor of shape [%d]" % K)
        if n_iterations < 0:
            raise ValueError("n_iterations must be >= 0")
        dev = unary.device
        u = unary.detach().contiguous()
        for k, w in enumerate(weights.detach().cpu().tolist()):
            crf.set_pairwise_weight(k, w)
        cur = torch.cuda.current_stream(dev)
        ext = _handle_stream(crf, dev)
        ext.wait_stream(cur)
        crf.set_unary_device(u.data_ptr())
        crf.inference(int(n_iterations), False, float(relax))
        crf.synchronize()                                     # the completion rule of inference() results
        with torch.cuda.stream(ext):
            q = _device_view(crf.device_buffers()["current"], (crf.N, crf.L), dev).clone()
        cur.wait_stream(ext)
        q.record_stream(cur)
        ctx.crf, ctx.n_iterations, ctx.relax = crf, int(n_iterations), float(relax)
        ctx.weights_device = weights.device
        ctx.save_for_backward(u, weights.detach().clone())
        return q

    @staticmethod
    def backward(ctx, grad_q):
        u, w = ctx.saved_tensors
        crf = ctx.crf
        dev = u.device
        g = grad_q.detach().to(device=dev, dtype=torch.float32).contiguous()
        cur = torch.cuda.current_stream(dev)
        K = int(w.numel())
        # the handle is re-armed with the inputs of this forward (it may have run other inputs since)
        for k, wk in enumerate(w.cpu().tolist()):
            crf.set_pairwise_weight(k, wk)
        grad_u = torch.empty_like(u)
        grad_w = torch.empty(max(K, 1), dtype=torch.float32, device=dev)
        ext = _handle_stream(crf, dev)
        ext.wait_stream(cur)
        crf.set_unary_device(u.data_ptr())
        crf.inference_backward_device(ctx.n_iterations, ctx.relax, g.data_ptr(), grad_u.data_ptr(),
                                      grad_w.data_ptr() if K else None)
        cur.wait_stream(ext)
        if K == 0:
            grad_w = torch.zeros(0, dtype=torch.float32, device=dev)
        return None, grad_u, grad_w[:K].to(ctx.weights_device), None, None


def mean_field(crf, unary, weights, n_iterations=5, relax=1.0):
    """Q_T of DenseCRF::inference(n_iterations, relax) with unary energies `unary` [N, L] (float32, GPU) and pairwise
    weights `weights` [K] (float32, any device) on the terms of `crf`; differentiable in both."""
    return _MeanField.apply(crf, unary, weights, n_iterations, relax)


class MeanFieldCRF(torch.nn.Module):
    """A dense CRF layer: a DenseCRFHIP handle over fixed features, its term weights an nn.Parameter.

    features: list of [N, d_k] arrays (already divided by the kernel's standard deviation, as lccrf_add_pairwise takes
    them); weights: their initial weights.  forward(unary [N, L]) -> Q [N, L]."""

    def __init__(self, n_points, n_labels, features, weights, n_iterations=5, relax=1.0, device=0):
        super().__init__()
        if len(features) != len(weights):
            raise ValueError("one weight per feature array")
        self.crf = _pkg.DenseCRFHIP(n_points, n_labels, device=device)
        for f, w in zip(features, weights):
            f = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
            self.crf.add_pairwise(np.ascontiguousarray(f, np.float32), float(w))
        self.weights = torch.nn.Parameter(torch.tensor([float(w) for w in weights], dtype=torch.float32))
        self.n_iterations, self.relax = int(n_iterations), float(relax)

    def forward(self, unary):
        return mean_field(self.crf, unary, self.weights, self.n_iterations, self.relax)

    def close(self):
        self.crf.close()

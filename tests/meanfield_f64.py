"""Float64 restatement of DenseCRF::inference (densecrf_base.h:65-91) in torch, for the gradient tests.

Built from the oracle's lattices (pyoracle.OracleCRF.kernel(k): offset, bary, nbr, norm), with exact exp: torch autograd
through it gives the reference gradients that lccrf_inference_backward (include/lccrf.h section 1c) is checked against.
Not product code."""
import numpy as np
import torch

D = torch.float64


class Lattice:
    """One term's filter Phi = alpha S^T B_d .. B_0 S on N points (permutohedral_cpu.h:634-699), and its transpose."""

    def __init__(self, kern):
        self.d = int(kern["d"])
        self.V = int(kern["V"])
        self.offset = torch.as_tensor(np.asarray(kern["offset"], np.int64)) + 1       # vertex id + 1: row 0 is "absent"
        self.bary = torch.as_tensor(np.asarray(kern["bary"], np.float64))
        nbr = torch.as_tensor(np.asarray(kern["nbr"], np.int64)) + 1
        self.n1, self.n2 = nbr[..., 0], nbr[..., 1]                                   # [d+1][V]
        self.norm = torch.as_tensor(np.asarray(kern["norm"], np.float64))
        self.alpha = 1.0 / (1.0 + 2.0 ** (-self.d))

    def apply(self, x, reverse=False):
        return self.filter(x, self.bary, reverse)

    def filter(self, x, bary, reverse=False):
        """Phi x with the barycentric weights `bary` (reverse: Phi^T x).  apply() is the one door the forward goes through, so a
        test may swap it for a filter with a planted fault (tests/grad_support.py: planted)."""
        N, L = x.shape
        D1 = self.d + 1
        bary = bary.to(x.dtype)
        contrib = (bary[:, :, None] * x[:, None, :]).reshape(N * D1, L)
        val = torch.zeros(self.V + 1, L, dtype=x.dtype).index_add(0, self.offset.reshape(-1), contrib)
        for j in (reversed(range(D1)) if reverse else range(D1)):
            blurred = val[1:] + 0.5 * (val[self.n1[j]] + val[self.n2[j]])
            val = torch.cat([val[:1] * 0, blurred], 0)
        return ((bary * self.alpha)[:, :, None] * val[self.offset]).sum(1)


def lattices(crf, K):
    return [Lattice(crf.kernel(k)) for k in range(K)]


def pinned(Q, at, t):
    """Q_t with the VALUE at[t] and its own derivative: with at = [Q_0 .. Q_T] the float32 iterates of the oracle's step path (the
    device's bits), autograd differentiates the iteration linearised where the device evaluates it, and the float64 and float32
    checkers no longer drift apart along the forward trajectory (they still differ by the backward's own amplification)"""
    return Q if at is None else Q + (torch.as_tensor(np.asarray(at[t], np.float64)).to(Q.dtype) - Q).detach()


def forward(U, w, lats, n_iterations, relax=1.0, at=None):
    """Q_T for unary U [N, L] and weights w [K] (float64 tensors); at: see pinned()."""
    Q = pinned(torch.softmax(-U, 1), at, 0)
    for t in range(n_iterations):
        x = -U
        for k, lat in enumerate(lats):
            x = x + w[k] * lat.norm.to(U.dtype)[:, None] * lat.apply(Q)
        P = torch.softmax(x, 1)
        Q = pinned(P if relax == 1.0 else (1.0 - relax) * Q + relax * P, at, t + 1)
    return Q


def gradients(U, w, lats, n_iterations, relax, G, dtype=D, at=None):
    """(dL/dU, dL/dw) of L = <G, Q_T>, as float64 numpy arrays.  dtype=torch.float32 runs the same computation in single
    precision: how far THAT lands from the float64 result is what fp32 arithmetic alone costs on a case."""
    U = torch.as_tensor(np.asarray(U, np.float64)).to(dtype).clone().requires_grad_(True)
    w = torch.as_tensor(np.asarray(w, np.float64)).to(dtype).clone().requires_grad_(True)
    Q = forward(U, w, lats, n_iterations, relax, at)
    (Q * torch.as_tensor(np.asarray(G, np.float64)).to(dtype)).sum().backward()
    return (U.grad.double().numpy(), w.grad.double().numpy() if w.grad is not None else np.zeros(len(lats)))

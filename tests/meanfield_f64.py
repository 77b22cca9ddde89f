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
        N, L = x.shape
        D1 = self.d + 1
        bary = self.bary.to(x.dtype)
        contrib = (bary[:, :, None] * x[:, None, :]).reshape(N * D1, L)
        val = torch.zeros(self.V + 1, L, dtype=x.dtype).index_add(0, self.offset.reshape(-1), contrib)
        for j in (reversed(range(D1)) if reverse else range(D1)):
            blurred = val[1:] + 0.5 * (val[self.n1[j]] + val[self.n2[j]])
            val = torch.cat([val[:1] * 0, blurred], 0)
        return ((bary * self.alpha)[:, :, None] * val[self.offset]).sum(1)


def lattices(crf, K):
    return [Lattice(crf.kernel(k)) for k in range(K)]


def forward(U, w, lats, n_iterations, relax=1.0):
    """Q_T for unary U [N, L] and weights w [K] (float64 tensors)."""
    Q = torch.softmax(-U, 1)
    for _ in range(n_iterations):
        x = -U
        for k, lat in enumerate(lats):
            x = x + w[k] * lat.norm.to(U.dtype)[:, None] * lat.apply(Q)
        P = torch.softmax(x, 1)
        Q = P if relax == 1.0 else (1.0 - relax) * Q + relax * P
    return Q


def gradients(U, w, lats, n_iterations, relax, G, dtype=D):
    """(dL/dU, dL/dw) of L = <G, Q_T>, as float64 numpy arrays.  dtype=torch.float32 runs the same computation in single
    precision: how far THAT lands from the float64 result is what fp32 arithmetic alone costs on a case."""
    U = torch.as_tensor(np.asarray(U, np.float64)).to(dtype).clone().requires_grad_(True)
    w = torch.as_tensor(np.asarray(w, np.float64)).to(dtype).clone().requires_grad_(True)
    Q = forward(U, w, lats, n_iterations, relax)
    (Q * torch.as_tensor(np.asarray(G, np.float64)).to(dtype)).sum().backward()
    return (U.grad.double().numpy(), w.grad.double().numpy() if w.grad is not None else np.zeros(len(lats)))

"""Restatements of mean-field inference with label-compatibility matrices (include/lccrf.h section 1e), for the tests.

restate_f32: the float32 arithmetic contract, built from the oracle only -- the lattice filter, the norm and the softmax are the
oracle's own; the matrix sum is numpy float32 with one rounding per operation.  forward_f64 / gradients_f64: tests/meanfield_f64.py's
forward with x + w[k] * norm * (Phi_k(Q) @ mu[k].T), for the gradients.  Not product code."""
import numpy as np
import torch

import meanfield_f64 as mf

F32 = np.float32


def _po():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _softmax_oracle(x):
    """expAndNormalize(x) as the oracle forms it: a term-less CRF whose unary is -x (scale -1 on -x is exact)"""
    N, L = x.shape
    o = _po().OracleCRF(N, L)
    o.set_unary(-x)
    o.start_inference()
    p = o.probability()
    o.close()
    return p


def compat_sum_f32(mu, t):
    """s[i][l] = 0; for l' = 0 .. L-1: s = s + mu[l][l'] * t[i][l'] -- every product and every sum rounded to float32"""
    mu, t = np.asarray(mu, F32), np.asarray(t, F32)
    s = np.zeros_like(t)
    for lp in range(t.shape[1]):
        s = (s + (mu[None, :, lp] * t[:, lp, None]).astype(F32)).astype(F32)
    return s


def term_f32(base, feat, w, norm, mu, Q):
    """base + w * norm * (mu applied to the oracle's Phi(Q)), the expression shape of the slice kernels"""
    t, _ = _po().oracle_lattice_filter(feat, Q)
    s = t if mu is None else compat_sum_f32(mu, t)
    wn = (F32(w) * np.asarray(norm, F32)).astype(F32)
    return (base + (wn[:, None] * s).astype(F32)).astype(F32)


def norms(N, L, features):
    o = _po().OracleCRF(N, L)
    o.set_unary(np.zeros((N, L), F32))
    for f in features:
        o.add_pairwise(f, 1.0)
    out = [o.kernel(k)["norm"] for k in range(len(features))]
    o.close()
    return out


def restate_f32(U, features, weights, compats, T, relax):
    """Q_T [N][L] float32.  compats: per term an [L][L] matrix or None (Potts)."""
    U = np.ascontiguousarray(U, F32)
    N, L = U.shape
    nrm = norms(N, L, features)
    Q = _softmax_oracle((-U).astype(F32))
    r = F32(relax)
    for _ in range(T):
        x = (-U).astype(F32)
        for f, w, n, mu in zip(features, weights, nrm, compats):
            x = term_f32(x, f, w, n, mu, Q)
        P = _softmax_oracle(x)
        Q = P if relax == 1.0 else (((F32(1.0) - r) * Q).astype(F32) + (r * P).astype(F32)).astype(F32)
    return Q


def map_of(Q):
    """buildMap (densecrf3d.h:136-151): the first largest label"""
    return np.argmax(Q, 1).astype(np.int16)


def compat_product(t, m):
    """mu applied to the filter's output: out[i][l] = sum_l' m[l][l'] t[i][l'].  The one door the float64 forwards go through, so
    a test may swap it for a product with a planted fault (tests/grad_support.py: planted)."""
    return t @ m.T


def forward_f64(U, w, mu, lats, n_iterations, relax=1.0, at=None):
    """Q_T for unary U [N, L], weights w [K] and matrices mu [K, L, L] (tensors of one dtype); at: meanfield_f64.pinned"""
    Q = mf.pinned(torch.softmax(-U, 1), at, 0)
    for t in range(n_iterations):
        x = -U
        for k, lat in enumerate(lats):
            x = x + w[k] * lat.norm.to(U.dtype)[:, None] * compat_product(lat.apply(Q), mu[k])
        P = torch.softmax(x, 1)
        Q = mf.pinned(P if relax == 1.0 else (1.0 - relax) * Q + relax * P, at, t + 1)
    return Q


def gradients_f64(U, w, mu, lats, n_iterations, relax, G, dtype=mf.D, at=None):
    """(dL/dU, dL/dw, dL/dmu) of L = <G, Q_T> as float64 numpy arrays; dtype=torch.float32: the same computation in single precision"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype).clone().requires_grad_(True)
    U, w, mu = t(U), t(w), t(mu)
    Q = forward_f64(U, w, mu, lats, n_iterations, relax, at)
    (Q * torch.as_tensor(np.asarray(G, np.float64)).to(dtype)).sum().backward()
    z = lambda x, like: x.grad.double().numpy() if x.grad is not None else np.zeros(tuple(like.shape))
    return z(U, U), z(w, w), z(mu, mu)

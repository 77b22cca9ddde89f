"""The checker of lccrf_inference_backward_modes (include/lccrf.h sections 1m and 2i) and what its tests share.

The reference is tests/normalization_checker.py's forward_f64 run over tests/meanfield_f64_features.py's FeatureLattice lattices bound
to feature tensors that require gradients.  lat.norm is then a function of the features, so normalization_checker.factors_f64 -- n,
sqrt(n) -- is differentiated with everything else: torch autograd gives (dL/dU, dL/dw, dL/dmu, [dL/df_k]) in float64 and, with
dtype=torch.float32, in single precision.  Every output is held to grad_support.bar_of's rule (grad_support.Reference).

sweep_f64 restates the reverse sweep as section 1m writes it, float64, no autograd, in the manner of
meanfield_f64_features.sweep_feature_gradients.  held("n") / held("pre") plant the two faults a wrong sweep would most likely have: the
norm's factors, or the factor in front of the filter alone, treated as constants.  Not product code."""
import importlib

import numpy as np
import torch

import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import joint_checker as jc
import meanfield_f64_features as mff
import normalization_checker as nc
from abi_support import dev

pkg = importlib.import_module("lc-crf-slam_amd")
D = torch.float64
NAMES = ("dL/dU", "dL/dw", "dL/dmu")


# ---- the autograd reference -------------------------------------------------------------------------------------------------
def mode_gradients(U, w, mu, lats, modes, n_iterations, relax, G, dtype=D, at=None):
    """(dL/dU, dL/dw, dL/dmu, [dL/df_k]) of L = <G, Q_T>, float64 numpy arrays; the topology fixed, the factors of every mode
    functions of the features through the lattices' norm.  dtype=torch.float32: the same computation in single precision."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype).clone().requires_grad_(True)
    U, w, mu = t(U), t(w), t(mu)
    fs = [t(lat.feat32) for lat in lats]
    for lat, f in zip(lats, fs):
        lat.bind(f)
    Q = nc.forward_f64(U, w, mu, lats, modes, n_iterations, relax, at)
    (Q * torch.as_tensor(np.asarray(G, np.float64)).to(dtype)).sum().backward()
    for lat in lats:                                             # leave the lattices bound to plain float64 features
        lat.bind(torch.as_tensor(lat.feat32.astype(np.float64)))
    z = lambda x: x.grad.double().numpy() if x.grad is not None else np.zeros(tuple(x.shape))
    return z(U), z(w), z(mu), [z(f) for f in fs]


class held:
    """with held("n"): normalization_checker.factors_f64 hands out both factors as constants (n is not differentiated: what the
    sweep of section 1f would give if it were let through); with held("pre"): the factor in front of the filter alone"""

    def __init__(self, what):
        assert what in ("n", "pre"), what
        self.what = what

    def __enter__(self):
        self.saved, what = nc.factors_f64, self.what

        def factors(lat, mode, dtype):
            a, b = self.saved(lat, mode, dtype)
            return (a.detach() if a is not None and what == "n" else a), (b.detach() if b is not None else b)
        nc.factors_f64 = factors

    def __exit__(self, *exc):
        nc.factors_f64 = self.saved


def mode_reference(U, w, mu, lats, modes, T, relax, G, name="", at=None):
    """lccrf_inference_backward_modes' outputs against mode_gradients: the floors of sections 1e (dL/dU, dL/dw, dL/dmu) and 1d (dL/df)"""
    fl_u, fl_w = gs.floors_of(G, w)
    floors = {"dL/dU": fl_u, "dL/dw": fl_w, "dL/dmu": fl_w}
    floors.update(("dL/df%d" % k, fl_u) for k in range(len(lats)))

    def grads(dtype):
        g = mode_gradients(U, w, mu, lats, modes, T, relax, G, dtype=dtype, at=at)
        return gs._named(g[:3], g[3])
    return gs.Reference("%s T=%d relax=%g" % (name, T, relax), grads, floors)


# ---- section 1m's sweep, restated without autograd ----------------------------------------------------------------------------
def sweep_f64(U, w, mu, lats, modes, n_iterations, relax, G, at=None):
    """(dL/dU, dL/dw, dL/dmu, [dL/df_k]) by the reverse sweep of include/lccrf.h section 1m, float64.  at: the pinned iterates
    (meanfield_f64.pinned: the values the filters see are at[t], the softmax is differentiated where it is evaluated)."""
    with torch.no_grad():
        U = torch.as_tensor(np.asarray(U, np.float64))
        w = [float(x) for x in np.asarray(w, np.float64)]
        mu = torch.as_tensor(np.asarray(mu, np.float64))
        Gt = torch.as_tensor(np.asarray(G, np.float64)).clone()
        T, K = n_iterations, len(lats)
        fac = [nc.factors_f64(lat, m, D) for lat, m in zip(lats, modes)]           # (a_k, b_k), None = 1
        one = lambda v: 1.0 if v is None else v[:, None]
        pin = lambda Q, t: Q if at is None else torch.as_tensor(np.asarray(at[t], np.float64))

        def x_of(Q):
            x, parts = -U, []
            for k, lat in enumerate(lats):
                a, b = fac[k]
                xin = one(b) * Q
                res = lat.values(xin)                                               # (B S x)
                phi = lat.alpha * (lat.bary[:, :, None] * res[lat.offset]).sum(1)
                m = phi @ mu[k].T
                x = x + w[k] * one(a) * m
                parts.append((xin, res, phi, m))
            return x, parts
        hist = [pin(torch.softmax(-U, 1), 0)]
        for t in range(T):
            Q = hist[-1]
            P = torch.softmax(x_of(Q)[0], 1)
            hist.append(pin(P if relax == 1.0 else (1.0 - relax) * Q + relax * P, t + 1))
        gU, gw, gmu = torch.zeros_like(U), torch.zeros(K, dtype=D), torch.zeros_like(mu)
        gb = [torch.zeros(U.shape[0], lat.d + 1, dtype=D) for lat in lats]
        gn = [torch.zeros(U.shape[0], dtype=D) for lat in lats]                     # the ONE accumulator of g_post and g_pre
        for t in range(T, 0, -1):
            Q = hist[t - 1]
            x, parts = x_of(Q)
            P = torch.softmax(x, 1)
            gamma = relax * P * (Gt - (Gt * P).sum(1, keepdim=True))
            gU -= gamma
            Gt = (1.0 - relax) * Gt
            for k, lat in enumerate(lats):
                a, b = fac[k]
                xin, res, phi, m = parts[k]
                gw[k] += (gamma * one(a) * m).sum()
                gmu[k] += w[k] * (one(a) * gamma).T @ phi
                y = one(a) * (gamma @ mu[k])                                        # a_k (mu_k^T gamma_t)
                if a is not None:
                    gn[k] += w[k] * (gamma * m).sum(1)                               # post adjoint
                gb[k] += lat.alpha * w[k] * (y[:, None, :] * res[lat.offset]).sum(2)            # slice side
                rt = lat.values(y, reverse=True)
                gb[k] += lat.alpha * w[k] * (xin[:, None, :] * rt[lat.offset]).sum(2)           # splat side: the row is b_k Q
                zt = lat.alpha * (lat.bary[:, :, None] * rt[lat.offset]).sum(1)
                if b is not None:
                    gn[k] += w[k] * (Q * zt).sum(1)                                  # pre adjoint, before z is scaled by b_k
                Gt = Gt + w[k] * one(b) * zt
        P0 = torch.softmax(-U, 1)
        gU -= P0 * (Gt - (Gt * P0).sum(1, keepdim=True))
        out = []
        for k, lat in enumerate(lats):
            if modes[k] != nc.NONE:
                g_n = gn[k] * (0.5 / torch.sqrt(lat.norm)) if modes[k] == nc.SYMMETRIC else gn[k]
                a = (-lat.norm * lat.norm * g_n)[:, None]
                gb[k] += lat.alpha * (a * lat.values(torch.ones_like(a))[lat.offset][:, :, 0])
                gb[k] += lat.alpha * lat.values(a, reverse=True)[lat.offset][:, :, 0]
            out.append(mff.corner_to_feature(gb[k].numpy(), lat.scale, lat.rank))
        return gU.numpy(), gw.numpy(), gmu.numpy(), out


# ---- the settings of the GPU tests (and of the CPU test of their bars) ---------------------------------------------------------------
CASES = ["slam1001:s38", "d1_L3:s3", "L21:d3_d5"]               # normalization_checker.case
ONE_MODE = [nc.BEFORE, nc.SYMMETRIC, nc.NONE]
MIXED = [[nc.SYMMETRIC, nc.BEFORE], [nc.NONE, nc.SYMMETRIC]]     # on slam1001:s38
T_SET, RELAX_SET, KINDS = (0, 1, 5), (1.0, 0.7), ("dense", "potts")
SETTINGS = [(n, (m,), T, r, kind) for n in CASES for m in ONE_MODE for T in T_SET for r in RELAX_SET for kind in KINDS] + \
           [("slam1001:s38", tuple(ms), T, r, kind) for ms in MIXED for T in T_SET for r in RELAX_SET for kind in KINDS]


def setting_id(s):
    n, ms, T, r, kind = s
    return "%s-%s-T%d-r%g-%s" % (n, "+".join(nc.MODE_NAMES[m] for m in ms), T, r, kind)


_REFS = {}


def reference_for(po, wl, golden, name, ms, T, relax, kind):
    """What a setting is checked against, computed once and shared (leave it unchanged): the problem, the modes, the float32 weights
    (normalization_checker.weights_f32), the matrices handed to the handle (kind "dense": joint_checker.dense on every term and
    d_grad_compat asked for; "potts": none), G and the grad_support.Reference of mode_gradients.  slam1001:s38 and L21:d3_d5 are
    linearised at the device's iterates from T = 1 on (gradient_settings.LINEARISED)."""
    key = (name, tuple(ms), T, relax, kind)
    if key not in _REFS:
        pb, U32, nrm = gset.norm_prepared(name, golden, po, wl)
        K, L = len(pb["kernels"]), pb["L"]
        modes = list(ms) * K if len(ms) == 1 else list(ms)
        mats = jc.dense(K, L) if kind == "dense" else [None] * K
        w = nc.weights_f32(pb, nrm, modes)
        o, lats, U = jc.checker(po, pb)
        o.close()
        G = gset.grad_prob(pb)
        at = None
        if gset.linearised("modes", name, T, relax):
            at = gset.device_iterates(po, pb, T, relax, mats if kind == "dense" else None, modes, w, nrm)
        w64 = np.array([float(x) for x in w])
        tag = "%s %s %s" % (name, "+".join(nc.MODE_NAMES[m] for m in modes), kind)
        ref = mode_reference(U, w64, jc.checker_mu(mats, L), lats, modes, T, relax, G, tag, at)
        _REFS[key] = dict(pb=pb, modes=modes, mats=mats, w=w, w64=w64, G=G, U=U, lats=lats, at=at, ref=ref,
                          dims=[lat.d for lat in lats], dense=kind == "dense")
    return _REFS[key]


# ---- the device --------------------------------------------------------------------------------------------------------------
def handle(pb, weights, modes, mats=None):
    """a GPU handle of the problem with the given weights, modes and matrices (None entries: Potts terms)"""
    h = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, w) for (f, _), w in zip(pb["kernels"], weights)]))
    for k, m in enumerate(modes):
        h.set_normalization(k, m)
    for k, m in enumerate(mats or []):
        if m is not None:
            h.set_pairwise_compatibility(k, m)
    return h


def backward(h, dims, L, T, relax, G, skip=(), unary=True, weights=True, compat=True, features=True, entry="modes"):
    """(dL/dU, dL/dw, dL/dmu, [dL/df_k or None]) from lccrf_inference_backward_modes (entry="all": lccrf_inference_backward_all);
    every output pre-filled with NaN.  An output that is not asked for comes back as filled."""
    K, N = len(dims), G.shape[0]
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    gm = torch.full((max(K, 1), L, L), float("nan"), device="cuda")
    gf = [None if k in skip else torch.full((N, d), float("nan"), device="cuda") for k, d in enumerate(dims)]
    torch.cuda.synchronize()
    call = h.inference_backward_modes_device if entry == "modes" else h.inference_backward_all_device
    call(T, relax, g.data_ptr(), gu.data_ptr() if unary else None, gw.data_ptr() if K and weights else None,
         [t.data_ptr() if t is not None else None for t in gf] if features else None, gm.data_ptr() if compat else None)
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy(), gm[:K].cpu().numpy(), [t.cpu().numpy() if t is not None else None for t in gf]


def batch_backward(b, fr, T, relax, G, features=True, compat=True, model=True, entry="modes"):
    """dict(gu, gw, gf, gm, model) of lccrf_batch_inference_backward_modes (entry="all": .._all), every output pre-filled with NaN"""
    F, K, L = len(fr.N), fr.K, fr.L
    g = dev(np.ascontiguousarray(G[:F], np.float32))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    gu, gw, gm, md = nan(F, fr.maxN, L), nan(F, max(K, 1)), nan(F, max(K, 1), L, L), nan(max(K, 1) * (1 + L * L))
    gf = [nan(F, fr.maxN, d) for d in fr.dims]
    torch.cuda.synchronize()
    call = b.inference_backward_modes_device if entry == "modes" else b.inference_backward_all_device
    call(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [t.data_ptr() for t in gf] if features else None,
         gm.data_ptr() if compat else None, md.data_ptr() if model else None)
    b.synchronize()
    torch.cuda.synchronize()
    return dict(gu=gu.cpu().numpy(), gw=gw[:, :K].cpu().numpy(), gm=gm[:, :K].cpu().numpy(), gf=[t.cpu().numpy() for t in gf],
                model=md[:K * (1 + L * L)].cpu().numpy())

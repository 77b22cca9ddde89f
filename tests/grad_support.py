"""What the gradient tests share (include/lccrf.h sections 1c - 1e, 2c, 2d): the float64 checker set up on a problem, a GPU handle
of that problem, the backward calls with their outputs pre-filled with NaN, and the bar the gradients are held to."""
import importlib

import numpy as np

import crf_cases as cc
import meanfield_f64 as mf
from abi_support import dev

pkg = importlib.import_module("lc-crf-slam_amd")
GRAD_TOL = 1e-4


def weights(pb):
    return np.array([float(w) for _, w in pb["kernels"]], np.float64)


def checker(po, pb):
    """(oracle CRF, its lattices, U as float64)"""
    o = cc.setup(po.OracleCRF, pb)
    return o, mf.lattices(o, len(pb["kernels"])), o.unary().astype(np.float64)


def gpu_handle(pb, image=None):
    import torch
    if image is None:
        return cc.setup(pkg.DenseCRFHIP, pb), []
    W, H, im = image
    d_lab, d_img = dev(pb["label"]), dev(im)
    torch.cuda.synchronize()
    h = pkg.DenseCRFHIP(pb["N"], pb["L"])
    h.set_unary_from_label_device(d_lab.data_ptr(), pb["conf"])
    h.add_image_kernel(W, H, 3.0, 3.0)
    h.add_image_kernel(W, H, 10.0, 60.0, d_img.data_ptr(), pkg.IMAGE_U8, 20.0)
    return h, [d_lab, d_img]


def backward(h, T, relax, G, K):
    import torch
    g = dev(G.astype(np.float32))
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((max(K, 1),), float("nan"), device="cuda")
    torch.cuda.synchronize()
    h.inference_backward_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr() if K else None)
    h.synchronize()
    return gu.cpu().numpy(), gw[:K].cpu().numpy()


def batch_backward(b, T, relax, G, K, stream=None):
    import torch
    g = dev(G)
    gu = torch.full(G.shape, float("nan"), device="cuda")
    gw = torch.full((G.shape[0], max(K, 1)), float("nan"), device="cuda")
    torch.cuda.synchronize()
    b.inference_backward_device(T, relax, g.data_ptr(), gu.data_ptr(), gw.data_ptr() if K else None, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    return gu.cpu().numpy(), gw[:, :K].cpu().numpy()


def rel(a, b, floor=0.0):
    """relative L2 error; gradients smaller than `floor` are compared in absolute terms against it"""
    nb = max(np.linalg.norm(b), floor)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


BAR_CAP = 1e-2                                                   # a bar beyond it checks nothing (notes/normalization.md section 4)


def worst_row(a, b, floor=0.0):
    """(max_i |a_i - b_i|_2 / (|b|_F / sqrt(N)), i): the worst row of a per-point array [N][.] on the scale of the reference's
    root-mean-square row norm; the floor enters as in rel()"""
    N = b.shape[0]
    if N == 0:
        return 0.0, 0
    nb = max(np.linalg.norm(b), floor)
    d = np.linalg.norm((np.asarray(a, np.float64) - b).reshape(N, -1), axis=1)
    i = int(np.argmax(d))
    return float(d[i]) * np.sqrt(N) / (nb if nb > 0 else 1.0), i


def bar_of(f32_error):
    """THE bar of every gradient test: max(GRAD_TOL, 10 x the float32 checker's own value of the same metric)"""
    return max(GRAD_TOL, 10 * f32_error)


def bars(ref, f32, floor=0.0, rows=False):
    """(L2 bar, row bar or None, the float32 checker's L2 error, its row value or None) of one output, from the checkers alone"""
    f = rel(f32, ref, floor)
    fr = worst_row(f32, ref, floor)[0] if rows else None
    return bar_of(f), (bar_of(fr) if rows else None), f, fr


def assert_within_bar(what, got, ref, f32, floor=0.0, rows=False):
    """One output `got` of the device against the float64 checker's `ref`, `f32` being the same checker run in float32: relative L2
    error <= bar_of(the float32 checker's); with rows=True (per-point outputs [N][.]: dL/dU, dL/df_k) also the worst row on the
    scale of the reference's rms row norm <= bar_of(the float32 checker's worst row).  A bar beyond BAR_CAP checks nothing: that is
    an error of the test's case, asserted first.  Prints the figures; returns (L2 error, L2 bar, row error or None, row bar or None)."""
    bar, rbar, f, fr = bars(ref, f32, floor, rows)
    e = rel(got, ref, floor)
    line = "%s: relative L2 error %.3g (bar %.3g, float32 checker %.3g, |ref| %.3g)" % (what, e, bar, f, np.linalg.norm(ref))
    er, i = worst_row(got, ref, floor) if rows else (None, 0)
    if rows:
        line += "; worst row %.3g at row %d of %d (bar %.3g, float32 checker %.3g)" % (er, i, ref.shape[0], rbar, fr)
    print(line)
    assert bar <= BAR_CAP and (rbar is None or rbar <= BAR_CAP), "a bar beyond %g checks nothing -- %s" % (BAR_CAP, line)
    assert e <= bar, line
    assert not rows or er <= rbar, line
    return e, bar, er, rbar


class Reference:
    """What the outputs of one setting are held to.  grads(dtype) runs the setting's checker and returns {output: array}; floors
    {output: floor}; rows the per-point outputs [N][.].  The float64 and float32 runs are made once, here, and left unchanged."""

    def __init__(self, tag, grads, floors, rows=("dL/dU",)):
        import torch
        self.tag, self.grads, self.floors = tag, grads, floors
        self.ref, self.f32 = grads(torch.float64), grads(torch.float32)
        self.rows = {n for n in self.ref if n in rows or n.startswith("dL/df")}

    def bars(self):
        """{output: (L2 bar, row bar or None, float32 checker's L2 error, its row value or None)}"""
        return {n: bars(r, self.f32[n], self.floors[n], n in self.rows) for n, r in self.ref.items()}

    def faulty(self, fault):
        """the float64 checker's outputs with `fault` planted in its backward"""
        import torch
        with planted(fault):
            return self.grads(torch.float64)

    def check(self, got):
        """every output of the device in `got` ({output: array or None}) within its bars"""
        for n, a in got.items():
            if a is not None:
                assert_within_bar("%s %s" % (self.tag, n), a, self.ref[n], self.f32[n], self.floors[n], n in self.rows)


def floors_of(G, w):
    """gradients below 1e-6 of |dL/dQ| (x max(|w|, 1) for dL/dw and dL/dmu) are compared in absolute terms against that floor"""
    fl = 1e-6 * np.linalg.norm(G)
    return fl, fl * max(np.linalg.norm(w), 1.0)


def _named(arrays, feats=None):
    out = dict(zip(("dL/dU", "dL/dw", "dL/dmu"), arrays))
    out.update(("dL/df%d" % k, a) for k, a in enumerate(feats or []))
    return out


def reference(U, w, lats, T, relax, G, name="", at=None):
    """lccrf_inference_backward's outputs (section 1c) against meanfield_f64.gradients"""
    fl_u, fl_w = floors_of(G, w)
    return Reference("%s T=%d relax=%g" % (name, T, relax), lambda dt: _named(mf.gradients(U, w, lats, T, relax, G, dtype=dt, at=at)),
                     {"dL/dU": fl_u, "dL/dw": fl_w})


def feature_reference(U, w, lats, T, relax, G, name="", at=None):
    """dL/df of every term (section 1d) against meanfield_f64_features.feature_gradients over FeatureLattice lattices"""
    import meanfield_f64_features as mff
    fl_u, _ = floors_of(G, w)
    return Reference("%s T=%d relax=%g" % (name, T, relax),
                     lambda dt: _named((), mff.feature_gradients(U, w, lats, T, relax, G, dtype=dt, at=at)[2]),
                     {"dL/df%d" % k: fl_u for k in range(len(lats))})


def compat_reference(U, w, mats, lats, T, relax, G, name="", modes=None, at=None):
    """lccrf_inference_backward_compat's outputs (sections 1e, 1g) against compat_checker.gradients_f64 or, with per-term
    normalisation modes, normalization_checker.gradients_f64"""
    import compat_checker as ck
    import normalization_checker as nc
    mu = np.stack(mats).astype(np.float64)
    fl_u, fl_w = floors_of(G, w)
    if modes is None:
        grads = lambda dt: _named(ck.gradients_f64(U, w, mu, lats, T, relax, G, dtype=dt, at=at))
    else:
        grads = lambda dt: _named(nc.gradients_f64(U, w, mu, lats, modes, T, relax, G, dtype=dt, at=at))
    return Reference("%s T=%d relax=%g" % (name, T, relax), grads, {"dL/dU": fl_u, "dL/dw": fl_w, "dL/dmu": fl_w})


def assert_matches_checker(gu, gw, U, w, lats, T, relax, G, name=""):
    """The bar of test_gradients_match_the_checker (assert_within_bar): dL/dU by its L2 norm and by its worst row, dL/dw by its L2
    norm, gradients below 1e-6 of |dL/dQ| compared in absolute terms against that floor; at T = 0 dL/dw is 0.
    Returns the checker's (dL/dU, dL/dw)."""
    r = reference(U, w, lats, T, relax, G, name)
    r.check({"dL/dU": gu, "dL/dw": gw})
    if T == 0:
        assert np.all(gw == 0)
    return r.ref["dL/dU"], r.ref["dL/dw"]


# ---- planted faults: what a wrong backward would give, from the float64 checker (tests/test_gradient_bars.py) -----------------
def _untransposed_apply(self, x, reverse=False):
    import torch

    class Untransposed(torch.autograd.Function):
        """Phi x whose backward hands Phi g upstream where the sweep needs Phi^T g: the blur passes not reversed.  (The gradient
        with respect to the barycentric weights is left right.)"""
        @staticmethod
        def forward(ctx, x, bary):
            ctx.save_for_backward(x, bary)
            return self.filter(x, bary, reverse)

        @staticmethod
        def backward(ctx, g):
            x, bary = ctx.saved_tensors
            gb = None
            if ctx.needs_input_grad[1]:
                with torch.enable_grad():
                    b = bary.detach().requires_grad_(True)
                    gb, = torch.autograd.grad(self.filter(x.detach(), b, reverse), b, g)
            return self.filter(g, bary.detach(), reverse), gb
    return Untransposed.apply(x, self.bary)


def _untransposed_product(t, m):
    import torch

    class Untransposed(torch.autograd.Function):
        """t mu^T whose backward hands g mu^T upstream where the sweep needs g mu; dL/dmu is left right"""
        @staticmethod
        def forward(ctx, t, m):
            ctx.save_for_backward(t, m)
            return t @ m.T

        @staticmethod
        def backward(ctx, g):
            t, m = ctx.saved_tensors
            return g @ m.T, g.T @ t
    return Untransposed.apply(t, m)


class planted:
    """with planted("filter") / planted("compat"): the float64 checkers differentiate with that fault in their backward"""

    def __init__(self, fault):
        assert fault in ("filter", "compat"), fault
        self.fault = fault

    def __enter__(self):
        import compat_checker as ck
        if self.fault == "filter":
            self.saved = mf.Lattice.apply
            mf.Lattice.apply = _untransposed_apply
        else:
            self.saved = ck.compat_product
            ck.compat_product = _untransposed_product

    def __exit__(self, *exc):
        import compat_checker as ck
        if self.fault == "filter":
            mf.Lattice.apply = self.saved
        else:
            ck.compat_product = self.saved

"""Learnt models -- label-compatibility matrices, normalisation modes -- of three to eight labels in one launch on the fused engine
(csrc/fused_multilabel_general.hip; LCCRF_MULTILABEL_LEARNT of lccrf_set_multilabel_routes, engine 6).

CPU: the instantiation class every case is there for and the models they run under; the setter and getter, declared, exported and
bound, and their refusals of NULL arguments (the refusal of unknown bits needs a live handle, which needs a device: it is in the GPU
test of the two bits); the layers' attribute; the C++ mirror.  GPU: lccrf_inference with the bit on against the float32 restatement
of tests/normalization_checker.py, bit for bit on Q, the labels those of compat_checker.map_of, the engine report 6 with the shape
word the CPU part derived, and the same handle with the bit off on the streaming engine; the two bits' independence; everything beyond
the route, which keeps (1, 0) and the reference's bits; a ragged batch; the torch layers."""
import importlib
import inspect
import os
import subprocess

import numpy as np
import pytest

import abi_support
import compat_checker as ck
import crf_cases as cc
import fused_multilabel_cases as mc
import fused_multilabel_learnt_cases as lc
import normalization_checker as nc
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
POTTS, LEARNT = 1, 2
NAMES = ["lccrf_set_multilabel_routes", "lccrf_get_multilabel_routes", "lccrf_batch_set_multilabel_routes",
         "lccrf_batch_get_multilabel_routes"]


def _same(h, q, tag):
    got = h.probability()
    assert cc.same_bits(got, q), (tag, float(np.abs(got - q).max()))
    assert np.array_equal(h.map(), ck.map_of(q)), tag


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_instantiation_class_it_is_there_for(po, wl):
    seen, models = set(), {}
    for name, (args, want) in lc.CASES.items():
        c = lc.prepared(name, po, wl)
        assert c.cls == want, (name, c.cls, want)
        assert c.pb["N"] <= lc.PLAN[c.pb["L"]], name
        assert any(m != nc.AFTER for m in c.modes) or any(m is not None for m in c.mats), name      # a learnt model on every case
        inst = (c.pb["L"], len(c.pb["kernels"])) + c.cls[:2]
        seen.add(inst)
        models.setdefault(inst, []).append(c)
    # every instantiation of the kernel: (labels, terms, points per lane, row path) over the shipped range
    assert seen == {(L, k, p, ch) for L, n in lc.PLAN.items() for k in (1, 2) for p in range(1, n // lc.LANES + 1) for ch in (0, 1)}, seen
    # ... sees at least one matrix and one factor in front of a filter, every odd L a matrix
    for inst, cs in models.items():
        assert any(m is not None for c in cs for m in c.mats), inst
        assert any(m in (nc.BEFORE, nc.SYMMETRIC) for c in cs for m in c.modes), inst
    # the combinations: a matrix without a mode, a mode without a matrix, both on one term, a matrix on one term and a mode on the other
    kinds = set()
    for c in (lc.prepared(n, po, wl) for n in lc.CASES):
        on = [(m is not None, mode != nc.AFTER) for m, mode in zip(c.mats, c.modes)]
        kinds |= {"matrix alone" if all(not md for _, md in on) else "", "mode alone" if all(not mt for mt, _ in on) else "",
                  "both on one" if any(mt and md for mt, md in on) else "",
                  "one each" if len(on) == 2 and ((on[0] == (True, False) and on[1] == (False, True)) or
                                                  (on[1] == (True, False) and on[0] == (False, True))) else ""}
    assert kinds >= {"matrix alone", "mode alone", "both on one", "one each"}, kinds
    assert {c.cls[2] for c in (lc.prepared(n, po, wl) for n in lc.CASES)} == {0, 1}     # own and shared product buffers
    assert {m for c in (lc.prepared(n, po, wl) for n in lc.CASES) for m in c.modes} == set(nc.MODES)
    m = lc.matrix(3, 0)
    assert m.dtype == np.float32 and not np.array_equal(m, m.T)


def test_the_routes_are_declared_exported_and_bound(lib):
    src = abi_support.assert_declared_exported_bound(lib, NAMES)
    assert "LCCRF_MULTILABEL_POTTS = 1" in src and "LCCRF_MULTILABEL_LEARNT = 2" in src
    assert "#define LCCRF_ABI_VERSION 3" in open(pkg.HEADER_PATH).read() and lib.lccrf_abi_version() == 3
    assert (pkg.MULTILABEL_POTTS, pkg.MULTILABEL_LEARNT) == (1, 2)
    assert (pkg.BatchCRF.MULTILABEL_POTTS, pkg.BatchCRF.MULTILABEL_LEARNT) == (1, 2)
    for cls in (pkg.DenseCRFHIP, pkg.BatchCRF):
        assert callable(cls.set_multilabel_routes) and callable(cls.multilabel_routes)


def test_null_arguments_are_refused(lib):
    import ctypes as C
    r = C.c_uint(77)
    for name in NAMES:
        f = getattr(lib, name)
        assert f(None, 1 if "set" in name else C.byref(r)) == E_INVALID, name
        assert b"NULL" in lib.lccrf_last_error(), name
    assert r.value == 77                                         # nothing written


def test_the_layers_have_the_attribute_and_keep_their_constructors():
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    for layer in (ag.MeanFieldCRF, ag.BatchMeanFieldCRF, ag.CompatMeanFieldCRF, ag.BatchCompatMeanFieldCRF):
        assert isinstance(inspect.getattr_static(layer, "fused_multilabel_learnt"), property), layer
        params = list(inspect.signature(layer.__init__).parameters)
        assert params[-1] == "fused_backward" and "fused_multilabel_learnt" not in params, layer


def test_the_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "routes.cpp"
    src.write_text("""
#include "lccrf_densecrf.hpp"
unsigned routes_of(DenseCRF::DenseCRFHIP<4> &a)
{
    static_assert(LCCRF_MULTILABEL_POTTS == 1 && LCCRF_MULTILABEL_LEARNT == 2, "route bits");
    a.setMultilabelRoutes(LCCRF_MULTILABEL_POTTS | LCCRF_MULTILABEL_LEARNT);
    const DenseCRF::DenseCRFHIP<4> &c = a;
    return c.multilabelRoutes();
}
""")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


# ---- GPU: bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(lc.CASES))
def test_inference_is_the_restatement_bit_for_bit_on_engine_six(po, wl, name):
    c = lc.prepared(name, po, wl)
    q, _ = c.expected(5)
    h = c.handle(pkg)
    h.inference(5, True, 1.0)
    _same(h, q, (name, c.model_name))
    engine, word = h.engine()
    assert engine == 6, (name, engine, word)
    assert lc.shape_word(word) == (lc.LANES,) + c.cls[:2], (name, lc.shape_word(word), c.cls)
    h.set_multilabel_routes(0)                                   # the same handle with the bit off: the streaming engine, the same bits
    h.inference(5, True, 1.0)
    assert h.engine() == (1, 0), (name, h.engine())
    _same(h, q, (name, c.model_name, "off"))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T,relax", [(0, 1.0), (1, 1.0), (5, 1.0), (5, 0.5)])
def test_every_schedule_branch(po, wl, T, relax):
    c = lc.prepared(lc.SCHEDULE_CASE, po, wl)
    h = c.handle(pkg)
    h.inference(T, True, relax)
    _same(h, c.expected(T, relax)[0], (T, relax))
    assert h.engine()[0] == 6 and lc.shape_word(h.engine()[1]) == (lc.LANES,) + c.cls[:2]
    h.close()


@pytest.mark.gpu
def test_without_map_the_labels_are_left_untouched(po, wl):
    c = lc.prepared(lc.SCHEDULE_CASE, po, wl)
    (q0, m0), (q5, m5) = c.expected(0), c.expected(5)
    assert not np.array_equal(m0, m5)                            # (or the check below would show nothing)
    h = c.handle(pkg)
    h.inference(0, True, 1.0)
    assert np.array_equal(h.map(), m0)
    h.inference(5, False, 1.0)
    assert h.engine()[0] == 6
    assert cc.same_bits(h.probability(), q5)
    assert np.array_equal(h.map(), m0)
    h.close()


# ---- GPU: the two bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_two_bits_are_independent(po, wl, lib):
    import ctypes as C
    c = lc.prepared("L3/N1001", po, wl)
    potts_q, potts_m = mc.expected("L3/N1001", po, wl, 5, 1.0)
    learnt, potts = c.handle(pkg, routes=0), cc.setup(pkg.DenseCRFHIP, c.pb)

    def engines(routes):
        out = []
        for h, (q, m) in ((learnt, c.expected(5)), (potts, (potts_q, potts_m))):
            h.set_multilabel_routes(routes)
            assert h.multilabel_routes() == routes
            h.inference(5, True, 1.0)
            assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m), routes
            out.append(h.engine()[0])
        return tuple(out)

    assert engines(0) == (1, 1)
    assert engines(POTTS) == (1, 5) and learnt.engine() == (1, 0)
    assert engines(LEARNT) == (6, 1)
    assert engines(POTTS | LEARNT) == (6, 5)
    # option 9 IS bit 0, and touches it alone
    learnt.set_option(pkg.OPT_FUSED_MULTILABEL, 0)
    assert learnt.multilabel_routes() == LEARNT
    learnt.set_option(pkg.OPT_FUSED_MULTILABEL, 1)
    assert learnt.multilabel_routes() == (POTTS | LEARNT)
    learnt.set_multilabel_routes(LEARNT)
    potts.set_multilabel_routes(POTTS)
    potts.inference(5, True, 1.0)
    assert potts.engine()[0] == 5
    # refusals on a handle: bits beyond the two, a NULL out-pointer; nothing is written
    assert lib.lccrf_set_multilabel_routes(learnt.h, 4) == E_INVALID and b"LCCRF_MULTILABEL" in lib.lccrf_last_error()
    assert lib.lccrf_set_multilabel_routes(learnt.h, 0xffffffff) == E_INVALID
    assert lib.lccrf_get_multilabel_routes(learnt.h, None) == E_INVALID and b"NULL" in lib.lccrf_last_error()
    assert learnt.multilabel_routes() == LEARNT
    learnt.close(), potts.close()
    # a recycled handle starts without the bit, and the process-wide default of option 9 reaches bit 0 alone
    pkg.set_default_option(pkg.OPT_FUSED_MULTILABEL, 1)
    try:
        again = cc.setup(pkg.DenseCRFHIP, c.pb)
    finally:
        pkg.set_default_option(pkg.OPT_FUSED_MULTILABEL, 0)
    assert again.multilabel_routes() == POTTS
    again.close()
    fresh = cc.setup(pkg.DenseCRFHIP, c.pb)
    assert fresh.multilabel_routes() == 0
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["matrix", "mode"])
def test_removing_and_restoring_the_model(po, wl, what):
    pb, _ = mc.prepared("L3/N1001", po, wl)
    c = lc.Prepared("L3/N1001", po, wl, pb=pb, model_name="matrix0" if what == "matrix" else "before")
    potts_q, potts_m = mc.expected("L3/N1001", po, wl, 5, 1.0)
    for routes, bare in ((POTTS | LEARNT, 5), (LEARNT, 1)):
        h = c.handle(pkg, routes=routes)
        h.inference(5, True, 1.0)
        assert h.engine()[0] == 6
        _same(h, c.expected(5)[0], (what, routes))
        if what == "matrix":                                     # taken back: a Potts frame, engine 5 or 1 by the other bit
            h.set_pairwise_compatibility(0, None)
        else:
            h.set_normalization(0, nc.AFTER)
        h.inference(5, True, 1.0)
        assert h.engine()[0] == bare, (what, routes, h.engine())
        assert cc.same_bits(h.probability(), potts_q) and np.array_equal(h.map(), potts_m)
        c.put_model(h)                                           # ... and set again: engine 6 on the next inference
        h.inference(5, True, 1.0)
        assert h.engine()[0] == 6
        _same(h, c.expected(5)[0], (what, routes, "again"))
        h.close()


# ---- GPU: what does not move ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_converged_call_stays_on_the_streaming_engine(po, wl):
    c = lc.prepared("L3/N1001", po, wl)
    h = c.handle(pkg)
    rep = h.inference_converged(12, pkg.STOP_LABELS, 0.0, True, 1.0)
    assert h.engine() == (1, 0), h.engine()
    assert 0 < rep["iterations"] <= 12
    _same(h, c.expected(rep["iterations"], 1.0, cap=12)[0], rep)
    h.inference(5, True, 1.0)                                    # ... and a fixed count behind it takes the new route
    assert h.engine()[0] == 6
    _same(h, c.expected(5)[0], "fixed")
    h.close()


@pytest.mark.gpu
def test_the_stepwise_calls_stay_on_the_streaming_engine(po, wl):
    c = lc.prepared("L4/N1025", po, wl)
    h = c.handle(pkg)
    h.start_inference()
    for _ in range(5):
        h.step_inference(1.0)
    h.build_map()
    _same(h, c.expected(5)[0], "steps")
    h.inference(5, True, 1.0)
    assert h.engine()[0] == 6
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,args", [
    ("nine labels", dict(N=1001, L=9)),
    ("2049 points", dict(N=2049, L=3)),
    ("2049 points at four labels", dict(N=2049, L=4, unary="label")),
    ("1025 points at five labels", dict(N=1025, L=5, unary="label")),
    ("1025 points at six labels", dict(N=1025, L=6)),
    ("1025 points at seven labels", dict(N=1025, L=7)),
    ("1025 points at eight labels", dict(N=1025, L=8, unary="label")),
])
def test_frames_beyond_the_plan_stay_on_the_streaming_engine(po, wl, name, args):
    assert args["L"] not in lc.PLAN or args["N"] == lc.PLAN[args["L"]] + 1
    c = lc.Prepared(name, po, wl, pb=mc.problem(wl, **args), model_name="before+matrix")
    h = c.handle(pkg, routes=POTTS | LEARNT)
    h.inference(5, True, 1.0)
    assert h.engine() == (1, 0), (name, h.engine())
    _same(h, c.expected(5)[0], name)
    h.close()


@pytest.mark.gpu
def test_a_three_dimensional_term_stays_on_the_streaming_engine(po, wl):
    pb = mc.problem(wl, N=500, L=3)
    f3 = np.concatenate([pb["kernels"][1][0], pb["kernels"][0][0][:, :1]], 1).astype(np.float32)
    pb = dict(pb, kernels=[pb["kernels"][0], (f3, pb["kernels"][1][1])])
    c = lc.Prepared("3-D", po, wl, pb=pb, model_name="symmetric+matrix")
    h = c.handle(pkg, routes=POTTS | LEARNT)
    h.inference(5, True, 1.0)
    assert h.engine() == (1, 0), h.engine()
    _same(h, c.expected(5)[0], "3-D")
    h.close()


# ---- GPU: batches -------------------------------------------------------------------------------------------------------------
def _sizes(L):
    return tuple(n for n in (0, 5, 1001, 1025, 2048) if n <= lc.PLAN[L])


BATCH_MODEL = "before+matrix"                                    # (no term in mode NONE: one weight per term serves every frame)


def _batch(wl, L, routes):
    sizes = _sizes(L)
    pbs = [mc.problem(wl, N=n, L=L) for n in sizes if n]
    maxN, F = max(sizes), len(sizes)
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(2)]
    unary = np.zeros((F, maxN, L), np.float32)
    for pb in pbs:
        f = sizes.index(pb["N"])
        unary[f, :pb["N"]] = pb["unary"]
        for k in range(2):
            feats[k][f, :pb["N"]] = pb["kernels"][k][0]
    b = pkg.BatchCRF(F, maxN, L, [2, 2], [float(w) for _, w in pbs[0]["kernels"]])
    modes, mats = lc.model(BATCH_MODEL, 2, L)
    for k in range(2):                                           # section 2g's setters
        b.set_normalization(k, modes[k])
        if mats[k] is not None:
            b.set_pairwise_compatibility(k, mats[k])
    b.set_multilabel_routes(routes)
    b.set_inputs_host(list(sizes), feats, unary=unary)
    return b, pbs, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 4])
def test_a_ragged_batch_is_its_frames_on_handles(po, wl, L):
    b, pbs, sizes = _batch(wl, L, LEARNT)
    assert b.multilabel_routes() == LEARNT
    refs = []
    for pb in pbs:                                               # every frame on a handle of its own, on the streaming engine
        c = lc.Prepared("frame", po, wl, pb=pb, model_name=BATCH_MODEL)
        h = c.handle(pkg, routes=0)
        h.inference(5, True, 1.0)
        assert h.engine() == (1, 0)
        refs.append((h.probability(), h.map()))
        h.close()
    assert cc.same_bits(refs[-1][0], c.expected(5)[0])           # (the largest frame: the restatement too)

    def check(tag):
        Q, M = b.probability(), b.map()
        for pb, (rq, rm) in zip(pbs, refs):
            f, n = sizes.index(pb["N"]), pb["N"]
            assert cc.same_bits(Q[f, :n], rq), (tag, L, n, float(np.abs(Q[f, :n] - rq).max()))
            assert np.array_equal(M[f, :n], rm), (tag, L, n)

    b.build()
    b.inference(5, True, 1.0)
    check("inference")
    assert b.engine() == 6
    assert b.fused_shape() == (1024, (max(sizes) + 1023) // 1024)
    b.run(5, True, 1.0)                                          # builds into HBM for these frames, then the same route
    check("run")
    assert b.engine() == 6
    b.set_multilabel_routes(POTTS)
    b.inference(5, True, 1.0)
    check("bit off")
    assert b.engine() == 1
    b.close()


@pytest.mark.gpu
def test_fused_or_fail_is_honoured_with_the_bit_on_only(wl):
    b, _, _ = _batch(wl, 3, LEARNT)
    b.set_engine(2)
    b.build()
    b.inference(1, True, 1.0)
    assert b.engine() == 6
    b.close()
    b, _, _ = _batch(wl, 3, POTTS)
    b.set_engine(2)
    b.build()
    with pytest.raises(pkg.LccrfError):
        b.inference(1, True, 1.0)
    b.close()


# ---- GPU: the torch layers -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_layer_with_the_attribute_is_the_layer_without_it(po, wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = mc.problem(wl, N=1025, L=3)
    N, L, T, relax = pb["N"], 3, 5, 0.7
    c = lc.Prepared("layer", po, wl, pb=pb, model_name="before+matrix")
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((N, L)).astype(np.float32)).cuda()
    out = []
    for on in (False, True):
        layer = ag.CompatMeanFieldCRF(N, L, nc.feats(pb), [float(w) for w in c.w], n_iterations=T, relax=relax, normalization=c.modes)
        assert layer.fused_multilabel_learnt is False
        layer.fused_multilabel_learnt = on
        assert layer.fused_multilabel_learnt is on and layer.crf.multilabel_routes() == (LEARNT if on else 0)
        with torch.no_grad():
            layer.compat.copy_(torch.from_numpy(np.stack(c.mats)))
        u = torch.from_numpy(pb["unary"]).cuda().requires_grad_(True)
        q = layer(u)
        torch.cuda.synchronize()
        assert layer.crf.engine()[0] == (6 if on else 1)
        q.backward(G)
        torch.cuda.synchronize()
        out.append((q.detach().cpu().numpy(), u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), layer.compat.grad.cpu().numpy()))
        layer.close()
    assert cc.same_bits(out[0][0], c.expected(T, relax)[0])
    for a, b in zip(out[0], out[1]):
        assert cc.same_bits(a, b)
    assert all(np.abs(g).max() > 0 for g in out[0][1:])


@pytest.mark.gpu
def test_the_batch_layer_with_the_attribute_is_the_layer_without_it(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pbs = [mc.problem(wl, N=n, L=3) for n in (5, 1025)]
    F, maxN, L = 2, 1025, 3
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(2)]
    U = np.zeros((F, maxN, L), np.float32)
    for f, pb in enumerate(pbs):
        U[f, :pb["N"]] = pb["unary"]
        for k in range(2):
            feats[k][f, :pb["N"]] = pb["kernels"][k][0]
    modes, mats = lc.model(BATCH_MODEL, 2, L)
    G = torch.from_numpy(np.random.default_rng(3).standard_normal((F, maxN, L)).astype(np.float32)).cuda()
    out = []
    for on in (False, True):
        layer = ag.BatchCompatMeanFieldCRF([5, 1025], feats, [float(w) for _, w in pbs[0]["kernels"]], n_iterations=5, n_labels=L,
                                           normalization=modes)
        layer.fused_multilabel_learnt = on
        with torch.no_grad():
            layer.compat.copy_(torch.from_numpy(np.stack(mats)))
        u = torch.from_numpy(U).cuda().requires_grad_(True)
        q = layer(u)
        torch.cuda.synchronize()
        assert layer.batch.engine() == (6 if on else 1)
        q.backward(G)
        torch.cuda.synchronize()
        out.append((q.detach().cpu().numpy(), u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy(), layer.compat.grad.cpu().numpy()))
        layer.close()
    for f, pb in enumerate(pbs):
        for a, b in zip(out[0][:2], out[1][:2]):
            assert cc.same_bits(a[f, :pb["N"]], b[f, :pb["N"]])
    for a, b in zip(out[0][2:], out[1][2:]):
        assert cc.same_bits(a, b)
    assert all(np.abs(g).max() > 0 for g in out[0][1:])

"""Frames of three to eight labels in one launch on the fused engine (csrc/fused_multilabel.hip; LCCRF_OPT_FUSED_MULTILABEL, engine 5).

CPU: the instantiation class -- points per lane, kernel 0 on chain rows, own or shared product buffers -- every case is there for,
from the oracle's lattices.  GPU: lccrf_inference with the option on against pyoracle.OracleCRF, bit for bit on Q, the labels
identical, the engine report 5 with the shape word the CPU part derived; the streaming engine on the same handle; every frame and
model beyond the route, which keep today's engine and the oracle's bits; batches; the torch layer."""
import ctypes as C
import importlib

import numpy as np
import pytest

import compat_checker as ck
import crf_cases as cc
import fused_multilabel_cases as mc
import normalization_checker as nc
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
OPT = 9
E_INVALID = -1


def _handle(pb, on=True):
    h = cc.setup(pkg.DenseCRFHIP, pb)
    if on:
        h.set_option(OPT, 1)
    return h


def _oracle(po, pb, T, relax=1.0):
    o = cc.setup(po.OracleCRF, pb)
    o.inference_native(T, True, relax)
    q, m = o.probability(), o.map()
    o.close()
    return q, m


def _check_oracle(h, po, pb, T, relax, engine):
    h.inference(T, True, relax)
    q, m = _oracle(po, pb, T, relax)
    got = h.probability()
    assert cc.same_bits(got, q), (T, relax, float(np.abs(got - q).max()))
    assert np.array_equal(h.map(), m)
    assert h.engine() == engine, h.engine()


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_instantiation_class_it_is_there_for(po, wl):
    seen = set()
    for name, (args, want) in mc.CASES.items():
        pb, got = mc.prepared(name, po, wl)
        assert got == want, (name, got, want)
        assert pb["N"] <= mc.PLAN[pb["L"]], name
        seen.add((pb["L"], len(pb["kernels"])) + got[:2])
    # every instantiation of the kernel: (labels, terms, points per lane, row path) over the shipped range
    assert seen == {(L, k, p, ch) for L, n in mc.PLAN.items() for k in (1, 2) for p in range(1, n // mc.LANES + 1) for ch in (0, 1)}, seen
    # own and shared product buffers
    assert {mc.prepared(n, po, wl)[1][2] for n in mc.CASES} == {0, 1}
    assert mc.prepared("L3/N1025", po, wl)[0]["N"] % mc.LANES == 1 and mc.prepared("L3/N5", po, wl)[0]["N"] % 4 == 1
    # unknown labels occur in the label-derived cases
    assert (mc.prepared("L4/N2048", po, wl)[0]["label"] == -1).any()


# ---- GPU: bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mc.CASES))
def test_inference_is_the_oracle_bit_for_bit_on_engine_five(po, wl, name):
    pb, cls = mc.prepared(name, po, wl)
    q, m = mc.expected(name, po, wl, 5, 1.0)
    h = _handle(pb)
    h.inference(5, True, 1.0)
    got = h.probability()
    assert cc.same_bits(got, q), (name, float(np.abs(got - q).max()))
    assert np.array_equal(h.map(), m), name
    engine, word = h.engine()
    assert engine == 5, (name, engine, word)
    assert mc.shape_word(word) == (mc.LANES,) + cls[:2], (name, mc.shape_word(word), cls)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T,relax", [(0, 1.0), (1, 1.0), (5, 1.0), (5, 0.5)])
def test_every_schedule_branch(po, wl, T, relax):
    name = mc.SCHEDULE_CASE
    pb, cls = mc.prepared(name, po, wl)
    q, m = mc.expected(name, po, wl, T, relax)
    h = _handle(pb)
    h.inference(T, True, relax)
    assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m), (T, relax)
    assert h.engine()[0] == 5 and mc.shape_word(h.engine()[1]) == (mc.LANES,) + cls[:2]
    h.close()


@pytest.mark.gpu
def test_without_map_the_labels_are_left_untouched(po, wl):
    name = mc.SCHEDULE_CASE
    pb, _ = mc.prepared(name, po, wl)
    q0, m0 = mc.expected(name, po, wl, 0, 1.0)
    q5, m5 = mc.expected(name, po, wl, 5, 1.0)
    assert not np.array_equal(m0, m5)                            # (or the check below would show nothing)
    h = _handle(pb)
    h.inference(0, True, 1.0)
    assert np.array_equal(h.map(), m0)
    h.inference(5, False, 1.0)
    assert h.engine()[0] == 5
    assert cc.same_bits(h.probability(), q5)
    assert np.array_equal(h.map(), m0)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L3/N1025", "L8/N1001"])
def test_the_same_handle_on_both_routes(po, wl, name):
    """lccrf_start_inference + T x lccrf_step_inference is the streaming engine; lccrf_inference behind it takes the new route"""
    pb, _ = mc.prepared(name, po, wl)
    h = _handle(pb)
    for T, relax in ((5, 1.0), (3, 0.5)):
        h.start_inference()
        for _ in range(T):
            h.step_inference(relax)
        h.build_map()
        qs, ms = h.probability(), h.map()
        h.inference(T, True, relax)
        assert h.engine()[0] == 5
        assert cc.same_bits(h.probability(), qs) and np.array_equal(h.map(), ms), (name, T, relax)
    h.close()


# ---- GPU: refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_option_alone_moves_a_three_label_frame_from_engine_one_to_five(po, wl, lib):
    pb, cls = mc.prepared("L3/N1001", po, wl)
    off, on = _handle(pb, on=False), _handle(pb, on=False)
    assert lib.lccrf_set_option(on.h, OPT, 1) == 0
    assert lib.lccrf_set_option(on.h, 10, 1) == E_INVALID
    _check_oracle(off, po, pb, 5, 1.0, (1, 0))
    on.inference(5, True, 1.0)
    assert on.engine()[0] == 5 != off.engine()[0]
    assert cc.same_bits(on.probability(), off.probability()) and np.array_equal(on.map(), off.map())
    on.set_option(OPT, 0)                                        # takes effect with the next inference, both ways
    _check_oracle(on, po, pb, 5, 1.0, (1, 0))
    off.set_option(OPT, 1)
    off.inference(5, True, 1.0)
    assert off.engine() == (5, 1024 | cls[0] << 16 | cls[1] << 20)
    off.close(), on.close()


@pytest.mark.gpu
def test_two_labels_keep_their_engines_with_the_option_on_and_off(po, wl):
    pb = wl.slam_problem(1001, seed=21)
    q, m = _oracle(po, pb, 5)
    for on in (False, True):
        h = _handle(pb, on=on)
        h.inference(5, True, 1.0)
        first = h.engine()
        h.inference(5, True, 1.0)                                # (lattices in HBM now)
        assert first[0] in (2, 3) and h.engine()[0] in (2, 3), (on, first, h.engine())
        assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m), on
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,args", [
    ("nine labels", dict(N=1001, L=9)),                          # the first label count beyond the shipped maximum
    ("2049 points", dict(N=2049, L=3)),
    ("1025 points at five labels", dict(N=1025, L=5, unary="label")),   # (five to eight labels: frames of up to 1024 points)
])
def test_frames_beyond_the_plan_stay_on_the_streaming_engine(po, wl, name, args):
    pb = mc.problem(wl, **args)
    h = _handle(pb)
    _check_oracle(h, po, pb, 5, 1.0, (1, 0))
    h.close()


@pytest.mark.gpu
def test_a_three_dimensional_term_stays_on_the_streaming_engine(po, wl):
    pb = mc.problem(wl, N=500, L=3)
    f3 = np.concatenate([pb["kernels"][1][0], pb["kernels"][0][0][:, :1]], 1).astype(np.float32)
    pb = dict(pb, kernels=[pb["kernels"][0], (f3, pb["kernels"][1][1])])
    h = _handle(pb)
    _check_oracle(h, po, pb, 5, 1.0, (1, 0))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["matrix", "before"])
def test_a_matrix_or_a_mode_stays_on_the_streaming_engine(po, wl, what):
    pb = mc.problem(wl, N=1001, L=3)
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    rng = np.random.default_rng([77, 2, 3])
    mats = [(np.eye(3) + 0.3 * rng.standard_normal((3, 3))).astype(np.float32), None] if what == "matrix" else [None, None]
    modes = [nc.AFTER, nc.AFTER] if what == "matrix" else [nc.AFTER, nc.BEFORE]
    w = nc.weights_f32(pb, nrm, modes)
    ref = nc.restate_f32(U, nc.feats(pb), w, mats, modes, 5, 1.0, nrm)
    h = _handle(pb)
    if what == "matrix":
        h.set_pairwise_compatibility(0, mats[0])
    else:
        h.set_normalization(1, nc.BEFORE)
    h.inference(5, True, 1.0)
    assert h.engine() == (1, 0), h.engine()
    assert cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref))
    # taken back: the new route again
    if what == "matrix":
        h.set_pairwise_compatibility(0, None)
    else:
        h.set_normalization(1, nc.AFTER)
    h.inference(5, True, 1.0)
    assert h.engine()[0] == 5
    q, m = _oracle(po, pb, 5)
    assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m)
    h.close()


@pytest.mark.gpu
def test_the_converged_call_stays_on_the_streaming_engine(po, wl):
    pb, _ = mc.prepared("L3/N1001", po, wl)
    h = _handle(pb)
    rep = h.inference_converged(12, pkg.STOP_LABELS, 0.0, True, 1.0)
    assert h.engine() == (1, 0), h.engine()
    q, m = _oracle(po, pb, rep["iterations"])
    assert cc.same_bits(h.probability(), q) and np.array_equal(h.map(), m), rep
    h.inference(5, True, 1.0)                                    # ... and a fixed count behind it takes the new route
    assert h.engine()[0] == 5
    assert cc.same_bits(h.probability(), mc.expected("L3/N1001", po, wl, 5, 1.0)[0])
    h.close()


# ---- GPU: batches -------------------------------------------------------------------------------------------------------------
SIZES = (0, 5, 1001, 1025, 2048)


def _batch(wl, L, on):
    pbs = [mc.problem(wl, N=n, L=L) for n in SIZES if n]
    maxN, F = max(SIZES), len(SIZES)
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(2)]
    unary = np.zeros((F, maxN, L), np.float32)
    for pb in pbs:
        f = SIZES.index(pb["N"])
        unary[f, :pb["N"]] = pb["unary"]
        for k in range(2):
            feats[k][f, :pb["N"]] = pb["kernels"][k][0]
    b = pkg.BatchCRF(F, maxN, L, [2, 2], [float(w) for _, w in pbs[0]["kernels"]])
    if on:
        b.set_option(OPT, 1)
    b.set_inputs_host(list(SIZES), feats, unary=unary)
    return b, pbs


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 4])
def test_a_ragged_batch_is_its_frames_on_handles(po, wl, L, lib):
    b, pbs = _batch(wl, L, on=True)
    refs = []
    for pb in pbs:                                               # every frame on a handle of its own (the streaming engine)
        h = _handle(pb, on=False)
        h.inference(5, True, 1.0)
        assert h.engine() == (1, 0)
        refs.append((h.probability(), h.map()))
        h.close()
    q, m = _oracle(po, pbs[-1], 5)
    assert cc.same_bits(refs[-1][0], q) and np.array_equal(refs[-1][1], m)

    def check(tag):
        Q, M = b.probability(), b.map()
        for pb, (rq, rm) in zip(pbs, refs):
            f, n = SIZES.index(pb["N"]), pb["N"]
            assert cc.same_bits(Q[f, :n], rq), (tag, L, n, float(np.abs(Q[f, :n] - rq).max()))
            assert np.array_equal(M[f, :n], rm), (tag, L, n)

    b.build()
    b.inference(5, True, 1.0)
    check("inference")
    assert b.engine() == 5
    assert b.fused_shape() == (1024, 2)
    p, w = C.c_void_p(), C.c_int(0)
    assert lib.lccrf_batch_device_label_bits(b.h, C.byref(p), C.byref(w)) == E_INVALID   # two labels only, as before
    b.run(5, True, 1.0)                                          # builds into HBM for these frames, then the same route
    check("run")
    assert b.engine() == 5
    b.set_option(OPT, 0)
    b.inference(5, True, 1.0)
    check("option off")
    assert b.engine() == 1
    b.close()


@pytest.mark.gpu
def test_fused_or_fail_is_honoured_with_the_option_on_only(wl):
    b, _ = _batch(wl, 3, on=True)
    b.set_engine(2)
    b.build()
    b.inference(1, True, 1.0)
    assert b.engine() == 5
    b.close()
    b, _ = _batch(wl, 3, on=False)
    b.set_engine(2)
    b.build()
    with pytest.raises(pkg.LccrfError):
        b.inference(1, True, 1.0)
    b.close()


@pytest.mark.gpu
def test_the_process_wide_default_reaches_new_handles_only(po, wl):
    pb, _ = mc.prepared("L3/N1001", po, wl)
    before = _handle(pb, on=False)
    pkg.set_default_option(OPT, 1)
    try:
        after = _handle(pb, on=False)
    finally:
        pkg.set_default_option(OPT, 0)
    for h, engine in ((before, 1), (after, 5)):
        h.inference(5, True, 1.0)
        assert h.engine()[0] == engine
        assert cc.same_bits(h.probability(), mc.expected("L3/N1001", po, wl, 5, 1.0)[0])
        h.close()


# ---- GPU: the torch layer ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_layer_with_the_option_is_the_layer_without_it(po, wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb = mc.problem(wl, N=1025, L=3)
    N, L, T, relax = pb["N"], 3, 5, 0.7
    U = pb["unary"]
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((N, L)).astype(np.float32)).cuda()
    out = []
    for on in (False, True):
        layer = ag.MeanFieldCRF(N, L, nc.feats(pb), [float(w) for _, w in pb["kernels"]], n_iterations=T, relax=relax)
        assert layer.fused_multilabel is False
        layer.fused_multilabel = on
        assert layer.fused_multilabel is on
        u = torch.from_numpy(U).cuda().requires_grad_(True)
        q = layer(u)
        torch.cuda.synchronize()
        assert layer.crf.engine()[0] == (5 if on else 1)
        q.backward(G)
        torch.cuda.synchronize()
        out.append((q.detach().cpu().numpy(), u.grad.cpu().numpy(), layer.weights.grad.cpu().numpy()))
        layer.close()
    ref, _ = _oracle(po, pb, T, relax)
    assert cc.same_bits(out[0][0], ref)
    for a, b in zip(out[0], out[1]):
        assert cc.same_bits(a, b)
    assert np.abs(out[0][1]).max() > 0 and np.abs(out[0][2]).max() > 0


@pytest.mark.gpu
def test_the_batch_layer_takes_the_attribute(wl):
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pbs = [mc.problem(wl, N=n, L=3) for n in (5, 1025)]
    F, maxN = 2, 1025
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(2)]
    U = np.zeros((F, maxN, 3), np.float32)
    for f, pb in enumerate(pbs):
        U[f, :pb["N"]] = pb["unary"]
        for k in range(2):
            feats[k][f, :pb["N"]] = pb["kernels"][k][0]
    out = []
    for on in (False, True):
        layer = ag.BatchMeanFieldCRF([5, 1025], feats, [float(w) for _, w in pbs[0]["kernels"]], n_iterations=5, n_labels=3)
        layer.fused_multilabel = on
        q = layer(torch.from_numpy(U).cuda())
        torch.cuda.synchronize()
        assert layer.batch.engine() == (5 if on else 1)
        out.append(q.detach().cpu().numpy())
        layer.close()
    for f, pb in enumerate(pbs):
        assert cc.same_bits(out[0][f, :pb["N"]], out[1][f, :pb["N"]])

"""Batches with label-compatibility matrices and normalisation modes (include/lccrf.h section 2g): the setters, the fixed-count
inference of such a batch in one launch (csrc/fused_general.hip with a workgroup per frame) and the until-converged inference in one
launch (csrc/fused_general_converge.hip).

The reference of every frame is its own restated trace (normalization_checker.restate_trace_f32: bit-exact float32 with matrices
and modes); a handle holding the same frame with the same settings is the second witness.  The batches, their traces and what the
launchers must report are in tests/batch_general_cases.py.

CPU: the entry points, the argument checks that need no device, that the batches reach all eight instantiations of both kernels,
the stop profile of the convergence batches, and that one point decides in the frames the reach test picks.  GPU: the rest."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import batch_general_cases as bg
import compat_checker as ck
import converge_cases as cv
import crf_cases as cc
import normalization_checker as nc
import test_fused_general as fg
from abi_support import assert_declared_exported_bound, dev, lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
F32 = np.float32
E_INVALID, E_STATE = -1, -5
ENTRY_POINTS = ("lccrf_batch_set_pairwise_compatibility", "lccrf_batch_get_pairwise_compatibility",
                "lccrf_batch_set_pairwise_normalization", "lccrf_batch_get_pairwise_normalization")
SETTINGS = fg.SETTINGS
GENERAL = [s for s in SETTINGS if s != "after"]                   # (every term AFTER without a matrix is the Potts batch: engine 2)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound(lib, ENTRY_POINTS)
    assert lib.lccrf_abi_version() == 3                           # added without a step: callers probe by symbol
    for m in ("set_pairwise_compatibility", "pairwise_compatibility", "set_normalization", "normalization"):
        assert callable(getattr(pkg.BatchCRF, m, None)), m


def test_argument_checks_need_no_device(lib):
    """a NULL batch; and, refused before the batch is looked at, a kernel no batch can have, a mode of -1 or 4, a NULL output.  A NaN
    entry needs the batch's label count to be found: with a NULL batch the answer is the NULL batch's (the GPU test has the rest)."""
    eye = np.eye(2, dtype=F32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    flag, mode = C.c_int(7), C.c_int(7)
    assert lib.lccrf_batch_set_pairwise_compatibility(None, 0, p(eye)) == E_INVALID
    assert b"NULL" in lib.lccrf_last_error()
    assert lib.lccrf_batch_get_pairwise_compatibility(None, 0, p(eye), C.byref(flag)) == E_INVALID
    assert lib.lccrf_batch_set_pairwise_normalization(None, 0, nc.SYMMETRIC) == E_INVALID
    assert lib.lccrf_batch_get_pairwise_normalization(None, 0, C.byref(mode)) == E_INVALID
    for k in (-1, pkg.MAX_KERNELS):
        assert lib.lccrf_batch_set_pairwise_compatibility(None, k, p(eye)) == E_INVALID
        assert b"kernel index" in lib.lccrf_last_error()
        assert lib.lccrf_batch_get_pairwise_compatibility(None, k, None, None) == E_INVALID
        assert lib.lccrf_batch_set_pairwise_normalization(None, k, nc.BEFORE) == E_INVALID
        assert lib.lccrf_batch_get_pairwise_normalization(None, k, C.byref(mode)) == E_INVALID
    for bad in (-1, 4):
        assert lib.lccrf_batch_set_pairwise_normalization(None, 0, bad) == E_INVALID
        assert b"normalization mode" in lib.lccrf_last_error()
    nan = np.array([[1, np.nan], [0, 1]], F32)
    assert lib.lccrf_batch_set_pairwise_compatibility(None, 0, p(nan)) == E_INVALID
    assert lib.lccrf_batch_get_pairwise_normalization(None, 0, None) == E_INVALID
    assert b"mode is NULL" in lib.lccrf_last_error()
    assert (flag.value, mode.value) == (7, 7)


def test_batches_reach_all_eight_instantiations_of_both_kernels(po, wl, golden):
    """(K, points per lane, chain rows) batch-wide from the oracle's lattices: points per lane from the largest N of the batch, chain
    rows when kernel 0's longest row over the batch has at least 64 products and its largest V is at most 464"""
    seen = set()
    for name in bg.BATCHES:
        bt = bg.batch(name, golden, po, wl)
        assert bt.shape() == bg.WANT[name], (name, bt.shape(), bt.maxV, bt.row0)
        assert bt.lds_plan(16) == (True, True), name              # a product buffer per term, and room for the reduction's words
        assert 0 in bt.N[1:-1] and bt.maxN > bt.N.max() <= bg.MAX_POINTS, name    # an empty frame in the middle; max_points beyond N
        seen.add(bt.shape())
    assert seen == {(k, p, ch) for k in (1, 2) for p in (1, 2) for ch in (0, 1)}
    assert {int(n) for n in bg.batch("two/", golden, po, wl).N} == {5, 7, 1001, 1024, 0, 1025, 2000, 2048}
    assert sorted(int(n) for n in bg.batch("one/", golden, po, wl).N) == [0, 5, 7, 1001, 1001, 1024]
    # the sparse frame: both terms' products in ONE buffer, lattices beyond the prologue's register rounds (1365 / 2047 vertices);
    # next to c2 the plan does not fit one workgroup's LDS at all
    sp = bg.batch("sparse+N1025", golden, po, wl)
    assert sp.lds_plan(16) == (True, False) and sp.maxV[0] > 2047 and sp.shape() == (2, 2, 0), (sp.maxV, sp.shape())
    assert bg.batch("sparse+c2", golden, po, wl).lds_plan() == (False, False)


# (batch, setting, relax) -> LABELS at cap 12 on the restated traces; the profile is asserted per batch over its entries
PROFILE_FULL = ("two/", "one/", "two/appearance", "two/smooth", "two/smooth_first", "one/smooth_first")
# The one-point-per-lane batches of ONE term: no frame of at most 1024 points keeps flipping to the cap under any setting (the
# restatement: one/appearance stops at 1 .. 11, one/smooth at 1 .. 12 with the criterion met), so nothing there ends with
# converged = 0 at cap 12; the caps below a frame's stop (converged_settings) end runs there.
PROFILE_NO_CAP_FRAME = ("one/appearance", "one/smooth")


def _stops(po, wl, golden, name):
    out = []
    for bname, sname, relax in bg.CONVERGED:
        if bname == name:
            bt = bg.batch(bname, golden, po, wl)
            out += [cv.expect(tr, cv.LABELS, F32(0), bg.CAP) for tr in bg.traces(bt, sname, relax) if tr[0].shape[0]]
    return out


def test_convergence_batches_stop_at_different_iterations_below_and_at_the_cap(po, wl, golden):
    assert {b for b, _, _ in bg.CONVERGED} == set(bg.BATCHES) == set(PROFILE_FULL) | set(PROFILE_NO_CAP_FRAME)
    for bname, sname, _ in bg.CONVERGED:
        assert bg.is_general(*bg.setting(bg.batch(bname, golden, po, wl), sname)[:2]), (bname, sname)
    for name in bg.BATCHES:
        w = _stops(po, wl, golden, name)
        print(name, [(x[0], x[3]) for x in w])
        assert len({x[0] for x in w}) >= 3, (name, w)                       # at least three distinct stop iterations
        assert any(x[3] == 1 and x[0] < bg.CAP for x in w), (name, w)       # a frame that converges below the cap
        if name in PROFILE_FULL:
            assert any(x[3] == 0 and x[0] == bg.CAP for x in w), (name, w)  # a frame the cap ends
    # with matrices on BOTH terms of a two-term frame the labels keep flipping: the cap frames
    bt = bg.batch("two/", golden, po, wl)
    w = [cv.expect(tr, cv.LABELS, F32(0), bg.CAP) for tr in bg.traces(bt, "matrices", 1.0)]
    assert all((x[0], x[3]) == (bg.CAP, 0) for x, n in zip(w, bt.N) if n > 1000), w


# ---- one point decides: the frames of the reach test ---------------------------------------------------------------------------
REACH = {"N700": lambda wl: wl.slam_problem(700, seed=3), "c2": lambda wl: wl.slam_problem(2000, seed=12)}
REACH_SETTING, REACH_OTHERS = "symmetric", ("N7", "slam:N1001", "N1024")
_REACH = {}


def _learnt_trace(po, pb, cap=bg.CAP):
    """(U, features, norms, weights, modes, matrices, restated trace) of a two-term frame in the symmetric setting"""
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(2)]
    o.close()
    modes, mats = fg._settings(2)[REACH_SETTING]
    w = nc.weights_f32(pb, nrm, modes)
    return U, nc.feats(pb), nrm, w, modes, mats, nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, cap, 1.0, nrm)


def _reach(po, wl, name):
    """per target (rolled problem, its learnt trace, t, point, tol), or None where rolling moved the decision elsewhere"""
    if name not in _REACH:
        pb = REACH[name](wl)
        dec = cv.deciding(_learnt_trace(po, pb)[-1])
        out = {}
        for tname, tgt in cv.targets(pb["N"]).items():
            out[tname] = None
            if dec is None:
                continue
            pb2 = cv.rolled(pb, tgt - dec[1])
            lt = _learnt_trace(po, pb2)                           # rolling changes the bits: the expectation is the rolled input's
            d2 = cv.deciding(lt[-1])
            if d2 is not None and d2[1] == tgt:
                out[tname] = (pb2, lt) + d2
        _REACH[name] = (dec, out)
    return _REACH[name]


@pytest.mark.parametrize("name", list(REACH))
def test_one_point_decides_in_the_frames_the_reach_test_picks(po, wl, name):
    dec, cases = _reach(po, wl, name)
    assert dec is not None, name
    assert set(cases) == set(cv.targets(REACH[name](wl)["N"]))
    ok = [c for c in cases.values() if c is not None]
    assert 2 * len(ok) >= len(cases), {k: v is not None for k, v in cases.items()}     # at most half of the targets may be skipped
    for pb2, lt, t, point, tol in ok:
        tr = lt[-1]
        assert cv.expect(tr, cv.DELTA, tol, bg.CAP, skip=point)[0] == t < cv.expect(tr, cv.DELTA, tol, bg.CAP)[0]


# ---- GPU: fixed-count inference --------------------------------------------------------------------------------------------------
def _check_engine(b, general, fits=True):
    if not general:
        assert b.engine() == 2, b.engine()
    elif fits:
        assert b.engine() == 4 and b.fused_shape() == (1024, 1), (b.engine(), b.fused_shape())
    else:
        assert b.engine() == 1, b.engine()


def _run_fixed(bname, sname, golden, po, wl, fits=True, engine=None):
    bt = bg.batch(bname, golden, po, wl)
    modes, mats, w = bg.setting(bt, sname)
    general = bg.is_general(modes, mats)
    b = bg.make(bt, modes, mats, w, engine=engine)
    for relax in (1.0, 0.7):
        trs = bg.traces(bt, sname, relax, 5)
        for T in (0, 1, 5):
            b.inference(T, True, relax)
            bg.check_frames(b, bt, [tr[T] for tr in trs], (bname, sname, T, relax))
            _check_engine(b, general, fits and engine != 1)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sname", SETTINGS)
@pytest.mark.parametrize("bname", list(bg.BATCHES))
def test_batch_inference_is_every_frames_restatement(po, wl, golden, bname, sname):
    _run_fixed(bname, sname, golden, po, wl)


@pytest.mark.gpu
@pytest.mark.parametrize("sname", GENERAL)
def test_sparse_frame_shares_one_product_buffer_and_takes_the_copy_loops(po, wl, golden, sname):
    _run_fixed("sparse+N1025", sname, golden, po, wl)


@pytest.mark.gpu
def test_sparse_frame_next_to_c2_is_beyond_lds_and_streams(po, wl, golden):
    _run_fixed("sparse+c2", "mixed", golden, po, wl, fits=False)


@pytest.mark.gpu
def test_every_frame_agrees_with_a_handle_holding_it(po, wl, golden):
    """the handle may have taken another instantiation: its own N decides its points per lane and its rows"""
    bt = bg.batch("two/", golden, po, wl)
    modes, mats, w = bg.setting(bt, "mixed")
    b = bg.make(bt, modes, mats, w)
    T, relax = 5, 0.7
    b.inference(T, True, relax)
    q, m = b.probability(), b.map()
    words = set()
    for f, fr in enumerate(bt.frames):
        if fr is None:
            continue
        n, U, ft, _ = fr
        h = fg._handle(dict(N=n, L=2, unary=U, kernels=[(x, 0.0) for x in ft]), w, modes, mats)
        h.inference(T, True, relax)
        assert h.engine()[0] == 4
        words.add(h.engine()[1])
        assert cc.same_bits(q[f, :n], h.probability()) and np.array_equal(m[f, :n], h.map()), f
        h.close()
    assert len(words) >= 3, words                                 # short rows / chain rows, one / two points per lane
    b.close()


# ---- GPU: beyond the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_2049_point_frame_sends_the_batch_to_the_streaming_engine(po, wl, golden):
    bt = bg.Batch("big", ("N7", bg.EMPTY, "N2049"), "", golden, po, wl)
    assert bt.N.max() == bg.MAX_POINTS + 1
    modes, mats, w = bg.setting(bt, "mixed")
    b = bg.make(bt, modes, mats, w)
    for T, relax in ((5, 1.0), (1, 0.7)):
        b.inference(T, True, relax)
        assert b.engine() == 1
        bg.check_frames(b, bt, [tr[T] for tr in bg.traces(bt, "mixed", relax, 5)], ("2049", T, relax))
    b.close()


@pytest.mark.gpu
def test_a_three_label_batch_with_matrices_streams(po, wl, golden):
    pb = cc.golden_problem(golden, "generic:d1_L3")
    K, L, N = len(pb["kernels"]), pb["L"], pb["N"]
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(K)]
    o.close()
    mats, modes = fg._dense(K, L), [nc.AFTER] * K
    w = nc.weights_f32(pb, nrm, modes)
    dims = [f.shape[1] for f in nc.feats(pb)]
    Ns = np.array([N, 0, N], np.int32)
    maxN = N + 3
    feats = [np.zeros((3, maxN, d), F32) for d in dims]
    unary = np.zeros((3, maxN, L), F32)
    for f in (0, 2):
        unary[f, :N] = U
        for k in range(K):
            feats[k][f, :N] = nc.feats(pb)[k]
    b = pkg.BatchCRF(3, maxN, L, dims, [float(x) for x in w])
    for k in range(K):
        b.set_pairwise_compatibility(k, mats[k])
        got, is_set = b.pairwise_compatibility(k)
        assert is_set and cc.same_bits(got, mats[k])
    b.set_inputs_host(Ns, feats, unary=unary)
    b.build()
    for T, relax in ((5, 1.0), (1, 0.7)):
        ref = nc.restate_f32(U, nc.feats(pb), w, mats, modes, T, relax, nrm)
        b.inference(T, True, relax)
        assert b.engine() == 1
        q, m = b.probability(), b.map()
        for f in (0, 2):
            assert cc.same_bits(q[f, :N], ref) and np.array_equal(m[f, :N], ck.map_of(ref)), (f, T, relax)
    b.close()


@pytest.mark.gpu
def test_set_engine_1_keeps_such_a_batch_on_the_streaming_engine(po, wl, golden):
    _run_fixed("one/", "mixed", golden, po, wl, engine=1)


@pytest.mark.gpu
def test_more_frames_bound_later_find_their_factors(po, wl, golden):
    """the array of ones behind a BEFORE / NONE term is made once: the batch first holds two frames, then six"""
    bt = bg.batch("one/", golden, po, wl)
    modes, mats, w = bg.setting(bt, "before")
    first = bg.Batch("first two", ("N7", "N1024"), "", golden, po, wl)
    first.maxN = bt.maxN
    b = bg.make(first, modes, mats, w, max_frames=len(bt.frames))
    b.inference(2, True, 1.0)
    bg.check_frames(b, first, [nc.restate_f32(fr[1], fr[2], w, mats, modes, 2, 1.0, fr[3]) for fr in first.frames], "two frames")
    n, feats, unary = bt.inputs()
    b.set_inputs_host(n, feats, unary=unary)
    b.build()
    b.inference(5, True, 0.7)
    assert b.engine() == 4
    bg.check_frames(b, bt, [tr[5] for tr in bg.traces(bt, "before", 0.7, 5)], "six frames")
    b.close()


# ---- GPU: the setters --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_setters_getters_and_refusals_on_a_batch(po, wl, golden, lib):
    bt = bg.batch("one/", golden, po, wl)
    b = bg.make(bt, [nc.AFTER] * 2, [None] * 2, bt.w0, build=False)
    for k in range(2):                                            # a batch from lccrf_batch_create: no matrix, every term AFTER
        got, is_set = b.pairwise_compatibility(k)
        assert not is_set and np.array_equal(got, np.eye(2, dtype=F32)) and b.normalization(k) == nc.AFTER
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    eye, mode = np.eye(2, dtype=F32), C.c_int(7)
    for bad_k in (-1, 2):
        assert lib.lccrf_batch_set_pairwise_compatibility(b.h, bad_k, p(eye)) == E_INVALID
        assert lib.lccrf_batch_get_pairwise_compatibility(b.h, bad_k, None, None) == E_INVALID
        assert lib.lccrf_batch_set_pairwise_normalization(b.h, bad_k, nc.BEFORE) == E_INVALID
        assert lib.lccrf_batch_get_pairwise_normalization(b.h, bad_k, C.byref(mode)) == E_INVALID
    for bad in (-1, 4):
        assert lib.lccrf_batch_set_pairwise_normalization(b.h, 0, bad) == E_INVALID
    for bad in (np.nan, np.inf):
        m = np.array([[1, 0], [bad, 1]], F32)
        assert lib.lccrf_batch_set_pairwise_compatibility(b.h, 1, p(m)) == E_INVALID
    assert lib.lccrf_batch_get_pairwise_normalization(b.h, 0, None) == E_INVALID
    assert not b.pairwise_compatibility(1)[1] and mode.value == 7  # nothing was set by the refused calls
    mats = fg._dense(2, 2)
    b.set_pairwise_compatibility(1, mats[1])
    b.set_normalization(0, nc.NONE)
    got, is_set = b.get_pairwise_compatibility(1)
    assert is_set and cc.same_bits(got, mats[1]) and b.get_normalization(0) == nc.NONE and b.normalization(1) == nc.AFTER
    b.set_pairwise_compatibility(1, None)
    assert not b.pairwise_compatibility(1)[1]
    b.close()


def _potts_frames(golden, po, wl, F):
    """F frames of 1024 .. 2048 points in turn, c2 first: the shape whose inference runs from prepared launch records"""
    names = ("c2", "N2048", "N1025", "N1024")
    bt = bg.Batch("potts", names, "", golden, po, wl)
    n4, f4, u4 = bt.inputs()
    idx = np.arange(F) % len(names)
    return bt, (n4[idx], [f[idx] for f in f4], u4[idx])


@pytest.mark.gpu
def test_a_matrix_and_a_mode_set_and_taken_back_leave_the_prepared_records_alone(po, wl, golden):
    F = 256
    bt, (n, feats, unary) = _potts_frames(golden, po, wl, F)
    b = pkg.BatchCRF(F, bt.maxN, 2, [2, 2], [float(x) for x in bt.w0])
    b.set_inputs_host(n, feats, unary=unary)
    b.build()
    T, relax = 5, 1.0
    for _ in range(3):                                            # the records are written by the first, read by the others
        b.inference(T, True, relax)
    assert b.engine() == 2
    kept_q, kept_m, runs = b.probability(), b.map(), b.last_prepare()[1]
    potts = bg.traces(bt, "after", relax, 5)
    for f in range(4):
        assert cc.same_bits(kept_q[f, :n[f]], potts[f][T]), f
    # the detour: a matrix on term 0, SYMMETRIC on term 1
    mats, modes = [fg._dense(2, 2)[0], None], [nc.AFTER, nc.SYMMETRIC]
    bg.apply(b, modes, mats)
    b.inference(T, True, relax)
    assert b.engine() == 4 and b.fused_shape() == (1024, 1)
    q = b.probability()
    assert not cc.same_bits(q, kept_q)
    for f in (0, 1, 2, 3, F - 1):
        fr = bt.frames[f % 4]
        want = nc.restate_f32(fr[1], fr[2], [F32(x) for x in bt.w0], mats, modes, T, relax, fr[3])
        assert cc.same_bits(q[f, :n[f]], want), f
    # a new weight between two general inferences
    b.set_pairwise_weight(1, 17.5)
    b.inference(T, True, relax)
    q = b.probability()
    for f in (0, F - 3):
        fr = bt.frames[f % 4]
        want = nc.restate_f32(fr[1], fr[2], [F32(bt.w0[0]), F32(17.5)], mats, modes, T, relax, fr[3])
        assert cc.same_bits(q[f, :n[f]], want), f
    b.set_pairwise_weight(1, float(bt.w0[1]))
    runs_w = b.last_prepare()[1]
    # taken back: the fast engine, the kept bits, and no prepare because of the detour
    bg.apply(b, [nc.AFTER] * 2, [None] * 2)
    for i in range(2):
        b.inference(T, True, relax)
        assert b.engine() == 2
        assert cc.same_bits(b.probability(), kept_q) and np.array_equal(b.map(), kept_m), i
    # (lccrf_batch_set_pairwise_weight invalidates the records, as it always has: at most that one rewrite, none from the setters)
    assert runs_w == runs and b.last_prepare()[1] <= runs + 1, (runs, runs_w, b.last_prepare())
    b.close()


@pytest.mark.gpu
def test_setters_alone_cause_no_prepare(po, wl, golden):
    F = 256
    bt, (n, feats, unary) = _potts_frames(golden, po, wl, F)
    b = pkg.BatchCRF(F, bt.maxN, 2, [2, 2], [float(x) for x in bt.w0])
    b.set_inputs_host(n, feats, unary=unary)
    b.build()
    for _ in range(2):
        b.inference(5, True, 1.0)
    kept, runs = b.probability(), b.last_prepare()[1]
    b.set_normalization(0, nc.BEFORE)
    b.inference(5, True, 1.0)
    assert b.engine() == 4
    b.set_normalization(0, nc.AFTER)
    b.inference(5, True, 1.0)
    assert b.engine() == 2 and cc.same_bits(b.probability(), kept)
    assert b.last_prepare()[1] == runs, (runs, b.last_prepare())
    b.close()


# ---- GPU: until converged ----------------------------------------------------------------------------------------------------------
def _device_i32(addr, n):
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(n, np.int32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), C.c_size_t(4 * n), 2) == 0
    return out


def _check_converged(b, bt, trs, crit, tol, cap, want_engine, tag):
    wants = [cv.expect(tr, crit, tol, cap) for tr in trs]
    rep = b.convergence()
    print(tag, "criterion", crit, "tol", tol, "cap", cap, "iterations", rep["iterations"], "want", [w[0] for w in wants])
    assert b.engine() == want_engine, (tag, b.engine())
    for f, w in enumerate(wants):
        got = {k: v[f] for k, v in rep.items()}
        assert cv.same_report(got, w), (tag, f, got, w)
        if bt.N[f] == 0:
            assert (got["iterations"], got["changed"], got["converged"]) == (0, 0, 0) and got["delta"].view(np.int32) == 0
    bg.check_frames(b, bt, [tr[w[0]] for tr, w in zip(trs, wants)], tag)          # Q, the labels and the bits at the reported t
    d, F = b.device_convergence(), len(trs)
    assert np.array_equal(_device_i32(d["iterations"], F), rep["iterations"])
    assert np.array_equal(_device_i32(d["delta"], F), rep["delta"].view(np.int32))
    assert np.array_equal(_device_i32(d["changed"], F), rep["changed"])
    assert np.array_equal(_device_i32(d["converged"], F), rep["converged"])
    return wants


@pytest.mark.gpu
@pytest.mark.parametrize("bname,sname,relax", bg.CONVERGED)
def test_batch_converges_frame_by_frame_in_one_launch(po, wl, golden, bname, sname, relax):
    bt = bg.batch(bname, golden, po, wl)
    modes, mats, w = bg.setting(bt, sname)
    trs = bg.traces(bt, sname, relax)
    b = bg.make(bt, modes, mats, w)
    for crit, tol, cap in bg.converged_settings(trs, bg.DESIGNATED[bname.split("/")[0]]):
        b.inference_converged(cap, crit, tol, True, relax)
        _check_converged(b, bt, trs, crit, tol, cap, 4, (bname, sname, relax))
        assert b.fused_shape() == (1024, 1)
    b.inference(3, True, relax)                                   # the fixed-count path behind a converged call
    assert b.engine() == 4
    bg.check_frames(b, bt, [tr[3] for tr in trs], (bname, sname, "fixed behind converged"))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bname,sname,relax", [c for c in bg.CONVERGED if c[0] in ("two/", "one/")])
def test_the_streaming_engine_gives_the_same_reports(po, wl, golden, bname, sname, relax):
    bt = bg.batch(bname, golden, po, wl)
    modes, mats, w = bg.setting(bt, sname)
    trs = bg.traces(bt, sname, relax)
    b = bg.make(bt, modes, mats, w, engine=1)
    for crit, tol, cap in bg.converged_settings(trs, bg.DESIGNATED[bname.split("/")[0]]):
        b.inference_converged(cap, crit, tol, True, relax)
        _check_converged(b, bt, trs, crit, tol, cap, 1, (bname, sname, relax, "streaming"))
    b.close()


@pytest.mark.gpu
def test_a_handle_sized_batch_takes_the_kernel_and_the_sparse_plan_has_room(po, wl, golden):
    one = bg.Batch("single", ("c2",), "", golden, po, wl)
    modes, mats, w = bg.setting(one, "mixed")
    trs = bg.traces(one, "mixed", 1.0)
    b = bg.make(one, modes, mats, w, max_frames=1)
    b.inference_converged(bg.CAP, cv.LABELS, 0.0, True, 1.0)
    _check_converged(b, one, trs, cv.LABELS, F32(0), bg.CAP, 4, "max_frames = 1")
    b.close()
    sp = bg.batch("sparse+N1025", golden, po, wl)                 # one shared product buffer: the loop's other form
    modes, mats, w = bg.setting(sp, "mixed")
    trs = bg.traces(sp, "mixed", 0.5)
    b = bg.make(sp, modes, mats, w)
    for crit, tol, cap in ((cv.LABELS, F32(0), bg.CAP), (cv.DELTA, F32(1e-2), bg.CAP), (cv.LABELS, F32(0), 2)):
        b.inference_converged(cap, crit, tol, True, 0.5)
        _check_converged(b, sp, trs, crit, tol, cap, 4, ("sparse+N1025", crit, cap))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sites,engine", [(cv.EDGE_FULL, 1), (cv.EDGE_ROOM, 4)], ids=["full", "room"])
def test_a_plan_without_room_for_the_reductions_words_streams(po, sites, engine):
    """three frames -- the frame whose plan fills the workgroup's LDS to the byte (tests/converge_cases.py: edge_problem; or the one
    96 bytes short of it), its first five points, the frame again -- with a matrix and the SYMMETRIC mode on the first term: k_general
    takes the batch either way (lccrf_batch_inference: engine 4); k_general_converge takes it only with 16 bytes to spare -- without
    them its launcher returns 0 and the converged call runs on the streaming step (engine 1), with the same results"""
    pb = cv.edge_problem(sites)
    modes, mats = [nc.SYMMETRIC, nc.AFTER], [(np.eye(2) + 0.3 * np.random.default_rng(5).standard_normal((2, 2))).astype(F32), None]
    w = [F32(x) for _, x in pb["kernels"]]
    N = np.array([cv.EDGE_N, 5, cv.EDGE_N], np.int32)
    maxN = cv.EDGE_N + bg.MAX_POINTS_SLACK
    feats, unary, frames = [np.zeros((3, maxN, 2), F32) for _ in range(2)], np.zeros((3, maxN, 2), F32), {}
    for n in (cv.EDGE_N, 5):
        p = dict(pb, N=n, label=pb["label"][:n], kernels=[(f[:n], x) for f, x in pb["kernels"]])
        o = cc.setup(po.OracleCRF, p)
        frames[n] = (o.unary(), nc.feats(p), [o.kernel(k)["norm"] for k in range(2)])
        o.close()
    for f, n in enumerate(N):
        unary[f, :n] = frames[n][0]
        for k in range(2):
            feats[k][f, :n] = frames[n][1][k]
    b = pkg.BatchCRF(3, maxN, 2, [2, 2], [float(x) for x in w])
    bg.apply(b, modes, mats)
    b.set_inputs_host(N, feats, unary=unary)
    b.build()
    shape = types.SimpleNamespace(N=N)                            # (what _check_converged and check_frames read of a Batch)
    for relax in cv.RELAX:
        trs = [nc.restate_trace_f32(frames[n][0], frames[n][1], w, mats, modes, bg.CAP, relax, frames[n][2]) for n in N]
        for crit, tol, cap in ((cv.LABELS, F32(0), bg.CAP), (cv.DELTA, F32(1e-3), bg.CAP), (cv.DELTA, F32(0), 2)):
            b.inference_converged(cap, crit, tol, True, relax)
            _check_converged(b, shape, trs, crit, tol, cap, engine, (sites, crit, cap, relax))
    b.inference(2, True, 1.0)                                     # the fixed count on the same lattices: k_general takes both
    assert b.engine() == 4 and b.fused_shape() == (1024, 1)
    bg.check_frames(b, shape, [nc.restate_trace_f32(frames[n][0], frames[n][1], w, mats, modes, 2, 1.0, frames[n][2])[2] for n in N], sites)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REACH))
def test_one_point_decides_wherever_it_sits(po, wl, golden, name):
    """tol lies between the largest and the second-largest per-point change at iteration t: a reduction that dropped the point -- in
    the first wavefront, the last wavefront with a point, the last slot, at index N - 1 -- would stop at t, one too early.  The frame
    sits in a batch of four whose other frames stop elsewhere."""
    _, cases = _reach(po, wl, name)
    for tname, case in cases.items():
        if case is None:
            continue
        pb2, (U, ft, nrm, w, modes, mats, tr), t, point, tol = case
        others = [bg.base(o, golden, po, wl) for o in REACH_OTHERS]
        frames = [(pb["N"], Uo, nc.feats(pb), no) for pb, Uo, no, _, _ in others]
        frames.insert(1, (pb2["N"], U, ft, nrm))
        trs = [nc.restate_trace_f32(fr[1], fr[2], w, mats, modes, bg.CAP, 1.0, fr[3]) if i != 1 else tr
               for i, fr in enumerate(frames)]
        bt = bg.Batch.__new__(bg.Batch)
        bt.name, bt.K, bt.frames = "reach", 2, frames
        bt.N = np.array([fr[0] for fr in frames], np.int32)
        bt.maxN = int(bt.N.max()) + bg.MAX_POINTS_SLACK
        b = bg.make(bt, modes, mats, w)
        b.inference_converged(bg.CAP, cv.DELTA, tol, True, 1.0)
        wants = _check_converged(b, bt, trs, cv.DELTA, tol, bg.CAP, 4, (name, tname, point))
        assert wants[1][0] > t, (tname, wants[1], t)              # at t and not at t - 1 ... i.e. not where the run without the point stops
        assert any(x[0] != wants[1][0] for i, x in enumerate(wants) if i != 1), wants
        b.close()


# ---- GPU: run and run_converged; the refused gradients ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_run_and_run_converged_are_build_plus_inference(po, wl, golden):
    bt = bg.batch("one/", golden, po, wl)
    modes, mats, w = bg.setting(bt, "matrices")
    relax = 0.5
    trs = bg.traces(bt, "matrices", relax)
    b = bg.make(bt, modes, mats, w, build=False)
    b.run(5, True, relax)
    bg.check_frames(b, bt, [tr[5] for tr in trs], "run")
    assert b.engine() == 4 and b.fallback_frames() == 0
    twin = bg.make(bt, modes, mats, w)
    twin.inference(5, True, relax)
    assert cc.same_bits(b.probability(), twin.probability()) and np.array_equal(b.map(), twin.map())
    for crit, tol, cap in ((cv.LABELS, F32(0), bg.CAP), (cv.DELTA, F32(1e-2), 4)):
        b.run_converged(cap, crit, tol, True, relax)
        _check_converged(b, bt, trs, crit, tol, cap, 4, ("run_converged", crit))
        assert b.fallback_frames() == 0
        twin.inference_converged(cap, crit, tol, True, relax)
        r1, r2 = b.convergence(), twin.convergence()
        assert all(np.array_equal(r1[k].view(np.int32), r2[k].view(np.int32)) for k in r1)
    b.close(), twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("matrix", "mode"))
def test_gradients_of_such_a_batch_are_refused_and_leave_it_as_it_was(po, wl, golden, what):
    bt = bg.batch("one/", golden, po, wl)
    mats = [fg._dense(2, 2)[0], None] if what == "matrix" else [None, None]
    modes = [nc.AFTER, nc.AFTER] if what == "matrix" else [nc.AFTER, nc.BEFORE]
    w = [F32(x) for x in bt.w0]
    b = bg.make(bt, modes, mats, w)
    b.inference(3, True, 1.0)
    q, m = b.probability(), b.map()
    F = len(bt.frames)
    G = dev(np.random.default_rng(4).standard_normal((F, bt.maxN, 2)).astype(F32))
    gu, gw = dev(np.zeros((F, bt.maxN, 2), F32)), dev(np.zeros((F, 2), F32))
    gf = [dev(np.zeros((F, bt.maxN, 2), F32)) for _ in range(2)]
    with pytest.raises(pkg.LccrfError) as e1:
        b.inference_backward_device(3, 1.0, G.data_ptr(), gu.data_ptr(), gw.data_ptr())
    with pytest.raises(pkg.LccrfError) as e2:
        b.inference_backward_features_device(3, 1.0, G.data_ptr(), gu.data_ptr(), gw.data_ptr(), [x.data_ptr() for x in gf])
    assert e1.value.code == e2.value.code == E_STATE
    assert float(gu.abs().max()) == 0.0 and all(float(x.abs().max()) == 0.0 for x in gf)      # nothing was written
    assert cc.same_bits(b.probability(), q) and np.array_equal(b.map(), m)
    b.inference(3, True, 1.0)
    assert b.engine() == 4 and cc.same_bits(b.probability(), q)
    trs = [nc.restate_f32(fr[1], fr[2], w, mats, modes, 3, 1.0, fr[3]) if fr else np.zeros((0, 2), F32) for fr in bt.frames]
    bg.check_frames(b, bt, trs, ("behind the refusal", what))
    bg.apply(b, [nc.AFTER] * 2, [None] * 2)                       # the Potts batch differentiates as it always has
    b.inference_backward_device(3, 1.0, G.data_ptr(), gu.data_ptr(), gw.data_ptr())
    b.synchronize()
    assert float(gu.abs().max()) > 0.0
    b.close()

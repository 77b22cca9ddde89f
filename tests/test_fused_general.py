"""The fused engine's kernel for terms with a label-compatibility matrix or a normalisation mode (csrc/fused_general.hip): a handle's
two-label frame of up to 2048 points with such terms runs lccrf_inference in one launch, and lccrf_get_engine says so.

CPU: which row path and how many points per lane every case is there for, from the oracle's lattices.  GPU: lccrf_inference against
the float32 restatement of tests/normalization_checker.py, bit for bit on Q, the labels against compat_checker.map_of, and against
lccrf_start_inference + T x lccrf_step_inference on the same handle (the streaming engine); the engine reports; the cases beyond the
kernel's range; the torch layer."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import compat_checker as ck
import crf_cases as cc
import grad_support as gs
import gradient_settings as gset
import normalization_checker as nc
from abi_support import lib  # noqa: F401

pkg = importlib.import_module("lc-crf-slam_amd")
E_INVALID = -1
LANES, MAX_POINTS = 1024, 2048


def _dense(K, L, seed=77):
    """I + 0.3 N(0, 1), seeded as in tests/test_normalization.py"""
    rng = np.random.default_rng([seed, K, L])
    return [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]


def _terms(pb, order):
    return dict(pb, kernels=[pb["kernels"][k] for k in order])


def _problem(name, golden, po, wl):
    """appearance = the SLAM frame's first term (a hundred-odd vertices, rows of hundreds of products from ~1000 points on: chain
    rows), smooth = its second (about one vertex per two points: short rows)"""
    if name == "slam:N1001":
        return cc.golden_problem(golden, name)
    if name == "c2":
        return wl.slam_problem(2000, seed=12)
    if name == "sparse:N1100":                                   # every point of the first term in a lattice cell of its own: V = 3 N
        return cc.shaped_problem(wl, 1100, "sparse", 5)
    base, _, terms = name.partition("/")
    pb = wl.slam_problem(int(base[1:]), seed=21) if base != "c2" else wl.slam_problem(2000, seed=12)
    return _terms(pb, {"": [0, 1], "appearance": [0], "smooth": [1], "smooth_first": [1, 0]}[terms])


# name: (points per lane, kernel 0 on chain rows) the case is there for; None: beyond the kernel's range
CASES = {
    "N5": (1, 0), "N7": (1, 0),                      # N % 4 != 0: phantom vertices; most lanes idle
    "slam:N1001": (1, 1),                            # one point per lane
    "N1025": (2, 1),                                 # the first two-points-per-lane frame: lane 0 alone has a second point
    "c2": (2, 1),                                    # 2000 points
    "N2048": (2, 1),                                 # the last frame the kernel takes
    "N2049": None,
    "c2/appearance": (2, 1), "N1001/smooth": (1, 0),  # K = 1: each of the two terms on its own
    "c2/smooth_first": (2, 0),                       # K = 2, kernel 0 with short rows
}
# ... and the instantiations those leave out, run in the mixed setting only
EXTRA = {"N1001/appearance": (1, 1), "c2/smooth": (2, 0), "N1001/smooth_first": (1, 0),
         "sparse:N1100": (2, 0)}                     # lattices so large that both terms' products share ONE buffer in LDS


def _own_product_buffers(N, V, chain0):
    """csrc/fused_loop.h: layout_core -- does the plan with a product buffer per term fit the 160 KiB of LDS?  (bytes, 16-aligned)"""
    a16 = lambda b: (b + 15) & ~15
    total = 128 + 64
    for k, v in enumerate(V):
        floats = (N * 3 + (14 * v + 16 if k == 0 and chain0 else 0) + 63) & ~63
        total += 2 * a16((v + 1) * 8) + a16(3 * v * 4) + a16((v + 2) * 2) + a16(floats * 8)
    return total <= 160 * 1024


_PREPARED = {}


def _prepared(name, golden, po, wl):
    """(problem, raw unary, norms, (V0, longest row of kernel 0, every V)) of a case: computed once, shared by the tests, never changed"""
    if name not in _PREPARED:
        pb = _problem(name, golden, po, wl)
        o = cc.setup(po.OracleCRF, pb)
        U = o.unary()
        ks = [o.kernel(k) for k in range(len(pb["kernels"]))]
        o.close()
        row0 = int(np.bincount(ks[0]["offset"].reshape(-1), minlength=ks[0]["V"]).max())
        _PREPARED[name] = (pb, U, [k["norm"] for k in ks], (ks[0]["V"], row0, [k["V"] for k in ks]))
    return _PREPARED[name]


def _settings(K):
    """name -> (modes, matrices): every mode on every term without matrices, matrices on every term, and one mixed setting"""
    out = {nc.MODE_NAMES[m]: ([m] * K, [None] * K) for m in nc.MODES}
    out["matrices"] = ([nc.AFTER] * K, _dense(K, 2))
    out["mixed"] = ([nc.SYMMETRIC, nc.BEFORE][:K], [_dense(K, 2)[0], None][:K])
    return out


SETTINGS = list(_settings(2))


def _handle(pb, weights, modes, mats):
    h = cc.setup(pkg.DenseCRFHIP, dict(pb, kernels=[(f, w) for (f, _), w in zip(pb["kernels"], weights)]))
    for k, m in enumerate(modes):
        h.set_normalization(k, m)
    for k, m in enumerate(mats):
        if m is not None:
            h.set_pairwise_compatibility(k, m)
    return h


def _shape(word):
    return word & 0xffff, (word >> 16) & 15, (word >> 20) & 1


def _check_engine(h, pb, general, want):
    engine, word = h.engine()
    if not general:
        assert engine in (2, 3), engine                          # a Potts, all-AFTER handle keeps the fast engines
        assert word == 0 or _shape(word)[0] in (512, LANES)
    elif pb["N"] <= MAX_POINTS:
        assert engine == 4, (engine, word)
        assert _shape(word) == (LANES,) + want, (_shape(word), want)
    else:
        assert (engine, word) == (1, 0), (engine, word)


def _run_setting(name, setting, golden, po, wl, want):
    pb, U, nrm, _ = _prepared(name, golden, po, wl)
    K = len(pb["kernels"])
    modes, mats = _settings(K)[setting]
    general = any(m != nc.AFTER for m in modes) or any(m is not None for m in mats)
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes, mats)
    for relax in (1.0, 0.7):
        trace = nc.restate_trace_f32(U, nc.feats(pb), w, mats, modes, 5, relax, nrm)
        for T in (0, 1, 5):
            h.inference(T, True, relax)
            q = h.probability()
            assert cc.same_bits(q, trace[T]), (name, setting, T, relax, float(np.abs(q - trace[T]).max()))
            assert np.array_equal(h.map(), ck.map_of(trace[T])), (name, setting, T, relax)
            _check_engine(h, pb, general, want)
            h.start_inference()                                  # the step path stays on the streaming engine
            for _ in range(T):
                h.step_inference(relax)
            assert cc.same_bits(h.probability(), q), (name, setting, T, relax)
    h.close()


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_cases_are_there_for_both_row_paths_and_both_points_per_lane(po, wl, golden):
    """csrc/fused_loop.h: kernel 0 takes chain rows when its longest splat row has at least 64 products and it has at most 464
    vertices (chain_wanted; the u16 slot bound holds for every frame of this size); a lane owns ceil(N / 1024) points."""
    seen = set()
    for name, want in {**CASES, **EXTRA}.items():
        pb, _, _, (V0, row0, V) = _prepared(name, golden, po, wl)
        if want is None:
            assert pb["N"] == MAX_POINTS + 1
            continue
        got = ((pb["N"] + LANES - 1) // LANES, int(row0 >= 64 and V0 <= 464))
        assert got == want, (name, got, want, V0, row0)
        assert _own_product_buffers(pb["N"], V, got[1]) == (name != "sparse:N1100"), (name, V)
        seen.add((len(pb["kernels"]),) + got)
    assert seen == {(k, p, ch) for k in (1, 2) for p in (1, 2) for ch in (0, 1)}      # the kernel's eight instantiations
    assert _prepared("N1025", golden, po, wl)[0]["N"] % LANES == 1 and _prepared("N5", golden, po, wl)[0]["N"] % 4 == 1


def test_lattices_lie_on_both_sides_of_the_prologues_register_rounds(po, wl, golden):
    """the self-contained prologue (csrc/fused_prologue.inc, included by k_general) keeps the neighbour table of up to 4096 / 3 = 1365 vertices and the row pointers of up to 2047 in
    registers; two copy loops take what lies beyond: sparse:N1100 is there for both, every other case stays within both"""
    V = {name: _prepared(name, golden, po, wl)[3][2] for name in {**CASES, **EXTRA}}
    assert V["sparse:N1100"][0] > 2047 and V["sparse:N1100"][1] <= 1365, V["sparse:N1100"]
    assert all(max(v) <= 1365 for name, v in V.items() if name != "sparse:N1100"), V


def test_the_prologues_text_lives_in_one_file():
    """k_fused, k_converge, k_general and k_general_converge include one text: the line that sizes its register rounds is in no other file"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lc-crf-slam_amd", "csrc")
    marker = "constexpr int kNbrRounds = 4096 / NT"
    holders = sorted(n for n in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, n)) and marker in open(os.path.join(csrc, n), errors="replace").read())
    assert holders == ["fused_prologue.inc"], holders


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", list(CASES))
def test_inference_is_the_restatement_and_the_step_path(po, wl, golden, name, setting):
    _run_setting(name, setting, golden, po, wl, CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXTRA))
def test_remaining_instantiations_in_the_mixed_setting(po, wl, golden, name):
    _run_setting(name, "mixed", golden, po, wl, EXTRA[name])


@pytest.mark.gpu
def test_shape_words_reach_both_row_paths_and_both_points_per_lane(po, wl, golden):
    """one inference with matrices per case: the shape words of the whole set, as the kernel's launcher reports them"""
    seen = set()
    for name, want in {**CASES, **EXTRA}.items():
        pb, _, nrm, _ = _prepared(name, golden, po, wl)
        K = len(pb["kernels"])
        h = _handle(pb, nc.weights_f32(pb, nrm, [nc.AFTER] * K), [nc.AFTER] * K, _dense(K, 2))
        h.inference(1, False, 1.0)
        engine, word = h.engine()
        h.close()
        if want is None:
            assert (engine, word) == (1, 0), (name, engine, word)
            continue
        assert engine == 4 and _shape(word)[0] == LANES, (name, engine, word)
        seen.add((K,) + _shape(word)[1:])
    assert {s[1] for s in seen} == {1, 2} and {s[2] for s in seen} == {0, 1}, seen
    assert seen == {(k, p, ch) for k in (1, 2) for p in (1, 2) for ch in (0, 1)}, seen


@pytest.mark.gpu
def test_matrix_and_modes_set_and_taken_back_return_the_fast_engines_and_their_bits(po, wl, golden, lib):
    pb, _, _, _ = _prepared("slam:N1001", golden, po, wl)
    fresh, h = cc.setup(pkg.DenseCRFHIP, pb), cc.setup(pkg.DenseCRFHIP, pb)
    assert h.engine() == (1, 0)                                  # nothing has run yet
    assert lib.lccrf_get_engine(h.h, None, None) == E_INVALID
    e = C.c_int(0)
    assert lib.lccrf_get_engine(h.h, C.byref(e), None) == 0 and e.value == 1
    fresh.inference(5, True, 0.7)
    assert fresh.engine()[0] in (2, 3)
    mats = _dense(2, 2)
    h.set_pairwise_compatibility(0, mats[0])
    h.set_normalization(1, nc.SYMMETRIC)
    h.inference(5, True, 0.7)
    assert h.engine()[0] == 4 and not cc.same_bits(h.probability(), fresh.probability())
    h.set_normalization(1, nc.AFTER)
    h.inference(5, True, 0.7)
    assert h.engine()[0] == 4                                    # the matrix is still there
    h.set_pairwise_compatibility(0, None)
    for T, relax in ((5, 0.7), (3, 1.0), (0, 1.0)):
        fresh.inference(T, True, relax)
        h.inference(T, True, relax)
        assert h.engine()[0] in (2, 3), h.engine()
        assert cc.same_bits(h.probability(), fresh.probability()) and np.array_equal(h.map(), fresh.map()), (T, relax)
    h.close(), fresh.close()


@pytest.mark.gpu
def test_three_labels_one_dimension_with_a_matrix_stay_on_the_streaming_engine(po, wl, golden):
    pb = cc.golden_problem(golden, "generic:d1_L3")
    K, L = len(pb["kernels"]), pb["L"]
    o = cc.setup(po.OracleCRF, pb)
    U, nrm = o.unary(), [o.kernel(k)["norm"] for k in range(K)]
    o.close()
    mats, modes = _dense(K, L), [nc.AFTER] * K
    w = nc.weights_f32(pb, nrm, modes)
    h = _handle(pb, w, modes, mats)
    for T, relax in ((5, 1.0), (1, 0.7)):
        ref = nc.restate_f32(U, nc.feats(pb), w, mats, modes, T, relax, nrm)
        h.inference(T, True, relax)
        assert h.engine() == (1, 0)
        assert cc.same_bits(h.probability(), ref) and np.array_equal(h.map(), ck.map_of(ref)), (T, relax)
    h.close()


@pytest.mark.gpu
def test_compat_layer_forward_is_the_restatement_and_its_backward_matches_the_checker(po, wl, golden):
    """CompatMeanFieldCRF on slam:N1001, T = 5, relax 0.7: the forward runs on the new kernel, the backward replays on the step path
    -- on the bar of tests/grad_support.py (max(1e-4, 10 x the float32 checker's own error), floors included) against
    compat_checker.gradients_f64."""
    import torch
    ag = importlib.import_module("lc-crf-slam_amd.autograd")
    pb, U, nrm, _ = _prepared("slam:N1001", golden, po, wl)
    K, L, N, T, relax = 2, 2, pb["N"], 5, 0.7
    w0 = [float(w) for _, w in pb["kernels"]]
    mats = _dense(K, L)
    layer = ag.CompatMeanFieldCRF(N, L, nc.feats(pb), w0, n_iterations=T, relax=relax)
    with torch.no_grad():
        layer.compat.copy_(torch.from_numpy(np.stack(mats)))
    u = torch.from_numpy(U).cuda().requires_grad_(True)
    G = np.random.default_rng(2).standard_normal((N, L))
    q = layer(u)
    torch.cuda.synchronize()
    assert layer.crf.engine()[0] == 4
    ref = nc.restate_f32(U, nc.feats(pb), [np.float32(x) for x in w0], mats, [nc.AFTER] * K, T, relax, nrm)
    assert cc.same_bits(q.detach().cpu().numpy(), ref)
    q.backward(torch.from_numpy(G.astype(np.float32)).cuda())
    torch.cuda.synchronize()
    got = (u.grad.cpu().numpy(), layer.weights.grad.numpy(), layer.compat.grad.numpy())
    o, lats, U64 = gs.checker(po, pb)
    o.close()
    at = gset.device_iterates(po, pb, T, relax, mats)            # (the fixture's bars need it: tests/gradient_settings.py, LINEARISED)
    gs.compat_reference(U64, np.array(w0), mats, lats, T, relax, G, "layer", at=at).check(dict(zip(("dL/dU", "dL/dw", "dL/dmu"), got)))
    layer.close()

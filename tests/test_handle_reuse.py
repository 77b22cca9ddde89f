"""What a handle forgets when it is parked, and what a batch reports of its last run (csrc/host_engine.h: Engine::Options,
Engine::RunReport, Engine::LearntModel; notes/host_state.md).

The frames are the smallest with two terms: 64 points, 2 labels, two 2-D terms (workloads.slam_problem), 2 iterations."""
import importlib

import numpy as np
import pytest

import batch_cases as bc
import crf_cases as cc
import grad_support as gs

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

N, T = 64, 2
STREAM = pkg.BACKWARD_STREAM


def _grad(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _run(h, K):
    """inference(2, True) and a backward call: (Q, labels, dL/dU, dL/dw, engine, backward route)"""
    h.inference(T, True)
    q, m = h.probability(), h.map()
    e = h.engine()
    gu, gw = gs.backward(h, T, 1.0, _grad((N, 2), 5), K)
    return q, m, gu, gw, e, h.backward_route()


def test_a_parked_handle_comes_back_as_a_fresh_one(wl):
    pb = wl.slam_problem(N, seed=11)
    K = len(pb["kernels"])
    assert K == 2 and pb["L"] == 2 and all(f.shape[1] == 2 for f, _ in pb["kernels"])
    pkg.lib().lccrf_trim_cache()
    # a user who leaves nothing at its default
    h = pkg.DenseCRFHIP(N, 2)
    for option, value in ((pkg.OPT_SINGLE_WORKGROUP, 1), (pkg.OPT_FRAME_GENERAL, 1), (pkg.OPT_FUSED_BACKWARD, 1), (pkg.OPT_VERTEX_ORDER, 2)):
        h.set_option(option, value)
    h.set_unary_from_label(pb["label"], pb["conf"])
    for f, w in pb["kernels"]:
        h.add_pairwise(f, w)
    h.set_pairwise_compatibility(0, [[0.0, 1.5], [0.5, 0.25]])
    h.set_normalization(1, pkg.NORMALIZE_SYMMETRIC)
    h.inference(T, True)
    h.map()
    assert h.engine() == (3, 0), h.engine()                          # (option 5: the learnt model in one launch)
    gs.backward(h, T, 1.0, _grad((N, 2), 5), K)
    h.inference(T, True)                                             # (the backward left the lattices in HBM: the general kernel)
    engine, shape = h.engine()
    assert engine == 4 and shape != 0 and h.backward_route() == STREAM, (engine, shape, h.backward_route())
    address = h.h.value
    h.close()
    # the next user of the same size gets the same object ...
    h = pkg.DenseCRFHIP(N, 2)
    assert h.h.value == address, "the parked handle was not handed out again: the test proves nothing"
    # ... which reports nothing of the last one's runs, and holds nothing of its model
    assert h.engine() == (1, 0) and h.backward_route() == pkg.BACKWARD_NONE, (h.engine(), h.backward_route())
    h.set_unary_from_label(pb["label"], pb["conf"])
    for f, w in pb["kernels"]:
        h.add_pairwise(f, w)
    for k in range(K):
        m, is_set = h.get_pairwise_compatibility(k)
        assert not is_set and np.array_equal(m, np.eye(2, dtype=np.float32)), (k, is_set, m)
        assert h.get_normalization(k) == pkg.NORMALIZE_AFTER, k
    got = _run(h, K)
    # ... and runs as a handle that was never used does
    pkg.lib().lccrf_trim_cache()
    fresh = cc.setup(pkg.DenseCRFHIP, pb)
    want = _run(fresh, K)
    for name, a, b in zip(("Q", "labels", "dL/dU", "dL/dw"), got, want):
        assert cc.same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b), name
    assert got[4] == want[4] and got[5] == want[5], (got[4:], want[4:])
    assert got[5] == STREAM and want[5] == STREAM, "LCCRF_OPT_FUSED_BACKWARD leaked into the next user's handle"
    h.close()
    fresh.close()


# What the parent of the commit that introduced Engine::RunReport answered to the sequence below, on the MI355X: per stage
# (engine, fused_shape, fallback_frames, backward_route).  Written down from a run of report_sequence() against that build.
PARENT_REPORT = {
    "created": (1, (0, 0), 0, 0),
    "build + inference": (2, (1024, 1), 0, 0),
    "run": (3, (1024, 1), 0, 0),
    "run_converged": (3, (1024, 1), 0, 0),
    "backward": (3, (1024, 1), 0, 1),
    "build + inference_converged": (2, (1024, 1), 0, 1),
}


def report_sequence(wl):
    """{stage: [first answers, second answers]} of a batch of 3 frames of 64 points"""
    fr = bc.Frames([wl.slam_problem(N, seed=21 + f) for f in range(3)], [wl.TUM3["w1"], wl.TUM3["w2"]])
    b = fr.batch(build=False)
    out = {}

    def ask_each_twice(stage):
        """every getter twice in a row (not the four in turn): the second answer of each beside its first"""
        pairs = [(g(), g()) for g in (b.engine, b.fused_shape, b.fallback_frames, b.backward_route)]
        out[stage] = [tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)]

    ask_each_twice("created")
    b.build()
    b.inference(T, True)
    ask_each_twice("build + inference")
    b.run(T, True)
    ask_each_twice("run")
    b.run_converged(10)
    ask_each_twice("run_converged")
    gs.batch_backward(b, T, 1.0, fr.grad_prob(3), fr.K)
    ask_each_twice("backward")
    b.build()                                                        # (lattices in HBM and a converged run: the getter's two rules at once)
    b.inference_converged(10)
    ask_each_twice("build + inference_converged")
    b.close()
    return out


def test_the_report_of_a_batch(wl):
    got = report_sequence(wl)
    print("report of a batch:", got)
    assert list(got) == list(PARENT_REPORT)
    for stage, (first, second) in got.items():
        assert second == first, (stage, first, second)
        assert first == PARENT_REPORT[stage], (stage, first, PARENT_REPORT[stage])

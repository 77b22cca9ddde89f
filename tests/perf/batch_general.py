#!/usr/bin/env python3
"""Time of a batch of c2 frames (2000 points, two 2-D terms, two labels; 64 distinct frames, workloads.slam_problem) whose terms carry
label-compatibility matrices I + 0.3 N(0, 1) on both terms ("matrices") or the mixed setting of tests/test_fused_general.py
(SYMMETRIC with a matrix on the first term, BEFORE on the second): include/lccrf.h section 2g, csrc/fused_general.hip and
csrc/fused_general_converge.hip.  Per batch size (256 and 4096 frames) and setting, microseconds per call:

    potts_fixed5          lccrf_batch_inference(5) without matrices or modes: the Potts lean shape, for context
    general_fixed5        lccrf_batch_inference(5) with them: one launch, a workgroup per frame (engine 4)
    stream_fixed5         the same batch under lccrf_batch_set_engine(1): the streaming step, what the one launch replaces
    general_converged12   lccrf_batch_inference_converged(12, LCCRF_STOP_LABELS) in one launch (engine 4)
    stream_converged12    ... and on the streaming step with the bookkeeping behind it (engine 1)
    handles_fixed5        256 handles holding the first 256 frames, lccrf_inference(5) called one after another and then waited for:
                          what a user without the batch setters does (host clock: the handles have a stream each)

HIP events on the batch's stream around `--reps` calls, warm-up calls first, the variants in turn `--rounds` times over; median with
[min .. max].  Prints one JSON line.  Run by hand on the GPU box; not collected by pytest, not called by bench.py.

    python tests/perf/batch_general.py [--frames 256 4096] [--reps 20] [--rounds 9]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--handles", type=int, default=256)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    N, K, L, T, CAP = 2000, 2, 2, 5, 12
    pbs = [wl.slam_problem(N, seed=1 + i) for i in range(a.distinct)]
    w = [float(x) for _, x in pbs[0]["kernels"]]
    rng = np.random.default_rng([77, K, L])
    dense = [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]
    settings = {"matrices": ([pkg.NORMALIZE_AFTER] * K, dense),
                "mixed": ([pkg.NORMALIZE_SYMMETRIC, pkg.NORMALIZE_BEFORE], [dense[0], None])}
    potts = ([pkg.NORMALIZE_AFTER] * K, [None] * K)

    def arm(c, setting):
        for k in range(K):
            c.set_normalization(k, setting[0][k])
            c.set_pairwise_compatibility(k, setting[1][k])

    stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
    out = dict(shape="c2: N=2000 L=2 K=2, %d distinct frames" % a.distinct, reps=a.reps, rounds=a.rounds, batches={})
    for F in a.frames:
        idx = [i % a.distinct for i in range(F)]
        feats = [np.stack([pbs[i]["kernels"][k][0] for i in idx]) for k in range(K)]
        label = np.stack([pbs[i]["label"] for i in idx])
        batches = {}
        for engine in (0, 1):
            b = pkg.BatchCRF(F, N, L, [2] * K, w)
            b.set_engine(engine)
            b.set_inputs_host([N] * F, feats, label=label, conf=pbs[0]["conf"])
            b.build()
            batches[engine] = b
        fused, stream = batches[0], batches[1]
        res = {}
        for sname, setting in settings.items():
            variants = {
                "potts_fixed5": (fused, potts, lambda: fused.inference(T, True, 1.0)),
                "general_fixed5": (fused, setting, lambda: fused.inference(T, True, 1.0)),
                "stream_fixed5": (stream, setting, lambda: stream.inference(T, True, 1.0)),
                "general_converged12": (fused, setting, lambda: fused.inference_converged(CAP, pkg.STOP_LABELS, 0.0, True, 1.0)),
                "stream_converged12": (stream, setting, lambda: stream.inference_converged(CAP, pkg.STOP_LABELS, 0.0, True, 1.0)),
            }
            engines, ev = {}, {}
            for name, (b, st, call) in variants.items():          # warm-up of every variant
                arm(b, st)
                for _ in range(3):
                    call()
                b.synchronize()
                engines[name] = [b.engine(), list(b.fused_shape())]
            it = fused.convergence()["iterations"]
            for _ in range(a.rounds):
                for name, (b, st, call) in variants.items():
                    arm(b, st)
                    call()
                    b.synchronize()
                    ev.setdefault(name, []).append(timed(b.own_stream(), call, a.reps))
                    b.synchronize()
            res[sname] = dict(engine_and_shape=engines, event_us_per_call={k: stat(v) for k, v in ev.items()},
                              iterations={int(t): int(n) for t, n in zip(*np.unique(it, return_counts=True))})
        for b in batches.values():
            b.close()
        out["batches"][str(F)] = res
    # the same frames one handle at a time
    hs = []
    for i in range(a.handles):
        pb = pbs[i % a.distinct]
        h = pkg.DenseCRFHIP(N, L)
        h.set_unary_from_label(pb["label"], pb["conf"])
        for f, x in pb["kernels"]:
            h.add_pairwise(f, x)
        hs.append(h)
    out["handles"] = {}
    for sname, setting in settings.items():
        for h in hs:
            arm(h, setting)
        wall = []
        for r in range(3 + a.rounds):
            t0 = time.perf_counter()
            for h in hs:
                h.inference(T, True, 1.0)
            for h in hs:
                h.synchronize()
            if r >= 3:
                wall.append((time.perf_counter() - t0) * 1e6)
        out["handles"][sname] = dict(handles=len(hs), engine=list(hs[0].engine()), wall_us_all_handles_fixed5=stat(wall))
    for h in hs:
        h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

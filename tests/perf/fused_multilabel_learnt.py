#!/usr/bin/env python3
"""Time of lccrf_inference(5, with_map) on built lattices for frames of three to eight labels under a LEARNT model -- the SLAM
frame's two terms, a label-compatibility matrix on both, term 1 normalised SYMMETRICally -- with LCCRF_MULTILABEL_LEARNT on (one
launch, csrc/fused_multilabel_general.hip, engine 6 where the plan takes the frame) against off (the parent's route for these frames:
the streaming engine, engine 1), on the same build: one handle per (points, labels), the frame of tests/fused_multilabel_cases.py with
raw unaries.  Beside them the floor: Potts k_multilabel (engine 5) on the same frame.  Then a batch of `--frames` frames of 2000
points at four labels through lccrf_batch_inference, both ways (lccrf_batch_last_timing's events).

HIP events on the handle's stream around `--reps` calls, after warm-up calls; the routes take turns, `--runs` times over: the median
of the runs' figures with [min .. max], the spread the acceptance rule of notes/fused_multilabel.md section 6 is read against.
Prints one JSON line.  Run by hand on the GPU box; not collected by pytest, not called by bench.py.

    python tests/perf/fused_multilabel_learnt.py [--reps 20] [--runs 3] [--frames 1024]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fused_multilabel_cases as mc  # noqa: E402
import fused_multilabel_learnt_cases as lc  # noqa: E402
import normalization_checker as nc  # noqa: E402

T = 5
MODES = (nc.AFTER, nc.SYMMETRIC)
ROUTES = {"off": 0, "on": lc.LEARNT, "potts": lc.POTTS}


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def put_model(h, L, on):
    """the learnt model (on) or the Potts model normalised AFTER"""
    for k in range(2):
        h.set_pairwise_compatibility(k, lc.matrix(L, k) if on else None)
        h.set_normalization(k, MODES[k] if on else nc.AFTER)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1024)
    a = ap.parse_args()
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    out = dict(reps=a.reps, runs=a.runs, T=T, handles={}, batch={})

    def arm(h, L, r):
        put_model(h, L, r != "potts")
        h.set_multilabel_routes(ROUTES[r])

    for N in (500, 1000, 2000):
        for L in (3, 4, 6, 8):
            pb = mc.problem(wl, N=N, L=L)
            h = pkg.DenseCRFHIP(N, L)
            h.set_unary(pb["unary"])
            for f, w in pb["kernels"]:
                h.add_pairwise(f, w)
            call = lambda: h.inference(T, True, 1.0)
            res = {r: [] for r in ROUTES}
            engines = {}
            for r in ROUTES:                                     # warm-up of every route (the first call builds the lattices)
                arm(h, L, r)
                for _ in range(3):
                    call()
                h.synchronize()
                engines[r] = list(h.engine())
            for _ in range(a.runs):
                for r in ROUTES:
                    arm(h, L, r)
                    call()
                    h.synchronize()
                    res[r].append(timed(h.stream(), call, a.reps))
                    h.synchronize()
            h.close()
            out["handles"]["N%d/L%d" % (N, L)] = dict(engine_and_shape=engines, event_us_per_call={r: stat(v) for r, v in res.items()})

    F, N, L = a.frames, 2000, 4
    pb = mc.problem(wl, N=N, L=L)
    b = pkg.BatchCRF(F, N, L, [2, 2], [float(w) for _, w in pb["kernels"]])
    b.set_inputs_host([N] * F, [np.repeat(f[None], F, 0) for f, _ in pb["kernels"]], unary=np.repeat(pb["unary"][None], F, 0))
    b.build()
    res, engines = {r: [] for r in ROUTES}, {}
    for r in res:
        arm(b, L, r)
        for _ in range(2):
            b.inference(T, True, 1.0)
        b.synchronize()
        engines[r] = b.engine()
    for _ in range(a.runs):
        for r in res:
            arm(b, L, r)
            t = []
            for _ in range(max(a.reps // 4, 3)):
                b.inference(T, True, 1.0)
                b.synchronize()
                t.append(b.last_timing()["inference_ms"] * 1e3)
            res[r].append(float(np.median(t)))
    b.close()
    out["batch"] = dict(frames=F, points=N, labels=L, engine=engines, event_us_per_call={r: stat(v) for r, v in res.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

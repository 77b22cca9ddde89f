#!/usr/bin/env python3
"""Time of the convergence kernel (csrc/fused_converge.hip) on the 2000-point two-label SLAM frame (tests/crf_cases.py: c2, two 2-D
terms), in the manner of tests/perf/fused_general.py: inference_converged(12, STOP_LABELS) on one handle holding the frame, and the
same on a batch of 256 such frames on built lattices.  HIP events around `--reps` calls, warm-up calls first, the two in turn,
`--rounds` times over; median with [min .. max].  Prints one JSON line.  `--root` names the tree the package is imported from, so
that two commits can be compared in one session.  Run by hand on the GPU box; not collected by pytest, not called by bench.py.

    python tests/perf/converge.py [--reps 20] [--rounds 9] [--root <tree to import the package from>]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

CAP, FRAMES = 12, 256


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    pb = wl.slam_problem(2000, seed=12)
    lib = pkg.lib()

    h = pkg.DenseCRFHIP(pb["N"], 2)
    h.set_unary_from_label(pb["label"], pb["conf"])
    for f, w in pb["kernels"]:
        h.add_pairwise(f, w)
    b = pkg.BatchCRF(FRAMES, pb["N"], 2, [2, 2], [float(w) for _, w in pb["kernels"]])
    b.set_inputs_host([pb["N"]] * FRAMES, [np.repeat(f[None], FRAMES, 0) for f, _ in pb["kernels"]],
                      label=np.repeat(pb["label"][None], FRAMES, 0), conf=pb["conf"])
    b.build()
    own = torch.cuda.Stream()

    def call_handle():                                           # (the entry point itself: the binding's method reads the report back)
        assert lib.lccrf_inference_converged(h.h, CAP, pkg.STOP_LABELS, 0.0, 1, 1.0) == 0

    def call_batch():
        b.inference_converged(CAP, pkg.STOP_LABELS, 0.0, True, 1.0, stream=own.cuda_stream)

    runs = {"handle": (h.stream(), call_handle, h.synchronize), "batch_%d" % FRAMES: (own.cuda_stream, call_batch, own.synchronize)}
    for _, call, sync in runs.values():                          # warm-up
        for _ in range(3):
            call()
        sync()
    report = dict(handle=dict(h.convergence(), delta=float(h.convergence()["delta"]), engine=list(h.engine())),
                  batch=dict(iterations=sorted(set(int(t) for t in b.convergence()["iterations"])), engine=b.engine()))
    ev = {}
    for _ in range(a.rounds):
        for name, (stream, call, sync) in runs.items():
            call()
            sync()
            ev.setdefault(name, []).append(timed(stream, call, a.reps))
            sync()
    h.close()
    b.close()
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(dict(shape="c2: N=2000 L=2 K=2, LABELS, cap %d, with_map" % CAP, root=a.root, reps=a.reps, rounds=a.rounds,
                          report=report, event_us_per_call={k: stat(v) for k, v in ev.items()})))


if __name__ == "__main__":
    main()

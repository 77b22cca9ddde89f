#!/usr/bin/env python3
"""Time of lccrf_batch_inference_backward (include/lccrf.h section 2c) on C2 frames -- 2000 keypoints, the two TUM3 terms, L = 2,
T = 5 -- for F = 1, 64, 1024, 16384 frames, against lccrf_inference_backward on one handle, in the same run.  HIP events around
the calls on the batch's / handle's own stream, after warm-up.  Prints one line per size and a JSON summary.  Run on the GPU box;
not collected by pytest.

    python tests/perf/batch_backward.py [--frames 1,64,1024,16384] [--reps 10]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("lc-crf-slam_amd")
wl = importlib.import_module("lc-crf-slam_amd.workloads")

N, L, T = 2000, 2, 5
POOL = 64                       # distinct frames, repeated to fill a batch


def bwd_bytes(F, K=2):
    S, B = N * L, (N + 255) // 256
    return 4 * (F * S * (T + K + 1) + max(T, 1) * K * F * B)


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                                         # warm-up (area, lattice sizes)
    fn()
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    probs = [wl.slam_problem(N, seed=1000 + i) for i in range(POOL)]
    w = [float(wl.TUM3["w1"]), float(wl.TUM3["w2"])]
    out = {}
    # one handle
    pb = probs[0]
    h = pkg.DenseCRFHIP(N, L)
    h.set_unary_from_label(pb["label"], pb["conf"])
    for (f, _), wk in zip(pb["kernels"], w):
        h.add_pairwise(f, wk)
    g = torch.randn((N, L), device="cuda")
    gu, gw = torch.empty_like(g), torch.empty(2, device="cuda")
    torch.cuda.synchronize()
    ms = timed(h.stream(), lambda: h.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()), a.reps)
    h.close()
    out["handle_ms_per_frame"] = ms
    print("handle    : %8.3f ms per frame" % ms)
    for F in [int(x) for x in a.frames.split(",")]:
        lab = np.stack([probs[f % POOL]["label"] for f in range(F)])
        feats = [np.stack([probs[f % POOL]["kernels"][k][0] for f in range(F)]) for k in range(2)]
        b = pkg.BatchCRF(F, N, L, [2, 2], w)
        b.set_inputs_host([N] * F, feats, label=lab, conf=pb["conf"])
        b.build()
        g = torch.randn((F, N, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty((F, 2), device="cuda")
        torch.cuda.synchronize()
        ms = timed(b.own_stream(), lambda: b.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()), a.reps)
        b.close()
        del g, gu, gw
        torch.cuda.empty_cache()
        out["F%d" % F] = dict(ms=ms, us_per_frame=1e3 * ms / F, area_bytes=bwd_bytes(F))
        print("F = %5d : %9.3f ms, %8.2f us per frame, area %.3g GB, %.0fx the handle per frame"
              % (F, ms, 1e3 * ms / F, bwd_bytes(F) / 1e9, out["handle_ms_per_frame"] * F / ms))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

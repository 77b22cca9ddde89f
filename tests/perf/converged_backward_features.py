#!/usr/bin/env python3
"""Time of lccrf_batch_inference_backward_modes_converged (include/lccrf.h section 2l) next to the fixed-count
lccrf_batch_inference_backward_features at the cap, on both routes (LCCRF_OPT_FUSED_BACKWARD_FEATURES off and on): a batch of C2 frames
-- 2000 keypoints, the two TUM3 terms (Potts, normalised AFTER), L = 2 --, cap 12, the counts those of a real
lccrf_batch_inference_converged run under STOP_LABELS, handed over on the device.  Both calls ask for dL/dU, the per-frame dL/dw and
both feature arrays, as the torch layer does.  A HIP event pair around every call on the batch's own stream; the median of --reps
calls after --warmup.  Reports the sum of the counts against F x cap -- the share of the fixed-count work the counts predict -- next
to the share seen, and the counts' histogram.  The batch repeats a pool of 64 distinct frames: in pool order (frame f is pool[f % 64])
or with --shuffle every slot drawn from the pool by a seeded generator.  Prints one line per timing and a JSON summary.  Run on the
GPU box; not collected by pytest.

    python tests/perf/converged_backward_features.py [--frames 1024] [--cap 12] [--reps 20] [--warmup 5] [--shuffle]"""
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

N, L, K = 2000, 2, 2
POOL = 64                       # distinct frames, repeated to fill a batch


def median_ms(stream, fn, reps, warmup):
    s = torch.cuda.ExternalStream(stream)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(s)
        fn()
        e1.record(s)
    ev[-1][1].synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--cap", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shuffle", action="store_true")
    a = ap.parse_args()
    F, cap = a.frames, a.cap
    pick = np.random.default_rng(5).integers(0, POOL, F) if a.shuffle else np.arange(F) % POOL
    probs = [wl.slam_problem(N, seed=1000 + i) for i in range(POOL)]
    w = [float(wl.TUM3["w1"]), float(wl.TUM3["w2"])]
    lab = np.stack([probs[i]["label"] for i in pick])
    feats = [np.stack([probs[i]["kernels"][k][0] for i in pick]) for k in range(K)]
    b = pkg.BatchCRF(F, N, L, [2, 2], w)
    b.set_inputs_host([N] * F, feats, label=lab, conf=probs[0]["conf"])
    b.build()
    b.inference_converged(cap, pkg.STOP_LABELS, 0.0, True, 1.0)
    counts = b.convergence()["iterations"].astype(np.int32)
    it = torch.from_numpy(counts).cuda()                          # (a copy: what a training step keeps of the forward)
    g = torch.randn((F, N, L), device="cuda")
    gu, gw = torch.empty_like(g), torch.empty((F, K), device="cuda")
    gf = [torch.empty((F, N, 2), device="cuda") for _ in range(K)]
    ptrs = [x.data_ptr() for x in gf]
    torch.cuda.synchronize()
    hist = np.bincount(counts, minlength=cap + 1).tolist()
    share = float(counts.sum()) / (F * cap)
    out = {"lib": pkg.LIB_PATH, "order": "shuffled" if a.shuffle else "pool", "frames": F, "cap": cap, "sum_counts": int(counts.sum()),
           "frames_x_cap": F * cap, "predicted_share": share, "histogram": hist}
    print("F = %d (%s order), cap %d: sum of the counts %d of %d (%.3f); histogram of t_f = 0 .. %d: %s"
          % (F, out["order"], cap, counts.sum(), F * cap, share, cap, hist))
    calls = {"converged": lambda: b.inference_backward_modes_converged_device(cap, 1.0, it.data_ptr(), g.data_ptr(), gu.data_ptr(),
                                                                              gw.data_ptr(), ptrs),
             "fixed": lambda: b.inference_backward_features_device(cap, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), ptrs)}
    for on, route in ((0, "stream"), (1, "fused")):
        b.set_option(pkg.OPT_FUSED_BACKWARD_FEATURES, on)
        for name, fn in calls.items():
            ms = median_ms(b.own_stream(), fn, a.reps, a.warmup)
            out["%s_%s_ms" % (name, route)] = ms
            out["%s_%s_route" % (name, route)] = b.backward_route()
        c, x = out["converged_%s_ms" % route], out["fixed_%s_ms" % route]
        out["seen_share_%s" % route] = c / x
        print("%-6s: converged %9.3f ms (route %d), fixed count %9.3f ms (route %d): share seen %.3f, share predicted by the counts %.3f"
              % (route, c, out["converged_%s_route" % route], x, out["fixed_%s_route" % route], c / x, share))
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

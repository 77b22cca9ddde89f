#!/usr/bin/env python3
"""Time of lccrf_inference_backward_features / lccrf_batch_inference_backward_features (include/lccrf.h sections 1d / 2d) with and
without feature pointers, against lccrf_inference_backward / lccrf_batch_inference_backward on the same inputs in the same
process: (a) one 2000-keypoint frame (the two TUM3 terms, L = 2, T = 5), (b) the 320 x 240 image (position and RGB terms, L = 21,
T = 10), (c) a batch of 1024 of the frames of (a).  HIP events around the calls on the handle's / batch's own stream, after
warm-up; the three variants of a case are timed in turn, `--rounds` times over, and the median of the rounds is reported with
their spread.  Prints one line per case and a JSON summary.  Run on the GPU box; not collected by pytest.

    python tests/perf/backward_features.py [--cases a,b,c] [--reps 10] [--rounds 5]"""
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

POOL = 64


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(name, stream, variants, reps, rounds, out):
    """variants: {label: fn}; warm-up of each, then `rounds` rounds of every variant in turn"""
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(stream, fn, reps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out[name] = dict(ms=med, spread={k: [min(v), max(v)] for k, v in ms.items()},
                     ratio_without=med["without"] / med["old"], ratio_with=med["with"] / med["old"])
    print("%-28s old %9.3f ms [%.3f .. %.3f]  new without pointers %9.3f ms (x %.3f)  with %9.3f ms (x %.2f)"
          % (name, med["old"], min(ms["old"]), max(ms["old"]), med["without"], out[name]["ratio_without"], med["with"],
             out[name]["ratio_with"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    cases = a.cases.split(",")
    out = {}
    w = [float(wl.TUM3["w1"]), float(wl.TUM3["w2"])]
    probs = [wl.slam_problem(2000, seed=1000 + i) for i in range(POOL)]
    if "a" in cases:
        N, L, T = 2000, 2, 5
        pb = probs[0]
        h = pkg.DenseCRFHIP(N, L)
        h.set_unary_from_label(pb["label"], pb["conf"])
        for (f, _), wk in zip(pb["kernels"], w):
            h.add_pairwise(f, wk)
        g = torch.randn((N, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty(2, device="cuda")
        gf = [torch.empty((N, 2), device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        compare("one 2000-keypoint frame", h.stream(), dict(
            old=lambda: h.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()),
            without=lambda: h.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), None),
            **{"with": lambda: h.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                                                    [t.data_ptr() for t in gf])}), a.reps, a.rounds, out)
        h.close()
    if "b" in cases:
        W, H, L, T = 320, 240, 21, 10
        rng = np.random.default_rng(3)
        im = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        y, x = np.mgrid[0:H, 0:W]
        lab = torch.from_numpy(((x // 40 + 3 * (y // 40)) % L).astype(np.int16).reshape(-1)).cuda()
        torch.cuda.synchronize()
        h = pkg.DenseCRFHIP(W * H, L)
        h.set_unary_from_label_device(lab.data_ptr(), 0.5)
        h.add_image_kernel(W, H, 3.0, 3.0)
        h.add_image_kernel(W, H, 10.0, 60.0, im.data_ptr(), pkg.IMAGE_U8, 20.0)
        g = torch.randn((W * H, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty(2, device="cuda")
        gf = [torch.empty((W * H, d), device="cuda") for d in (2, 5)]
        torch.cuda.synchronize()
        compare("320 x 240 image, L = 21", h.stream(), dict(
            old=lambda: h.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()),
            without=lambda: h.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), None),
            **{"with": lambda: h.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                                                    [t.data_ptr() for t in gf])}), max(a.reps // 3, 2), a.rounds, out)
        h.close()
    if "c" in cases:
        N, L, T, F = 2000, 2, 5, 1024
        lab = np.stack([probs[f % POOL]["label"] for f in range(F)])
        feats = [np.stack([probs[f % POOL]["kernels"][k][0] for f in range(F)]) for k in range(2)]
        b = pkg.BatchCRF(F, N, L, [2, 2], w)
        b.set_inputs_host([N] * F, feats, label=lab, conf=probs[0]["conf"])
        b.build()
        g = torch.randn((F, N, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty((F, 2), device="cuda")
        gf = [torch.empty((F, N, 2), device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        compare("1024 frames of 2000", b.own_stream(), dict(
            old=lambda: b.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()),
            without=lambda: b.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), None),
            **{"with": lambda: b.inference_backward_features_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                                                    [t.data_ptr() for t in gf])}), a.reps, a.rounds, out)
        b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of lccrf_inference_backward_features / lccrf_batch_inference_backward_features (both feature arrays plus dL/dU and dL/dw) with
LCCRF_OPT_FUSED_BACKWARD_FEATURES off and on (include/lccrf.h section 1l) on C2 frames -- 2000 keypoints, the two TUM3 terms, L = 2,
T = 5.  One handle and batches of --frames frames.  A HIP event pair around every call on the handle's / batch's own stream; the
median of --reps calls after --warmup.  The library is the one LCCRF_LIB names (else this tree's): a library from before the option
existed is timed with the option off only.  One process times one library; alternate processes for an A/B (three runs each, in one
session on one machine).  Prints one line per size and a JSON summary.  Run on the GPU box; not collected by pytest.

    [LCCRF_LIB=other/liblccrf_hip.so] python tests/perf/fused_backward_features.py [--frames 64,1024] [--reps 20] [--warmup 5]

--trace: no events and no timing -- for a run under `rocprofv3 --kernel-trace`, which gives the kernels' own time: --reps calls each
of the feature request (option 8 on) and of the request without feature arrays (option 6 on: k_backward), at T = 5 and at T = 1, on
the handle and on the largest batch.  A kernel's time is linear in T; what is left at T = 0 of k_backward_features beyond what is left
of k_backward is the part behind the sweep: the norm part's two width-1 filters per term, their corner dots and dL/db -> dL/df."""
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
OPT, OPT_PLAIN = 8, 6           # LCCRF_OPT_FUSED_BACKWARD_FEATURES, LCCRF_OPT_FUSED_BACKWARD


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


def has_option(obj):
    try:
        obj.set_option(OPT, 0)
        return True
    except pkg.LccrfError:
        return False


def both_ways(obj, stream, fn, reps, warmup):
    """{"off": ms, "on": ms or None, "route_on": the route the option-on calls took}"""
    fused = has_option(obj)
    out = {"off": median_ms(stream, fn, reps, warmup), "on": None, "route_on": None}
    if fused:
        obj.set_option(OPT, 1)
        out["on"] = median_ms(stream, fn, reps, warmup)
        out["route_on"] = obj.backward_route()
    return out


def show(name, r, frames):
    on = "     (no such option)" if r["on"] is None else "%9.3f ms on (route %d, %.2fx)" % (r["on"], r["route_on"], r["off"] / r["on"])
    print("%-12s: %9.3f ms off, %s, %8.2f us per frame off" % (name, r["off"], on, 1e3 * r["off"] / frames))


def trace(obj, features_call, plain_call, reps):
    """the calls a kernel trace is read from: features and plain, T = 5 and T = 1"""
    obj.set_option(OPT, 1)
    obj.set_option(OPT_PLAIN, 1)
    for t in (T, 1):
        for call in (features_call, plain_call):
            for _ in range(reps):
                call(t)
            obj.synchronize()
            assert obj.backward_route() == pkg.BACKWARD_FUSED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    probs = [wl.slam_problem(N, seed=1000 + i) for i in range(POOL)]
    w = [float(wl.TUM3["w1"]), float(wl.TUM3["w2"])]
    out = {"lib": pkg.LIB_PATH}
    pb = probs[0]
    h = pkg.DenseCRFHIP(N, L)
    h.set_unary_from_label(pb["label"], pb["conf"])
    for (f, _), wk in zip(pb["kernels"], w):
        h.add_pairwise(f, wk)
    g = torch.randn((N, L), device="cuda")
    gu, gw = torch.empty_like(g), torch.empty(2, device="cuda")
    gf = [torch.empty((N, 2), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    def handle_features(t=T):
        h.inference_backward_features_device(t, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [x.data_ptr() for x in gf])

    if a.trace:
        trace(h, handle_features, lambda t: h.inference_backward_device(t, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()), a.reps)
    else:
        out["handle"] = both_ways(h, h.stream(), handle_features, a.reps, a.warmup)
        show("handle", out["handle"], 1)
    h.close()
    sizes = [int(x) for x in a.frames.split(",") if x]
    for F in sizes[-1:] if a.trace else sizes:
        lab = np.stack([probs[f % POOL]["label"] for f in range(F)])
        feats = [np.stack([probs[f % POOL]["kernels"][k][0] for f in range(F)]) for k in range(2)]
        b = pkg.BatchCRF(F, N, L, [2, 2], w)
        b.set_inputs_host([N] * F, feats, label=lab, conf=pb["conf"])
        b.build()
        g = torch.randn((F, N, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty((F, 2), device="cuda")
        gf = [torch.empty((F, N, 2), device="cuda") for _ in range(2)]
        torch.cuda.synchronize()

        def batch_features(t=T):
            b.inference_backward_features_device(t, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), [x.data_ptr() for x in gf])

        if a.trace:
            trace(b, batch_features, lambda t: b.inference_backward_device(t, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()), a.reps)
        else:
            key = "F%d" % F
            out[key] = both_ways(b, b.own_stream(), batch_features, a.reps, a.warmup)
            show(key, out[key], F)
        b.close()
        del g, gu, gw, gf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

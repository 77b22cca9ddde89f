#!/usr/bin/env python3
"""Time of lccrf_inference_backward_compat / lccrf_batch_inference_backward_all (d_grad_compat, and d_grad_model for batches) with
LCCRF_OPT_FUSED_BACKWARD_LEARNT off and on (include/lccrf.h section 1k) on C2 frames -- 2000 keypoints, the two TUM3 terms, L = 2,
T = 5 -- under two learnt models: "matrices" (a dense matrix per term, normalised AFTER) and "symmetric" (Potts terms, the norm half
on either side of the filter).  One handle and batches of --frames frames.  A HIP event pair around every call on the handle's /
batch's own stream; the median of --reps calls after --warmup.  The library is the one LCCRF_LIB names (else this tree's): a library
from before the option existed is timed with the option off only.  One process times one library; alternate processes for an A/B
(three runs each, in one session on one machine).  Prints one line per model and size and a JSON summary.  Run on the GPU box; not
collected by pytest.

    [LCCRF_LIB=other/liblccrf_hip.so] python tests/perf/fused_backward_learnt.py [--frames 64,1024] [--reps 20] [--warmup 5]"""
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
OPT = 7                         # LCCRF_OPT_FUSED_BACKWARD_LEARNT
SYMMETRIC = 2                   # lccrf_normalization


def matrices():
    rng = np.random.default_rng(77)
    return [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(2)]


def arm(obj, model):
    if model == "matrices":
        for k, m in enumerate(matrices()):
            obj.set_pairwise_compatibility(k, m)
    else:
        for k in range(2):
            obj.set_normalization(k, SYMMETRIC)


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
    print("%-20s: %9.3f ms off, %s, %8.2f us per frame off" % (name, r["off"], on, 1e3 * r["off"] / frames))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="matrices,symmetric")
    a = ap.parse_args()
    probs = [wl.slam_problem(N, seed=1000 + i) for i in range(POOL)]
    w = [float(wl.TUM3["w1"]), float(wl.TUM3["w2"])]
    out = {"lib": pkg.LIB_PATH}
    pb = probs[0]
    for model in a.models.split(","):
        h = pkg.DenseCRFHIP(N, L)
        h.set_unary_from_label(pb["label"], pb["conf"])
        for (f, _), wk in zip(pb["kernels"], w):
            h.add_pairwise(f, wk)
        arm(h, model)
        g = torch.randn((N, L), device="cuda")
        gu, gw, gm = torch.empty_like(g), torch.empty(2, device="cuda"), torch.empty((2, L, L), device="cuda")
        torch.cuda.synchronize()
        key = model + " handle"
        out[key] = both_ways(h, h.stream(), lambda: h.inference_backward_compat_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                                                                        gm.data_ptr()), a.reps, a.warmup)
        h.close()
        show(key, out[key], 1)
        for F in [int(x) for x in a.frames.split(",") if x]:
            lab = np.stack([probs[f % POOL]["label"] for f in range(F)])
            feats = [np.stack([probs[f % POOL]["kernels"][k][0] for f in range(F)]) for k in range(2)]
            b = pkg.BatchCRF(F, N, L, [2, 2], w)
            arm(b, model)
            b.set_inputs_host([N] * F, feats, label=lab, conf=pb["conf"])
            b.build()
            g = torch.randn((F, N, L), device="cuda")
            gu, gw, gm = torch.empty_like(g), torch.empty((F, 2), device="cuda"), torch.empty((F, 2, L, L), device="cuda")
            md = torch.empty(2 + 2 * L * L, device="cuda")
            torch.cuda.synchronize()
            key = "%s F%d" % (model, F)
            out[key] = both_ways(b, b.own_stream(),
                                 lambda: b.inference_backward_all_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), None, gm.data_ptr(),
                                                                         md.data_ptr()), a.reps, a.warmup)
            b.close()
            del g, gu, gw, gm, md
            torch.cuda.empty_cache()
            show(key, out[key], F)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

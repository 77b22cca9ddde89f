#!/usr/bin/env python3
"""Time of lccrf_batch_inference_backward_all (include/lccrf.h section 2h) on c2 frames -- 2000 points, two 2-D terms, two labels,
T = 5; 64 distinct frames, workloads.slam_problem -- whose terms carry label-compatibility matrices I + 0.3 N(0, 1) on both terms
("matrices") or the mixed setting of tests/perf/batch_general.py (SYMMETRIC with a matrix on the first term, BEFORE on the second).
Per batch size (1, 64 and 1024 frames) and setting, microseconds per call:

    learnt_all      lccrf_batch_inference_backward_all with d_grad_unary, d_grad_weights, d_grad_compat and d_grad_model
    potts_2c        lccrf_batch_inference_backward on the same batch with its matrices and modes taken back: the path the call grew from
    handles_1e      handles holding the batch's first min(F, --handles) frames with the setting, lccrf_inference_backward_compat called
                    one after another and then waited for (host clock: the handles have a stream each), scaled to F frames

HIP events on the batch's stream around `--reps` calls, warm-up calls first, the variants in turn `--rounds` times over; median with
[min .. max].  Prints one JSON line.  Run by hand on the GPU box; not collected by pytest, not called by bench.py.

    python tests/perf/batch_backward_general.py [--frames 1 64 1024] [--reps 5] [--rounds 7] [--handles 64]"""
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
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--handles", type=int, default=64)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    N, K, L, T = 2000, 2, 2, 5
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

    stat = lambda v: dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1))
    out = dict(shape="c2: N=2000 L=2 K=2 T=5, %d distinct frames" % a.distinct, reps=a.reps, rounds=a.rounds, batches={})
    for F in a.frames:
        idx = [i % a.distinct for i in range(F)]
        feats = [np.stack([pbs[i]["kernels"][k][0] for i in idx]) for k in range(K)]
        label = np.stack([pbs[i]["label"] for i in idx])
        b = pkg.BatchCRF(F, N, L, [2] * K, w)
        b.set_inputs_host([N] * F, feats, label=label, conf=pbs[0]["conf"])
        b.build()
        g = torch.randn((F, N, L), device="cuda")
        gu, gw = torch.empty_like(g), torch.empty((F, K), device="cuda")
        gm, md = torch.empty((F, K, L, L), device="cuda"), torch.empty(K * (1 + L * L), device="cuda")
        nh = min(F, a.handles)
        hs = []
        for i in range(nh):
            pb = pbs[idx[i]]
            h = pkg.DenseCRFHIP(N, L)
            h.set_unary_from_label(pb["label"], pb["conf"])
            for f, x in pb["kernels"]:
                h.add_pairwise(f, x)
            hs.append(h)
        torch.cuda.synchronize()
        learnt = lambda: b.inference_backward_all_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), None, gm.data_ptr(), md.data_ptr())
        plain = lambda: b.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr())

        def handles():
            t0 = time.perf_counter()
            for i, h in enumerate(hs):
                h.inference_backward_compat_device(T, 1.0, g[i].data_ptr(), gu[i].data_ptr(), gw[i].data_ptr(), gm[i].data_ptr())
            for h in hs:
                h.synchronize()
            return (time.perf_counter() - t0) * 1e6 * F / nh
        res = {}
        for sname, setting in settings.items():
            for h in hs:
                arm(h, setting)
            ev = {}
            for st, call in ((setting, learnt), (potts, plain)):     # warm-up: the areas, the factors
                arm(b, st)
                for _ in range(2):
                    call()
                b.synchronize()
            handles()
            for _ in range(a.rounds):
                arm(b, setting)
                learnt()
                b.synchronize()
                ev.setdefault("learnt_all", []).append(timed(b.own_stream(), learnt, a.reps))
                arm(b, potts)
                plain()
                b.synchronize()
                ev.setdefault("potts_2c", []).append(timed(b.own_stream(), plain, a.reps))
                ev.setdefault("handles_1e", []).append(handles())
            res[sname] = dict(us_per_call={k: stat(v) for k, v in ev.items()}, handles=nh,
                              us_per_frame={k: round(float(np.median(v)) / F, 2) for k, v in ev.items()})
        for h in hs:
            h.close()
        b.close()
        del g, gu, gw, gm, md
        torch.cuda.empty_cache()
        out["batches"][str(F)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()

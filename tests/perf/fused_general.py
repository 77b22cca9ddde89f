#!/usr/bin/env python3
"""Time of lccrf_inference(5, with_map) on one handle holding the 2000-point two-label SLAM frame (tests/crf_cases.py: c2, two 2-D
terms) as a Potts model, with label-compatibility matrices I + 0.3 N(0, 1) on both terms, with both terms normalised SYMMETRICally,
and with both (include/lccrf.h sections 1e and 1g; csrc/fused_general.hip).  Two clocks per variant: HIP events on the handle's
stream around `--reps` calls, and the host's clock around one call + lccrf_get_map.  Warm-up calls first, then the variants in
turn, `--rounds` times over; median with [min .. max].  Prints one JSON line.  The same file runs on a tree without
lccrf_get_engine (engines then read null), so that two commits can be compared in one session.  Run by hand on the GPU box; not
collected by pytest, not called by bench.py.

    python tests/perf/fused_general.py [--reps 20] [--rounds 9] [--root <tree to import the package from>]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch


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
    K, L, T = 2, 2, 5
    rng = np.random.default_rng([77, K, L])
    dense = [(np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]
    after, sym = pkg.NORMALIZE_AFTER, pkg.NORMALIZE_SYMMETRIC
    setups = {"potts": ([None] * K, after), "matrices": (dense, after), "symmetric": ([None] * K, sym),
              "symmetric_matrices": (dense, sym)}
    h = pkg.DenseCRFHIP(pb["N"], L)
    h.set_unary_from_label(pb["label"], pb["conf"])
    for f, w in pb["kernels"]:
        h.add_pairwise(f, w)

    def arm(name):
        mats, mode = setups[name]
        for k in range(K):
            h.set_pairwise_compatibility(k, mats[k])
            h.set_normalization(k, mode)

    def call():
        h.inference(T, True, 1.0)

    engines = {}
    for name in setups:                                          # warm-up of every variant
        arm(name)
        for _ in range(3):
            call()
            h.map()
        engines[name] = list(h.engine()) if hasattr(h, "engine") else None
    ev, wall = {}, {}
    for _ in range(a.rounds):
        for name in setups:
            arm(name)
            call()
            h.synchronize()
            ev.setdefault(name, []).append(timed(h.stream(), call, a.reps))
            h.synchronize()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                h.map()
                t.append((time.perf_counter() - t0) * 1e6)
            wall.setdefault(name, []).append(float(np.median(t)))
    h.close()
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    out = dict(shape="c2: N=2000 L=2 K=2 T=5 with_map", root=a.root, reps=a.reps, rounds=a.rounds, engine_and_shape=engines,
               event_us_per_call={k: stat(v) for k, v in ev.items()}, wall_us_call_plus_get_map={k: stat(v) for k, v in wall.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What LCCRF_OPT_FRAME_GENERAL saves (include/lccrf.h; csrc/frame_general.hip; notes/frame_general.md section 5): a learnt model -- a
label-compatibility matrix I + 0.3 N(0, 1) and the SYMMETRIC normalisation on the first term, the second term Potts / AFTER -- on a
fresh frame, option off (the two-kernel route: build launches, a stream synchronisation, the factor kernels, k_general) against
option on (one launch).

  (a) single-frame latency: the host's wall clock of  set inputs -> inference(5, true) -> get_map  on a handle (taken from the
      handle cache, as the tracker's per-frame DenseCRF is), for a 2000-point and a 500-point frame;
  (b) batch throughput: lccrf_batch_run(5, true) by HIP events on the batch's stream, for a C2-shaped batch (workloads.slam_problem,
      2000 points, 64 distinct frames) of 1024 frames with the same model; and the same batch as a Potts / AFTER batch in one launch,
      the floor the general form cannot beat.

Warm-up calls first, the legs in turn `--rounds` times over, median with [min .. max] of the timed calls.  A library that refuses
option 5 (a build from before the option) runs the option-off legs alone.  Prints one JSON line.  Run by hand on the GPU box; not
collected by pytest, not called by bench.py.

    python tests/perf/frame_general.py [--frames 1024] [--reps 10] [--rounds 9] [--calls 200]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OPT = 5                                                           # LCCRF_OPT_FRAME_GENERAL


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
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    K, L, T = 2, 2, 5
    rng = np.random.default_rng([77, K, L])
    mu = (np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32)
    stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
    try:
        pkg.set_default_option(OPT, 0)
        legs = (0, 1)
    except pkg.LccrfError:
        legs = (0,)                                               # a library without the option: the baseline alone
    out = dict(library=pkg.LIB_PATH, option_known=len(legs) == 2, reps=a.reps, rounds=a.rounds, calls=a.calls)

    # ---- (a) one frame at a time
    out["single_frame_wall_us"] = {}
    for N in (2000, 500):
        pb = wl.slam_problem(N, seed=12)
        wall, engines = {on: [] for on in legs}, {}

        def frame(on):
            h = pkg.DenseCRFHIP(N, L)                             # (from the handle cache after the first)
            if on:
                h.set_option(OPT, 1)
            t0 = time.perf_counter()
            h.set_unary_from_label(pb["label"], pb["conf"])
            for f, x in pb["kernels"]:
                h.add_pairwise(f, x)
            h.set_pairwise_compatibility(0, mu)
            h.set_normalization(0, pkg.NORMALIZE_SYMMETRIC)
            h.inference(T, True, 1.0)
            m = h.map()
            dt = (time.perf_counter() - t0) * 1e6
            engines[on] = h.engine()[0]
            h.close()
            return dt, m

        ref = None
        for on in legs:
            for _ in range(20):
                _, m = frame(on)
            ref = m if ref is None else ref
            assert np.array_equal(m, ref)
        for _ in range(a.rounds):
            for on in legs:
                wall[on] += [frame(on)[0] for _ in range(a.calls // a.rounds + 1)]
        out["single_frame_wall_us"][str(N)] = {("on" if on else "off"): dict(engine=engines[on], **stat(wall[on])) for on in legs}

    # ---- (b) a batch of fresh frames
    N, F = 2000, a.frames
    pbs = [wl.slam_problem(N, seed=1 + i) for i in range(a.distinct)]
    w = [float(x) for _, x in pbs[0]["kernels"]]
    idx = [i % a.distinct for i in range(F)]
    feats = [np.stack([pbs[i]["kernels"][k][0] for i in idx]) for k in range(K)]
    label = np.stack([pbs[i]["label"] for i in idx])
    batches = {}
    for leg in legs + ("potts",):
        b = pkg.BatchCRF(F, N, L, [2] * K, w)
        if leg == 1:
            b.set_option(OPT, 1)
        if leg != "potts":
            b.set_pairwise_compatibility(0, mu)
            b.set_normalization(0, pkg.NORMALIZE_SYMMETRIC)
        b.set_inputs_host([N] * F, feats, label=label, conf=pbs[0]["conf"])
        batches[leg] = b
    ev, engines = {}, {}
    for leg, b in batches.items():
        for _ in range(3):
            b.run(T, True, 1.0)
        b.synchronize()
        engines[leg] = [b.engine(), list(b.fused_shape()), b.fallback_frames()]
    if len(legs) == 2:
        assert batches[0].probability().tobytes() == batches[1].probability().tobytes()
    for _ in range(a.rounds):
        for leg, b in batches.items():
            call = lambda: b.run(T, True, 1.0)
            call()
            b.synchronize()
            ev.setdefault(leg, []).append(timed(b.own_stream(), call, a.reps))
            b.synchronize()
    name = {0: "off", 1: "on", "potts": "potts_one_launch"}
    out["batch_run5_event_us"] = dict(frames=F, points=N, legs={name[k]: dict(engine_shape_fallback=engines[k], **stat(v)) for k, v in ev.items()})
    for b in batches.values():
        b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

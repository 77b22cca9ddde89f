#!/usr/bin/env python3
"""Cost of convergence-driven inference on a batch of SLAM frames (include/lccrf.h sections 2e and 2f; notes/convergence.md).

HIP-event time per batch (lccrf_batch_last_timing) of
    fixed       lccrf_batch_inference(5) as it stands -- full-size frames take the two-frames-per-CU shape
    never       the converged call with a criterion that is never met at cap 5 (LABELS and DELTA at tol 0): the same five
                iterations plus the reduction, one frame per CU
    labels      the converged call, LABELS at cap 12: every frame stops on its own
and, from inputs alone (the tracker's "build, infer once, read the labels"), on the same frames and with the same timing,
    run_5                   lccrf_batch_run(5): one launch per batch
    build_labels_cap_12     lccrf_batch_build + lccrf_batch_inference_converged, LABELS at cap 12: build time + inference time
    run_labels_cap_12       lccrf_batch_run_converged, the same: one launch per batch (engine 3)
with the histogram of iterations beside the times.  Prints one JSON line; none of the figures is a pass bar.

    python tools/converge_bench.py [--frames 4096] [--points 2000] [--distinct 64] [--reps 20] [--warmup 5]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("lc-crf-slam_amd")
    wl = importlib.import_module("lc-crf-slam_amd.workloads")
    pbs = [wl.slam_problem(a.points, seed=1 + i) for i in range(a.distinct)]
    idx = [i % a.distinct for i in range(a.frames)]
    feats = [np.stack([pbs[i]["kernels"][k][0] for i in idx]) for k in range(2)]
    label = np.stack([pbs[i]["label"] for i in idx])
    b = pkg.BatchCRF(a.frames, a.points, 2, [2, 2], [float(w) for _, w in pbs[0]["kernels"]])
    b.set_inputs_host([a.points] * a.frames, feats, label=label, conf=pbs[0]["conf"])
    b.build()

    def timed(call, with_build=False):
        ms = []
        for r in range(a.warmup + a.reps):
            call()
            b.synchronize()
            if r >= a.warmup:
                t = b.last_timing()
                ms.append(t["inference_ms"] + (t["build_ms"] if with_build else 0.0))
        ms = np.array(ms)
        return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), max_ms=round(float(ms.max()), 4),
                    cv=round(float(ms.std() / ms.mean()), 4), reps=int(ms.size))

    def histogram():
        it = b.convergence()["iterations"]
        return {int(t): int(n) for t, n in zip(*np.unique(it, return_counts=True))}

    out = dict(frames=a.frames, points=a.points, distinct=a.distinct)
    out["fixed_5"] = timed(lambda: b.inference(5, True, 1.0))
    out["fixed_5"]["engine"], out["fixed_5"]["fused_shape"] = b.engine(), b.fused_shape()
    out["never_met_cap_5"] = timed(lambda: b.inference_converged(5, pkg.STOP_DELTA | pkg.STOP_LABELS, 0.0, True, 1.0))
    out["never_met_cap_5"].update(engine=b.engine(), iterations=histogram())
    out["labels_cap_12"] = timed(lambda: b.inference_converged(12, pkg.STOP_LABELS, 0.0, True, 1.0))
    out["labels_cap_12"].update(engine=b.engine(), iterations=histogram())
    its = b.convergence()["iterations"]
    out["labels_cap_12"]["mean_iterations"] = round(float(its.mean()), 3)
    f5, n5, l12 = (out[k]["median_ms"] for k in ("fixed_5", "never_met_cap_5", "labels_cap_12"))
    out["frame_iterations_per_s"] = dict(fixed_5=round(a.frames * 5 / (f5 * 1e-3)), never_met_cap_5=round(a.frames * 5 / (n5 * 1e-3)),
                                         labels_cap_12=round(float(its.sum()) / (l12 * 1e-3)))
    # from inputs alone
    out["run_5"] = timed(lambda: b.run(5, True, 1.0))
    out["run_5"].update(engine=b.engine(), fallback_frames=b.fallback_frames())

    def build_and_converge():
        b.build()
        b.inference_converged(12, pkg.STOP_LABELS, 0.0, True, 1.0)
    out["build_labels_cap_12"] = timed(build_and_converge, with_build=True)
    out["build_labels_cap_12"].update(engine=b.engine(), iterations=histogram())
    out["run_labels_cap_12"] = timed(lambda: b.run_converged(12, pkg.STOP_LABELS, 0.0, True, 1.0))
    out["run_labels_cap_12"].update(engine=b.engine(), fallback_frames=b.fallback_frames(), iterations=histogram())
    for k in ("build_labels_cap_12", "run_labels_cap_12"):
        out["frame_iterations_per_s"][k] = round(float(its.sum()) / (out[k]["median_ms"] * 1e-3))
    out["frame_iterations_per_s"]["run_5"] = round(a.frames * 5 / (out["run_5"]["median_ms"] * 1e-3))
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of lccrf_inference with label-compatibility matrices (include/lccrf.h section 1e) on the reference's image example: 320 x
240 pixels, 21 labels, the position and RGB terms, 10 iterations (tests/golden/example_im1.npz).  (a) no matrices, on the streaming
engine (the handle is sized beyond the one-workgroup engines anyway); (b) identity matrices; (c) dense matrices I + 0.3 N(0, 1);
and lccrf_inference_backward_compat against lccrf_inference_backward.  HIP events on the handle's stream after warm-up; the
variants are timed in turn, `--rounds` times over, median and spread reported.  Prints one JSON line.  Run by hand on the GPU box;
not collected by pytest, not called by bench.py.

    python tests/perf/compatibility.py [--reps 5] [--rounds 7]"""
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


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_im1.npz"))
    W, H, L, T, K = 320, 240, 21, 10, 2
    im = torch.from_numpy(np.ascontiguousarray(z["im"], np.uint8)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(z["label"].reshape(-1), np.int16)).cuda()
    torch.cuda.synchronize()
    h = pkg.DenseCRFHIP(W * H, L)
    h.set_unary_from_label_device(lab.data_ptr(), 0.5)
    h.add_image_kernel(W, H, 3.0, 3.0)
    h.add_image_kernel(W, H, 10.0, 60.0, im.data_ptr(), pkg.IMAGE_U8, 20.0)
    rng = np.random.default_rng(7)
    eye = np.eye(L, dtype=np.float32)
    dense = [(eye + 0.3 * rng.standard_normal((L, L))).astype(np.float32) for _ in range(K)]
    g = torch.randn((W * H, L), device="cuda")
    gu, gw, gm = torch.empty_like(g), torch.empty(K, device="cuda"), torch.empty((K, L, L), device="cuda")
    torch.cuda.synchronize()

    def arm(mats):
        for k in range(K):
            h.set_pairwise_compatibility(k, mats[k])

    setups = {"a_potts": [None] * K, "b_identity": [eye] * K, "c_dense": dense}
    runs = {"inference": lambda: h.inference(T, False, 1.0),
            "backward": lambda: h.inference_backward_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr()),
            "backward_compat": lambda: h.inference_backward_compat_device(T, 1.0, g.data_ptr(), gu.data_ptr(), gw.data_ptr(), gm.data_ptr())}
    ms = {}
    # inference first: it runs in locality mode until the first backward re-builds the lattices the plain way (section 1c)
    for phase in (("inference",), ("backward", "backward_compat")):
        for name, mats in setups.items():                        # warm-up of every variant
            arm(mats)
            for rn in phase:
                runs[rn]()
                runs[rn]()
        h.synchronize()
        for _ in range(a.rounds):
            for name, mats in setups.items():
                arm(mats)
                h.synchronize()
                for rn in phase:
                    ms.setdefault(name + ":" + rn, []).append(timed(h.stream(), runs[rn], a.reps if rn == "inference" else max(a.reps // 2, 1)))
    h.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(shape="320x240 L=21 K=2 T=10", ms=med, spread={k: [min(v), max(v)] for k, v in ms.items()},
               identity_over_potts=med["b_identity:inference"] / med["a_potts:inference"],
               dense_over_potts=med["c_dense:inference"] / med["a_potts:inference"],
               backward_compat_over_backward_potts=med["a_potts:backward_compat"] / med["a_potts:backward"],
               backward_compat_over_backward_dense=med["c_dense:backward_compat"] / med["c_dense:backward"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()

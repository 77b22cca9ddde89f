#!/usr/bin/env python3
"""Generate tests/golden/labels.npz from the REFERENCE itself (oracle/_ref: the reference's own DenseCRF headers compiled in
place): the label counts, term counts and feature dimensions of include/lccrf.h beyond the other fixtures' corner (L up to 64,
eight terms, d = 7 and 8), and the bare lattice filter at value sizes up to 64.

    python tests/golden/make_golden_labels.py

Inputs are stored with the results (tests/crf_cases.py: case_problem() decodes them, label_problem() made them); per case the
reference's lattice internals (V, norm, offset, bary, nbr) of every kernel, the Q trace (T = 3, relax 0.75) and the labels.  The
archive is written with fixed member dates, so running the script twice gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crf_cases as cc  # noqa: E402
import pyoracle as po  # noqa: E402

T, RELAX = 3, 0.75
LABELS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 21, 22, 31, 32, 33, 63, 64)
FILTER_SIZES = (1, 3, 4, 7, 31, 33, 63, 64)


def cases():
    """(name, problem): every instantiated L at d = 2 or 3 (label input at every other L from 2), eight terms of d = 1..8 at
    L = 5 and 33, one term of d = 7 and of d = 8 at L = 2 and 64.  N shrinks with L so that the traces stay small."""
    out = []
    for i, L in enumerate(LABELS):
        N = 160 if L <= 9 else 64 if L <= 22 else 40
        d = 2 + i % 2
        out.append(("L%d" % L, cc.label_problem(N, L, [d], seed=1, spread=1.5, label=L >= 2 and i % 2 == 1)))
    for L in (5, 33):
        out.append(("K8_L%d" % L, cc.label_problem(32, L, list(range(1, 9)), seed=2, spread=1.0, label=L == 33)))
    for L in (2, 64):
        for d in (7, 8):
            out.append(("d%d_L%d" % (d, L), cc.label_problem(64 if L == 2 else 24, L, [d], seed=3, spread=2.0, label=L == 2)))
    return out


def filter_inputs():
    rng = np.random.default_rng(7)
    out = []
    for i, vs in enumerate(FILTER_SIZES):
        d = (2, 3, 5)[i % 3]
        f = rng.normal(0, 3, (60, d)).astype(np.float32)
        q = rng.random(60) < 0.3
        f[q] = np.round(f[q] * 2) / 2                                          # points on lattice-cell boundaries
        x = (np.round(rng.normal(0, 1, (60, vs)) * 16) / 16).astype(np.float32)
        out.append((vs, f, x))
    return out


def pack(z, p, pb):
    z[p + "N"], z[p + "L"], z[p + "K"] = np.int32(pb["N"]), np.int32(pb["L"]), np.int32(len(pb["kernels"]))
    if "unary" in pb:
        z[p + "unary"] = np.asarray(pb["unary"], np.float32)
    else:
        z[p + "label"], z[p + "conf"] = np.asarray(pb["label"], np.int16), np.float32(pb["conf"])
    for k, (f, w) in enumerate(pb["kernels"]):
        z[p + "feat%d" % k], z[p + "w%d" % k] = np.asarray(f, np.float32), np.float32(w)


def run(z, p, pb):
    r = cc.setup(po.RefCRF, pb)
    for k in range(len(pb["kernels"])):
        kv = r.kernel(k)
        z[p + "V%d" % k] = np.int32(kv["V"])
        for name in ("norm", "offset", "bary", "nbr"):
            z[p + "%s%d" % (name, k)] = kv[name]
    z[p + "trace"] = r.run_trace(T, relax=RELAX)
    r.build_map()
    z[p + "map"] = r.map()
    r.close()


def save(path, arrays):
    """np.savez_compressed with fixed member dates (zipfile would stamp the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    assert po.have_ref(), "oracle/_ref is not built (make -C oracle where the reference tree exists)"
    z = {}
    names = []
    for name, pb in cases():
        p = name + "_"
        pack(z, p, pb)
        run(z, p, pb)
        names.append(name)
    z["cases"] = np.array(names)
    z["relax"], z["iters"] = np.float32(RELAX), np.int32(T)
    for vs, f, x in filter_inputs():
        y, V = po.ref_lattice_filter(f, x)
        p = "filter%d_" % vs
        z[p + "features"], z[p + "x"], z[p + "y"], z[p + "V"] = f, x, y, np.int32(V)
    path = os.path.join(HERE, "labels.npz")
    save(path, z)
    print(path, os.path.getsize(path), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()

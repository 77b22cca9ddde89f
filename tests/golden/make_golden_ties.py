#!/usr/bin/env python3
"""Generate tests/golden/ties.npz from the REFERENCE itself (oracle/_ref: the reference's own DenseCRF headers compiled in place):
the cases of tests/lattice_tie_cases.py whose points sit on exact rounding ties and exact rank ties of the lattice build
(ties:d1 .. ties:d8, ties:slam256, ties:slam2047; not the 8192-point ones).

    python tests/golden/make_golden_ties.py

Inputs are stored with the results (tests/crf_cases.py: case_problem() decodes them); per case the reference's lattice internals
(V, norm, offset, bary, nbr) of every kernel, the Q trace (T = 3, relax 0.75) and the labels.  The archive is written with fixed
member dates, so running the script twice gives the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE]
import lattice_tie_cases as tc  # noqa: E402
import make_golden_labels as mgl  # noqa: E402
import pyoracle as po  # noqa: E402


def prefix(name):
    return name.replace(":", "_") + "_"


def main():
    assert po.have_ref(), "oracle/_ref is not built (make -C oracle where the reference tree exists)"
    z = {}
    for name in tc.GENERIC + tc.SLAM:
        pb = tc.problem(name)
        mgl.pack(z, prefix(name), pb)
        mgl.run(z, prefix(name), pb)
    z["cases"] = np.array(tc.GENERIC + tc.SLAM)
    z["relax"], z["iters"] = np.float32(mgl.RELAX), np.int32(mgl.T)
    path = os.path.join(HERE, "ties.npz")
    mgl.save(path, z)
    print(path, os.path.getsize(path), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()

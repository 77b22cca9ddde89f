"""Problems (tests/crf_cases.py) laid out as the inputs of one batch, and the ragged batches the batch tests share."""
import importlib

import numpy as np

import crf_cases as cc

pkg = importlib.import_module("lc-crf-slam_amd")


class Frames:
    """Problems laid out as one batch's inputs: [F][max_points][.] arrays, rows beyond a frame's points 0."""

    def __init__(self, probs, weights, max_points=None):
        self.probs, self.w = probs, [float(w) for w in weights]
        self.L = probs[0]["L"]
        self.N = np.array([pb["N"] for pb in probs], np.int32)
        self.maxN = int(max_points or self.N.max())
        self.dims = [f.shape[1] for f, _ in probs[0]["kernels"]]
        F = len(probs)
        self.U = np.zeros((F, self.maxN, self.L), np.float32)
        self.feats = [np.zeros((F, self.maxN, d), np.float32) for d in self.dims]
        for f, pb in enumerate(probs):
            self.U[f, :pb["N"]] = cc.raw_unary(pb)
            for k, (ft, _) in enumerate(pb["kernels"]):
                self.feats[k][f, :pb["N"]] = ft
        self.K = len(self.dims)

    def batch(self, weights=None, max_frames=None, build=True):
        b = pkg.BatchCRF(max_frames or len(self.probs), self.maxN, self.L, self.dims, weights or self.w)
        b.set_inputs_host(self.N, self.feats, unary=self.U)
        if build:
            b.build()
        return b

    def handle(self, f):
        h = pkg.DenseCRFHIP(int(self.N[f]), self.L)
        h.set_unary(self.U[f, :self.N[f]])
        for k, (ft, _) in enumerate(self.probs[f]["kernels"]):
            h.add_pairwise(ft, self.w[k])
        return h

    def grad_prob(self, seed):
        """dL/dQ [F][max_points][L]; NaN beyond every frame's points (read there, it would poison the frame)"""
        G = np.random.default_rng(seed).standard_normal((len(self.probs), self.maxN, self.L)).astype(np.float32)
        for f, n in enumerate(self.N):
            G[f, n:] = np.nan
        return G


def slam_frames(golden, wl, Ns=(0, 5, 7, 1000, 1001, 2000, 2002, 3000)):
    """SLAM frames (two terms, L = 2): the golden slam cases where they exist, else wl.slam_problem; the TUM3 weights"""
    probs = []
    for i, n in enumerate(Ns):
        if n == 0:
            probs.append(cc.empty_problem(2, [2, 2]))
        elif "N%d_N" % n in golden["slam"].files:
            probs.append(cc.case_problem(golden["slam"], "N%d" % n))
        else:
            probs.append(wl.slam_problem(n, seed=20 + i))
    return Frames(probs, [wl.TUM3["w1"], wl.TUM3["w2"]])


def generic_frames(wl, Ns=(300, 0, 1500, 77, 2500)):
    probs = [wl.generic_problem(n, [3], 3, seed=40 + i) if n else cc.empty_problem(3, [3]) for i, n in enumerate(Ns)]
    return Frames(probs, [2.5])


def label_frames(L, Ns, seed):
    """ragged frames of eight terms (d = 1 .. 8, tests/crf_cases.py: label_problem) with the first frame's weights"""
    EIGHT = list(range(1, 9))
    probs = [cc.label_problem(n, L, EIGHT, seed=seed + i) if n else cc.empty_problem(L, EIGHT) for i, n in enumerate(Ns)]
    w = [float(x) for _, x in probs[0]["kernels"]]
    return Frames([dict(pb, kernels=[(f, x) for (f, _), x in zip(pb["kernels"], w)]) for pb in probs], w)

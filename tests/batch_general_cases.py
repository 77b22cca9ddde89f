"""What the tests of batches with label-compatibility matrices or normalisation modes share (include/lccrf.h section 2g;
tests/test_batch_general.py): the batches, the float32 restatement of every frame's trace under every setting -- computed once,
shared by the tests, never changed -- and what the launchers must report for them.

The frames and the settings are those of tests/test_fused_general.py (imported, not copied); the reference of a frame is its own
restated trace (normalization_checker.restate_trace_f32), a handle holding the same frame with the same settings the second
witness.  A model is global: one weight, one matrix and one mode per term for every frame of a batch."""
import importlib

import numpy as np

import converge_cases as cv
import crf_cases as cc
import normalization_checker as nc
import test_fused_general as fg

F32 = np.float32
LANES, MAX_POINTS, CAP = fg.LANES, fg.MAX_POINTS, cv.CAP
EMPTY = "empty"
ORDERS = {"": [0, 1], "appearance": [0], "smooth": [1], "smooth_first": [1, 0]}

# Two points per lane: the sizes around the lane count and the kernel's last frame, an empty frame in the middle.  One point per
# lane: the frames of at most 1024 points from that list, plus a second 1001-point frame.
FRAMES = {
    "two": ("N5", "N7", "slam:N1001", "N1024", EMPTY, "N1025", "c2", "N2048"),
    "one": ("N5", "N7", "slam:N1001", EMPTY, "N1024", "N1001"),
}
BATCHES = {"%s/%s" % (fl, order): (FRAMES[fl], order) for fl in FRAMES for order in ORDERS}
# (K, points per lane, kernel 0 on chain rows) each is there for: the eight instantiations of k_general and k_general_converge
WANT = {"two/": (2, 2, 1), "one/": (2, 1, 1), "two/appearance": (1, 2, 1), "one/appearance": (1, 1, 1),
        "two/smooth": (1, 2, 0), "one/smooth": (1, 1, 0), "two/smooth_first": (2, 2, 0), "one/smooth_first": (2, 1, 0)}
# One shared product buffer and the copy loops beyond the prologue's register rounds.  sparse:N1100 (3300 + ~600 vertices) next to
# c2 (2000 points, ~1160 vertices on the second term) is a plan of 178 KiB: beyond one workgroup's LDS, so that batch streams; next
# to the 1025-point frame the plan fits with ONE product buffer for both terms, and the kernel takes it.
SPARSE = {"sparse+c2": (("sparse:N1100", EMPTY, "c2"), ""), "sparse+N1025": (("sparse:N1100", EMPTY, "N1025"), "")}
MAX_POINTS_SLACK = 7                                              # max_points of every batch is larger than its largest N

_BASE = {}


def base(name, golden, po, wl):
    """a frame with both its terms: (problem, raw unary, the two norms, the two vertex counts, the two longest splat rows)"""
    if name not in _BASE:
        pb = fg._problem(name, golden, po, wl)
        o = cc.setup(po.OracleCRF, pb)
        U = o.unary()
        ks = [o.kernel(k) for k in range(2)]
        o.close()
        rows = [int(np.bincount(k["offset"].reshape(-1), minlength=max(k["V"], 1)).max()) for k in ks]
        for a in [U] + [k["norm"] for k in ks]:
            a.setflags(write=False)
        _BASE[name] = (pb, U, [k["norm"] for k in ks], [k["V"] for k in ks], rows)
    return _BASE[name]


class Batch:
    """the frames of a batch with the terms taken in `order`: per frame None (empty) or (N, U, features, norms)"""

    def __init__(self, name, frames, order, golden, po, wl):
        self.name, self.order = name, ORDERS[order]
        self.K = len(self.order)
        self.frames, V, rows = [], [[0] for _ in self.order], [0]
        self.w0 = None
        for fn in frames:
            if fn == EMPTY:
                self.frames.append(None)
                continue
            pb, U, nrm, v, r = base(fn, golden, po, wl)
            self.frames.append((pb["N"], U, [pb["kernels"][k][0] for k in self.order], [nrm[k] for k in self.order]))
            for i, k in enumerate(self.order):
                V[i].append(v[k])
            rows.append(r[self.order[0]])
            if self.w0 is None or pb["N"] >= self.largest[0]:
                self.largest, self.w0 = self.frames[-1], [pb["kernels"][k][1] for k in self.order]
        self.N = np.array([fr[0] if fr else 0 for fr in self.frames], np.int32)
        self.maxN = int(self.N.max()) + MAX_POINTS_SLACK
        self.maxV, self.row0 = [max(v) for v in V], max(rows)

    def shape(self):
        """(K, points per lane, kernel 0 on chain rows) batch-wide, csrc/fused_loop.h: a lane owns ceil(largest N / 1024) points;
        kernel 0 takes chain rows when its longest row over the batch has at least 64 products and its largest V is at most 464"""
        return self.K, (int(self.N.max()) + LANES - 1) // LANES, int(self.row0 >= 64 and self.maxV[0] <= 464)

    def lds_plan(self, extra=0):
        """csrc/fused_loop.h: layout_core for the batch -- (fits one workgroup's 160 KiB with `extra` bytes behind it, every term
        has a product buffer of its own)"""
        a16 = lambda b: (b + 15) & ~15
        NA, chain0 = int(self.N.max()), self.shape()[2]
        fixed, prods = 128 + 64, []
        for k, v in enumerate(self.maxV):
            floats = (NA * 3 + (14 * v + 16 if k == 0 and chain0 else 0) + 63) & ~63
            fixed += 2 * a16((v + 1) * 8) + a16(3 * v * 4) + a16((v + 2) * 2)
            prods.append(a16(floats * 8))
        if fixed + sum(prods) + extra <= 160 * 1024:
            return True, True
        return fixed + max(prods) + extra <= 160 * 1024, False

    def weights(self, modes):
        """one float32 weight per term for every frame: normalization_checker.weights_f32 on the largest frame (a term in mode NONE
        has its weight scaled by the mean of that frame's norm; smaller frames have larger norms and fewer neighbours)"""
        pb = dict(kernels=[(None, w) for w in self.w0])
        return nc.weights_f32(pb, self.largest[3], modes)

    def inputs(self):
        """(n_points, features per term [F][maxN][2], unary [F][maxN][2]) as lccrf_batch_set_inputs_host takes them"""
        F = len(self.frames)
        feats = [np.zeros((F, self.maxN, 2), F32) for _ in range(self.K)]
        unary = np.zeros((F, self.maxN, 2), F32)
        for f, fr in enumerate(self.frames):
            if fr:
                n, U, ft, _ = fr
                unary[f, :n] = U
                for k in range(self.K):
                    feats[k][f, :n] = ft[k]
        return self.N, feats, unary


_BATCHES, _TRACES = {}, {}


def batch(name, golden, po, wl):
    if name not in _BATCHES:
        frames, order = {**BATCHES, **SPARSE}[name]
        _BATCHES[name] = Batch(name, frames, order, golden, po, wl)
    return _BATCHES[name]


def setting(bt, sname):
    """(modes, matrices, weights) of fg._settings' entry for the batch's term count"""
    modes, mats = fg._settings(bt.K)[sname]
    return modes, mats, bt.weights(modes)


def is_general(modes, mats):
    return any(m != nc.AFTER for m in modes) or any(m is not None for m in mats)


def traces(bt, sname, relax, T=CAP, weights=None):
    """per frame the restated trace [Q_0 .. Q_T] (an empty frame: T + 1 arrays of no rows)"""
    key = (bt.name, sname, relax, T, None if weights is None else tuple(float(w) for w in weights))
    if key not in _TRACES:
        modes, mats, w = setting(bt, sname)
        w = w if weights is None else [F32(x) for x in weights]
        out = []
        for fr in bt.frames:
            if fr is None:
                out.append([np.zeros((0, 2), F32)] * (T + 1))
                continue
            n, U, ft, nrm = fr
            tr = nc.restate_trace_f32(U, ft, w, mats, modes, T, relax, nrm)
            for q in tr:
                assert np.isfinite(q).all(), (bt.name, sname, relax)
                q.setflags(write=False)
            out.append(tr)
        _TRACES[key] = out
    return _TRACES[key]


def make(bt, modes, mats, weights, build=True, engine=None, max_frames=None):
    """a BatchCRF holding the batch's frames with the setting applied through the section 2g setters"""
    pkg = importlib.import_module("lc-crf-slam_amd")
    n, feats, unary = bt.inputs()
    b = pkg.BatchCRF(max_frames or len(bt.frames), bt.maxN, 2, [2] * bt.K, [float(w) for w in weights])
    if engine is not None:
        b.set_engine(engine)
    apply(b, modes, mats)
    b.set_inputs_host(n, feats, unary=unary)
    if build:
        b.build()
    return b


def apply(b, modes, mats):
    for k, m in enumerate(modes):
        b.set_normalization(k, m)
    for k, m in enumerate(mats):
        b.set_pairwise_compatibility(k, m)


def check_frames(b, bt, want_q, tag, bits=True):
    """Q bit for bit, the labels (compat_checker.map_of's rule: the first maximum wins) and the label bits of every frame"""
    import compat_checker as ck
    pkg = importlib.import_module("lc-crf-slam_amd")
    q, m = b.probability(), b.map()
    for f, want in enumerate(want_q):
        n = int(bt.N[f])
        assert cc.same_bits(q[f, :n], want), (tag, f, n, float(np.abs(q[f, :n] - want).max()) if n else 0)
        assert np.array_equal(m[f, :n], ck.map_of(want) if n else np.zeros(0, np.int16)), (tag, f)
    if bits:
        b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
        got = b.wait_download()["bits"]
        for f, want in enumerate(want_q):
            assert np.array_equal(got[f], cv.label_bits_of(want, got.shape[1])), (tag, f)


# ---- convergence ---------------------------------------------------------------------------------------------------------------
# (batch, setting, relax) of the converged tests: every instantiation of k_general_converge, the settings of the learnt models on the
# two batches of two-term frames.  With matrices on BOTH terms of a two-term frame the labels keep flipping and the cap ends the run:
# those are the cap frames; the frames of a few points settle at once.
CONVERGED = [("two/", "matrices", 1.0), ("two/", "mixed", 0.5), ("two/", "symmetric", 1.0),
             ("one/", "matrices", 0.5), ("one/", "mixed", 1.0),
             ("two/appearance", "none", 1.0), ("two/appearance", "mixed", 0.5),
             ("one/appearance", "none", 0.5), ("one/appearance", "matrices", 1.0),
             ("two/smooth", "symmetric", 1.0), ("two/smooth", "mixed", 1.0),
             ("one/smooth", "before", 0.5), ("one/smooth", "mixed", 0.5),
             ("two/smooth_first", "matrices", 1.0), ("two/smooth_first", "mixed", 1.0),
             ("one/smooth_first", "matrices", 1.0), ("one/smooth_first", "mixed", 0.5)]
# the frame whose stop the caps and the mid tolerance are taken from (index into the batch's frames): c2 / the second 1001-point frame
DESIGNATED = {"two": 6, "one": 5}


def converged_settings(trs, designated):
    """[(criterion, tol, cap)]: LABELS; DELTA at 1e-2 and at a mid tolerance of the designated frame's trace (between d_t and d_{t-1}
    at the first t >= 3 with d_t < d_{t-1}; a trace without one: 2e-2); BOTH; caps 0 and 1; one cap below and one above the
    designated frame's stop under LABELS.  No fixed 1e-3: it hits the cap on most two-term frames."""
    tr = trs[designated]
    d = cv.deltas(tr)
    t = next((t for t in range(3, CAP + 1) if d[t - 1] < d[t - 2]), None)
    mid = cv.mid_tol(tr, t) if t else F32(2e-2)
    out = [(cv.LABELS, F32(0), CAP), (cv.DELTA, F32(1e-2), CAP), (cv.DELTA, mid, CAP), (cv.BOTH, mid, CAP), (cv.LABELS, F32(0), 0),
           (cv.BOTH, F32(1e-2), 1)]
    stop = cv.expect(tr, cv.LABELS, F32(0), CAP)[0]
    if stop > 1:
        out.append((cv.LABELS, F32(0), stop - 1))
    if stop + 1 < CAP:
        out.append((cv.LABELS, F32(0), stop + 1))
    return out

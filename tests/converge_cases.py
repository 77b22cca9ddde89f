"""What the convergence tests (tests/test_converge.py) share: the contract of include/lccrf.h section 1h restated in numpy float32
on a trace Q_0 .. Q_cap, the cases, and their traces by the oracle -- computed once, shared by the tests, never changed.

    d_t = max |Q_t - Q_{t-1}|      one float32 subtraction and one abs per entry; the maximum of floats is exact
    c_t = points whose MAP label differs between Q_t and Q_{t-1}      np.argmax: the first maximum wins, as buildMap's rule
"""
import numpy as np

import crf_cases as cc

F32 = np.float32
DELTA, LABELS, BOTH = 1, 2, 3
CAP = 12
LANES = 1024


def deltas(trace):
    """d_1 .. d_cap as float32 (index t - 1)"""
    return np.array([np.abs(trace[t] - trace[t - 1]).max() if trace[t].size else F32(0) for t in range(1, len(trace))], F32)


def point_changes(trace, t):
    """per point max over the labels of |Q_t - Q_{t-1}|, float32"""
    return np.abs(trace[t] - trace[t - 1]).max(1)


def changed(trace, t):
    return int((np.argmax(trace[t], 1) != np.argmax(trace[t - 1], 1)).sum()) if trace[t].size else 0


def expect(trace, criterion, tol, cap, skip=None):
    """(iterations, delta as float32, changed, converged) of a run on `trace` (at least cap + 1 entries).
    skip: a point left out of both reductions -- what a kernel that dropped it would report."""
    assert len(trace) > cap
    tol = F32(tol)
    if cap == 0 or trace[0].shape[0] == 0:
        return 0, F32(0), 0, 0
    if skip is not None:
        trace = [np.delete(q, skip, 0) for q in trace]
    for t in range(1, cap + 1):
        d = np.abs(trace[t] - trace[t - 1]).max()
        assert d.dtype == F32
        c = changed(trace, t)
        met = (not (criterion & DELTA) or bool(d <= tol)) and (not (criterion & LABELS) or c == 0)
        if met or t == cap:
            return t, d, c, int(met)


def same_report(got, want):
    """exact: the counts, and the BITS of delta"""
    return (got["iterations"], got["changed"], got["converged"]) == (want[0], want[2], want[3]) and \
        np.array([got["delta"]], F32).view(np.int32)[0] == np.array([want[1]], F32).view(np.int32)[0]


def labels_of(q):
    return np.argmax(q, 1).astype(np.int16)


def label_bits_of(q, words):
    """the labels of a two-label Q, one bit per point (bit i % 64 of word i / 64), `words` uint64"""
    out = np.zeros(words, np.uint64)
    lab = labels_of(q)
    for i in np.nonzero(lab)[0]:
        out[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return out


def mid_tol(trace, t):
    """a tol strictly between d_t and d_{t-1} (d_t < d_{t-1} asserted): float32 midpoint"""
    d = deltas(trace)
    lo, hi = d[t - 1], d[t - 2]
    assert lo < hi, (t, lo, hi)
    m = F32((np.float64(lo) + np.float64(hi)) / 2)
    assert lo <= m < hi
    return m


# ---- the kernel path's cases: SLAM frames (workloads.slam_problem), terms by order -------------------------------------------
# name: (N, seed, the terms taken -- 0 appearance (long rows from ~1000 points on: chain rows), 1 smooth (short rows))
SIZES = (1, 2, 63, 64, 65, 1000, 1025, 2049, 3073, 4096)
CASES = {}
for _i, _n in enumerate(SIZES):
    CASES["N%d" % _n] = (_n, _i % 4, (0, 1))                      # K = 2
    CASES["N%d/appearance" % _n] = (_n, (_i + 1) % 4, (0,))       # K = 1
for _n, _s in ((1025, 2), (2049, 0), (3073, 3), (4096, 1)):       # kernel 0 on short rows at 2 .. 4 points per lane
    CASES["N%d/smooth_first" % _n] = (_n, _s, (1, 0))
    CASES["N%d/smooth" % _n] = (_n, _s, (1,))
RELAX = (1.0, 0.5)


def problem(wl, name):
    N, seed, order = CASES[name]
    pb = wl.slam_problem(N, seed=seed)
    return dict(pb, kernels=[pb["kernels"][k] for k in order])


_TRACES, _LATTICE = {}, {}


def oracle_trace(po, pb, relax, cap=CAP, cls=None):
    o = cc.setup(cls or po.OracleCRF, pb)
    tr = o.run_trace(cap, relax)
    o.close()
    return tr


def trace(po, wl, name, relax):
    key = (name, relax)
    if key not in _TRACES:
        _TRACES[key] = oracle_trace(po, problem(wl, name), relax)
        _TRACES[key].setflags(write=False)
    return _TRACES[key]


def want_shape(po, wl, name):
    """(points per lane, kernel 0 on chain rows) the launcher must report: csrc/fused_loop.h -- a lane owns ceil(N / 1024) points;
    kernel 0 takes chain rows when its longest splat row has at least 64 products and it has at most 464 vertices"""
    if name not in _LATTICE:
        pb = problem(wl, name)
        o = cc.setup(po.OracleCRF, pb)
        k0 = o.kernel(0)
        o.close()
        row0 = int(np.bincount(k0["offset"].reshape(-1), minlength=max(k0["V"], 1)).max())
        _LATTICE[name] = (max((pb["N"] + LANES - 1) // LANES, 1), int(row0 >= 64 and k0["V"] <= 464))
    return _LATTICE[name]


def settings(tr, N):
    """[(criterion, tol, cap)] of a case: DELTA at 0 and at a mid tol, LABELS, both bits; caps 0 and 1, one below the stop and one
    above it.  The mid tol is 1e-3 up to 2048 points; beyond, DELTA 1e-3 hits the cap of 12 in every frame, so it lies between two
    consecutive d_t of the oracle's trace (the first t >= 4 with d_t < d_{t-1})."""
    if N < 2049:
        mid = F32(1e-3)
    else:
        d = deltas(tr)
        t = next(t for t in range(4, CAP) if d[t - 1] < d[t - 2])
        mid = mid_tol(tr, t)
    out = [(DELTA, F32(0), CAP), (DELTA, mid, CAP), (LABELS, F32(0), CAP), (BOTH, mid, CAP), (LABELS, F32(0), 0), (BOTH, mid, 1)]
    for crit in (DELTA, LABELS):
        stop = expect(tr, crit, mid, CAP)[0]
        if stop > 1:
            out.append((crit, mid, stop - 1))                     # a cap below the stop
        if stop + 1 < CAP:
            out.append((crit, mid, stop + 1))                     # ... and one above it
    return out


# ---- a plan with no room for the reduction's words ---------------------------------------------------------------------------
# The converged kernels want 16 bytes of LDS behind the loop's plan (csrc/fused_loop.h: layout_core, kConvergeLds); a frame whose
# plan fills a workgroup's 160 KiB to the byte is one the fixed-count kernels take and the converged ones do not: their launchers
# return 0 and the call falls through to the streaming step.  Plans are multiples of 16 bytes, so that frame has to be built: 1025
# points (two per lane) dealt round robin over m far-apart sites per term -- every site a lattice cell of its own, V = 3 m, rows of
# at most two products -- with two product buffers of 8 * ceil64(3 * 1025) bytes.  (629, 631) sites: 163 840 bytes, the limit;
# (628, 631): 96 bytes below it, the nearest plan that still has room.
EDGE_N, EDGE_FULL, EDGE_ROOM, LDS_LIMIT = 1025, (629, 631), (628, 631), 160 * 1024


def edge_plan_bytes(N, V):
    """layout_core's total for lattices of V[k] vertices, every term with a product buffer of its own, no chain rows"""
    a16 = lambda b: (b + 15) & ~15
    tables = sum(2 * a16(8 * (v + 1)) + a16(12 * v) + a16(2 * (v + 2)) for v in V)
    return 128 + 64 + tables + len(V) * 8 * ((3 * N + 63) & ~63)


def edge_problem(sites, seed=11):
    """EDGE_N points, term k's features on sites[k] sites of a grid eight lattice units apart; random labels"""
    rng = np.random.default_rng([seed, EDGE_N])
    kernels = []
    for m in sites:
        side = int(np.ceil(np.sqrt(m)))
        site = np.arange(EDGE_N) % m
        f = np.stack([site % side, site // side], 1).astype(F32) * F32(8) + F32(0.25)
        kernels.append((f, F32(3.0)))
    return dict(N=EDGE_N, L=2, label=rng.integers(0, 2, EDGE_N).astype(np.int16), conf=F32(0.7), kernels=kernels)


# ---- the reduction's reach: cases in which ONE point decides -----------------------------------------------------------------
def deciding(tr, cap=8):
    """(t, point, tol) such that at iteration t the largest per-point change is alone above tol -- tol lies between it and the
    second largest -- and no earlier iteration stops with or without that point; None when the trace has no such iteration."""
    for t in range(2, cap):
        m = point_changes(tr, t)
        if m.size < 2:
            return None
        i1 = int(np.argmax(m))
        rest = np.delete(m, i1)
        m1, m2 = m[i1], rest.max()
        if not m2 < m1:
            continue
        tol = F32((np.float64(m1) + np.float64(m2)) / 2)
        if not (m2 <= tol < m1):
            continue
        if expect(tr, DELTA, tol, CAP, skip=i1)[0] == t and expect(tr, DELTA, tol, CAP)[0] > t:
            return t, i1, tol
    return None


def rolled(pb, shift):
    """the same frame with its points in another order: point i moves to (i + shift) % N"""
    r = lambda a: np.ascontiguousarray(np.roll(a, shift, 0))
    out = dict(pb, kernels=[(r(f), w) for f, w in pb["kernels"]])
    for k in ("label", "unary"):
        if k in pb:
            out[k] = r(pb[k])
    return out


def targets(N):
    """name -> index the deciding point is rolled to"""
    ppt = (N + LANES - 1) // LANES
    last_lane_with_point = min(N, LANES) - 1
    return {"first wavefront": 5,
            "last wavefront with a point": (last_lane_with_point // 64) * 64 + min(3, last_lane_with_point % 64),
            "last slot": (ppt - 1) * LANES + min(70, N - 1 - (ppt - 1) * LANES),
            "index N-1": N - 1}

"""The window splat's PLAN restated on the CPU, and the cases of tests/test_splat_window.py (notes/splat_window_tests.md).

With two labels, locality mode and the sorted build the streaming engine's splat takes the first blur passes along on an overlapped
LDS window (csrc/stream_filter.hip: k_splat2w).  How many passes, how wide a halo, which window and which instantiation follow from
numbers the build measures on the device (Engine::learn_sizes, csrc/host_engine.hip).  This module derives the same plan from the
FEATURES alone, in numpy:

  features (+ the phantom points of the last block of four)  ->  the lattice's vertices (scripts/sim_vertex_order.py, which
  tests/test_sim_vertex_order.py holds to the oracle's lattice)  ->  their coordinates in the basis of the blur directions  ->  ids in
  row-major order, coordinate 0 fastest  ->  per axis the largest id distance of a neighbour, over all frames of a batch  ->  the rule.

The rule's constants are READ from the sources (constants()), the rule itself is written out again here; nothing is taken from a
device run.  tests/test_splat_plan_cases.py checks the restatement and the case table without a GPU.
"""
import importlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lc-crf-slam_amd", "csrc")
if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))

PLAN_FIELDS = ("passes", "halo", "window", "lanes", "vertices_per_lane", "long_mode")


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: %d matches of %r (the plan rule's code changed shape: restate it here)" % (what, len(m), pattern)
    return m[0]


_constants = None


def constants():
    """the numbers of the plan rule, from the code as it stands"""
    global _constants
    if _constants is None:
        src = {n: open(os.path.join(CSRC, n)).read() for n in ("engine.h", "host_engine.h", "host_engine.hip")}
        c = {}
        for name, f in (("kNdistAxes", "engine.h"), ("kLongRowMin", "engine.h"), ("kLongRowListMinPoints", "engine.h"),
                        ("kSplatWideMaxFrames", "engine.h"), ("kSplatNarrowLanes", "engine.h"), ("kPermMinPointsDefault", "host_engine.h")):
            c[name] = int(_one(r"constexpr int %s = (\d+);" % name, src[f], name))
        hs = src["host_engine.hip"]
        cut, win, div = _one(r"nd\[j\] < 1 \|\| nd\[j\] > (\d+) \|\| halo \+ nd\[j\] > (\d+) / (\d+)\) break;", hs, "the halo rule")
        c["max_dist"], c["max_window"], c["halo_share"] = int(cut), int(win), int(div)
        c["max_passes"] = int(_one(r"const int cap = env_sp \? atoi\(env_sp\) : (\d+);", hs, "the pass cap"))
        _one(r"j < std::min\(kd\.D1, std::min\(cap, 3\)\)", hs, "the pass loop")
        steps = _one(r"kd\.splat_block = kd\.splat_halo \* (\d+) <= (\d+) \? (\d+) : kd\.splat_halo \* (\d+) <= (\d+) \? (\d+) : (\d+);", hs, "the window steps")
        s = [int(x) for x in steps]
        assert s[0] == s[3] == c["halo_share"] and s[1] == s[2] and s[4] == s[5] and s[6] == c["max_window"], steps
        c["windows"] = (s[2], s[5], s[6])
        c["demote_above_D1"] = int(_one(r"if \(kd\.splat_passes == 2 && kd\.nbr2 && kd\.D1 > (\d+)\) \{ kd\.splat_passes = 1; kd\.splat_halo = 1; \}", hs, "the demotion"))
        _one(r"if \(Fcap == 1 && L == 2 && allow_perm && \(rc = mem\.alloc\(&k\.nbr2,", hs, "the two-hop table's condition")
        c["long_per_row"] = int(_one(r"kd\.long_mode = kd\.longrow_ok && \(nlong > 0 \|\| \(long\)NAr \* kd\.D1 > (\d+)L \* std::max\(m, 1\)\);", hs, "long_mode"))
        c["long2_per_row"] = int(_one(r"if \(kd\.long_mode && \(long\)NAr \* kd\.D1 >= (\d+)L \* std::max\(m, 1\)\) kd\.long_mode = 2;", hs, "long_mode 2"))
        _one(r"if \(maxN > kLongRowListMinPoints\) \{", hs, "the lists' condition")
        _constants = c
    return _constants


def sim():
    return importlib.import_module("sim_vertex_order")


class Lattice:
    """One frame's lattice in the numbering of the sorted build: V vertices, coords [V][d] in the basis of the blur directions, ids in
    row-major order (coordinate 0 fastest), nbr[j] = id of the axis-j neighbour n2 of every vertex or -1 (n1 is the inverse relation),
    rows[v] = number of REAL points' entries of vertex v (phantom points add vertices, not products)."""

    def __init__(self, f):
        f = np.ascontiguousarray(f, np.float32)
        N, d = f.shape
        D1 = d + 1
        self.N, self.d = N, d
        pad = (-N) % 4
        fp = np.concatenate([f, np.zeros((pad, d), np.float32)]) if pad else f
        keys, _ = sim().lattice(fp)
        flat = keys.reshape(-1, d)
        # the sorted build hands a frame to the hash build when a key COULD leave int16 (k_points, conservative): no plan then
        scale = np.array([1.0 / np.sqrt((i + 2.0) * (i + 1.0)) * np.sqrt(2.0 / 3.0) * D1 for i in range(d)])
        lim = float(_one(r"if \(!\(mag \* \(float\)D1 < (\d+)\.0f\) && vbad\) \*vbad = 1;", open(os.path.join(CSRC, "stream_build.hip")).read(), "the key range check"))
        self.sortable = bool(((2.0 + (np.abs(fp.astype(np.float64)) * scale).sum(1)) * D1).max() < lim * (1 - 1e-4))
        assert np.abs(flat).max() < 32767
        uk, inv = np.unique(sim().pack(flat), return_inverse=True)
        inv = inv.reshape(-1)
        V = len(uk)
        ukeys = np.zeros((V, d), np.int64)
        ukeys[inv] = flat
        xd = -ukeys.sum(1)
        assert np.all((xd[:, None] - ukeys) % D1 == 0)
        c = (xd[:, None] - ukeys) // D1
        order = np.lexsort(tuple(c[:, j] for j in range(d)))           # (the last key is the primary one: coordinate d-1 slowest)
        ids = np.empty(V, np.int64)
        ids[order] = np.arange(V)
        self.V = V
        self.coords = c[order]
        self.entry_vertex = ids[inv].reshape(-1, D1)                   # [N + pad][d+1]
        self.rows = np.bincount(self.entry_vertex[:N].ravel(), minlength=V)
        # neighbours by coordinate: a code that is injective on the box (one guard column per side)
        lo = self.coords.min(0) - 1
        span = self.coords.max(0) - lo + 2
        stride = np.concatenate([[1], np.cumprod(span[:-1])]).astype(np.int64)
        assert float(np.prod(span.astype(np.float64))) < 2.0 ** 62
        code = ((self.coords - lo) * stride).sum(1)
        assert np.all(np.diff(code) > 0), "ids must follow the row-major codes"
        self.nbr = []
        for j in range(D1):
            step = stride[j] if j < d else -stride.sum()
            t = code + step
            pos = np.minimum(np.searchsorted(code, t), V - 1)
            self.nbr.append(np.where(code[pos] == t, pos, -1))

    def ndist(self, j):
        n = self.nbr[j]
        ok = n >= 0
        return int(np.abs(n[ok] - np.nonzero(ok)[0]).max()) if ok.any() else 0


def window_shape(window, F):
    """(lanes, vertices per lane) of the instantiation k_splat2w<lanes, per lane> for a window with F frames in flight"""
    c = constants()
    w256, w512, w1024 = c["windows"]
    assert (w256, w512, w1024, c["kSplatNarrowLanes"]) == (256, 512, 1024, 256), "the table below is written for these"
    few = F <= c["kSplatWideMaxFrames"]
    return {256: (256, 1),
            512: (512, 1) if few else (256, 2),
            1024: (512, 2) if F == 1 else (1024, 1) if few else (256, 4)}[window]


def plan_of(lattices, max_points, max_frames, passes_cap=None):
    """The plan of one term for the frames `lattices` (None = an empty frame) on an engine of capacity max_frames x max_points with
    two labels: the dict lccrf_batch_get_splat_plan fills, plus what it was derived from (nd, V, entries per row)."""
    c = constants()
    live = [l for l in lattices if l is not None]
    F, d = len(lattices), live[0].d
    D1 = d + 1
    NA = max(l.N for l in live)
    maxV = max(l.V for l in live)
    nd = [0] + [max(l.ndist(j) for l in live) for j in range(1, min(D1, c["kNdistAxes"]))]
    cap = c["max_passes"] if passes_cap is None else passes_cap
    passes, halo, window = 1, 1, 0
    if cap >= 2:
        h = 1
        for j in range(1, min(D1, cap, 3)):
            if nd[j] < 1 or nd[j] > c["max_dist"] or h + nd[j] > c["max_window"] // c["halo_share"]:
                break
            h += nd[j]
            passes, halo = j + 1, h
        if passes == 2 and max_frames == 1 and D1 > c["demote_above_D1"]:       # (the two-hop table pairs the passes (1,2), (3,4) ...)
            passes, halo = 1, 1
        if passes >= 2:
            window = next(w for w in c["windows"] if halo * c["halo_share"] <= w)
    lists = max_points > c["kLongRowListMinPoints"]
    nlong = max(int((l.rows > c["kLongRowMin"]).sum()) for l in live)
    long_mode = 0
    if lists and (nlong > 0 or NA * D1 > c["long_per_row"] * maxV):
        long_mode = 2 if NA * D1 >= c["long2_per_row"] * maxV else 1
    if long_mode:
        passes, halo, window = 0, 0, 0
    lanes, per = window_shape(window, F) if window else (0, 0)
    return dict(passes=passes, halo=halo, window=window, lanes=lanes, vertices_per_lane=per, long_mode=long_mode,
                nd=nd, maxV=maxV, per_row=NA * D1 / maxV, F=F, D1=D1)


def cross_edge_windows(lat, plan):
    """For the window splat of `plan` on frame `lat`: the workgroups (windows) that own a vertex one of whose neighbours along a pass
    of the window (axis 1; axis 2 with three passes) is owned by ANOTHER workgroup -- the value comes through the halo.
    -> (number of windows, sorted list of such windows)"""
    core = plan["window"] - 2 * plan["halo"]
    nw = (lat.V + core - 1) // core
    hit = set()
    v = np.arange(lat.V)
    for j in range(1, plan["passes"]):
        n = lat.nbr[j]
        ok = n >= 0
        a, b = v[ok] // core, n[ok] // core
        hit.update(a[a != b].tolist())                                 # v's n2 lies in another window ...
        hit.update(b[a != b].tolist())                                 # ... and v is that vertex's n1
    return nw, sorted(hit)


def halo_reach(lat, plan):
    """the farthest id distance from a vertex to anything its value after the window's passes depends on: must not exceed the halo"""
    V = lat.V
    lo = np.arange(V)
    hi = np.arange(V)
    for j in range(plan["passes"]):
        n2 = lat.nbr[j]
        n1 = np.full(V, -1, np.int64)
        n1[n2[n2 >= 0]] = np.nonzero(n2 >= 0)[0]
        nlo, nhi = lo.copy(), hi.copy()
        for n in (n1, n2):
            ok = n >= 0
            nlo[ok] = np.minimum(nlo[ok], lo[n[ok]])
            nhi[ok] = np.maximum(nhi[ok], hi[n[ok]])
        lo, hi = nlo, nhi
    return int(max((np.arange(V) - lo).max(), (hi - np.arange(V)).max()))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def box(n, sides, seed):
    """n points uniform in a box of feature space with the given sides: about two entries per lattice row at n ~ 8200 and a volume of
    ~13000 (2-D), which keeps the kernel away from the coarse-kernel rule.  The box starts at the origin; a side beyond 20000 is
    centred there (the lattice's keys are int16)."""
    rng = np.random.default_rng([int(seed), int(n)] + [int(round(8 * s)) for s in sides])
    side = np.asarray(sides, np.float64)
    return ((rng.uniform(0.0, 1.0, (n, len(sides))) - (side > 20000.0) * 0.5) * side).astype(np.float32)


def unary_of(n, seed):
    rng = np.random.default_rng([77, int(seed), int(n)])
    return (np.round(rng.uniform(0.05, 3.0, (n, 2)) * 256) / 256).astype(np.float32)


N0 = 8200          # points of a full frame (the locality threshold is 8192)


class Case:
    """One row of the table.  frames: per frame a list of per-term features; api: "batch" or "object"; env: switches of the
    instrumented library (a child process); classes: what the row is in the table for, checked by the CPU test."""

    def __init__(self, name, terms, frames, classes, api="batch", passes_cap=None, weights=None):
        self.name, self.terms, self.classes, self.api, self.passes_cap = name, terms, set(classes), api, passes_cap
        self.frame_specs = frames               # per frame: (n, seed) or None (empty); terms: per term the box sides
        self.weights = weights or [3.0 if i == 0 else 2.0 for i in range(len(terms))]
        self._frames = self._lat = None

    @property
    def F(self):
        return len(self.frame_specs)

    @property
    def max_points(self):
        return max(s[0] for s in self.frame_specs if s)

    def sides(self, k, f):
        t = self.terms[k]
        return t[f] if isinstance(t[0], (list, tuple)) else t

    def frames(self):
        """per frame: None or dict(N, unary, kernels=[(features, w) ...], L=2)"""
        if self._frames is None:
            out = []
            for f, spec in enumerate(self.frame_specs):
                if not spec:
                    out.append(None)
                    continue
                n, seed = spec
                out.append(dict(N=n, L=2, unary=unary_of(n, seed),
                                kernels=[(box(n, self.sides(k, f), seed + 100 * k), np.float32(self.weights[k])) for k in range(len(self.terms))]))
            self._frames = out
        return self._frames

    def lattices(self, k):
        if self._lat is None:
            self._lat = {}
        if k not in self._lat:
            self._lat[k] = [Lattice(fr["kernels"][k][0]) if fr else None for fr in self.frames()]
        return self._lat[k]

    def plan(self, k=0):
        assert all(l.sortable for l in self.lattices(k) if l), "a key could leave int16: the device falls back to the hash build"
        assert self.max_points >= constants()["kPermMinPointsDefault"], "below the locality threshold: no sorted build"
        return plan_of(self.lattices(k), self.max_points, self.F, self.passes_cap)

    def env(self):
        return {"LCCRF_SPLAT_PASSES": str(self.passes_cap)} if self.passes_cap is not None else {}


def _f(n=N0, seed=1):
    return (n, seed)


def _same(F, n=N0, step=37, seed=1):
    return [(n - step * f, seed + f) for f in range(F)]


# (sides a x b of the 2-D boxes: a*b ~ 13000; nd1 ~ a, nd2 = nd1 + 1, so halo ~ 2a + 2)
W256, W512, W1024 = (8.0, 1625.0), (20.0, 650.0), (30.0, 433.0)
CASES = [
    # windows 256 / 512 / 1024 at one, two and three frames in flight: all six instantiations
    Case("w256_F1", [W256], _same(1), {"window256", "F1", "P3", "P==D1"}),
    Case("w256_F2", [W256], _same(2), {"window256", "F2"}),
    Case("w256_F3", [W256], _same(3), {"window256", "F3"}),
    Case("w512_F1", [W512], _same(1), {"window512", "F1"}),
    Case("w512_F2", [W512], _same(2), {"window512", "F2"}),
    Case("w512_F3", [W512], _same(3), {"window512", "F3"}),
    Case("w1024_F1", [W1024], _same(1), {"window1024", "F1"}),
    Case("w1024_F2", [W1024], _same(2), {"window1024", "F2"}),
    Case("w1024_F3", [W1024], _same(3), {"window1024", "F3"}),
    Case("w512_F8", [W512], _same(8), {"window512", "F8"}),
    # the window steps, either side
    Case("halo_32", [(12.5, 1040.0)], _same(1), {"halo<=32"}),
    Case("halo_34", [(13.5, 963.0)], _same(1), {"halo>=33"}),
    Case("halo_64", [(26.0, 500.0)], _same(2), {"halo<=64"}),
    Case("halo_66", [(27.0, 481.0)], _same(2), {"halo>=65"}),
    Case("halo_31_d3", [(5.5, 5.5, 3570.25)], _same(1, seed=1), {"halo<=32", "d3", "odd_halo"}),
    Case("halo_33_d3", [(5.5, 5.5, 3570.25)], _same(1, seed=2), {"halo>=33", "d3", "odd_halo"}),
    # the halo + nd <= 128 break and the 127 cut
    Case("sum_below_128", [(400.0, 30.0)], _same(2), {"sum<=128"}),
    Case("sum_above_128", [(60.0, 200.0)], _same(2), {"sum>128", "P2"}),
    Case("nd1_120_127", [(118.0, 110.0)], _same(2), {"nd1_120_127", "P2"}),
    Case("nd1_above_127", [(150.0, 87.0)], _same(2), {"nd1>127", "P1"}),
    # P == D1 at d = 1; d = 3 and d = 4 (three passes leave one and two passes behind)
    Case("d1", [(27000.0,)], _same(2, seed=4), {"d1", "P==D1"}),
    Case("d3_F3", [(6.0, 6.0, 3000.0)], _same(3), {"d3", "P3", "left_odd"}),
    Case("d4_F1", [(4.0, 4.0, 4.0, 3000.0)], _same(1, seed=7), {"d4", "P3", "left_even", "F1"}),
    Case("d4_F3", [(4.0, 4.0, 4.0, 3000.0)], _same(3), {"d4", "P3", "left_even"}),
    # a single-frame engine demotes two passes to one at d >= 3: naturally (halo + nd2 > 128) and under the pass cap
    Case("demoted_d3", [(40.0, 40.0, 80.0)], _same(1), {"demoted"}),
    Case("cap2_d3", [(6.0, 6.0, 3000.0)], _same(1), {"demoted", "cap2"}, passes_cap=2),
    Case("cap2_w256", [W256], _same(2), {"cap2", "window256", "P2", "P==D1-1"}, passes_cap=2),
    Case("cap2_w512", [W512], _same(1), {"cap2", "P2", "F1"}, passes_cap=2),
    Case("cap2_w1024", [W1024], _same(3), {"cap2", "window512", "P2", "F3"}, passes_cap=2),
    # a coarse 2-D kernel beside a non-coarse one
    Case("coarse_beside", [W512, (30.0, 30.0)], _same(2), {"coarse"}),
    # batches of three: narrow, empty, wide and shorter -- and the wide frame first
    Case("mixed_narrow_first", [[(8.0, 400.0), (8.0, 400.0), W1024]], [_f(N0, 1), None, _f(N0 - 300, 3)], {"mixed"}),
    Case("mixed_wide_first", [[W1024, (8.0, 400.0), (8.0, 400.0)]], [_f(N0 - 300, 3), None, _f(N0, 1)], {"mixed"}),
    # the object API: one handle of >= 8192 points
    Case("object_w512", [W512], _same(1), {"object"}, api="object"),
]
BY_NAME = {c.name: c for c in CASES}
NO_WINDOW = {"P1", "demoted"}                   # classes whose cases run without a window (one pass in the splat)
# the same batch handle with new inputs: wide, narrow, wide
REBUILD_SEQUENCE = ["w1024_F2", "w256_F2", "w1024_F2"]


# ---- the device side (tests/test_splat_window.py; also run in a child process under a switch of the instrumented library) -------

def batch_inputs(case):
    """(n_points [F], per term [F][max_points][d] features, [F][max_points][2] unaries) of a case's frames"""
    frames, F, maxN = case.frames(), case.F, case.max_points
    npts = [fr["N"] if fr else 0 for fr in frames]
    dims = [len(case.sides(k, 0)) for k in range(len(case.terms))]
    feats = [np.zeros((F, maxN, d), np.float32) for d in dims]
    unary = np.zeros((F, maxN, 2), np.float32)
    for f, fr in enumerate(frames):
        if fr:
            unary[f, :fr["N"]] = fr["unary"]
            for k in range(len(dims)):
                feats[k][f, :fr["N"]] = fr["kernels"][k][0]
    return npts, dims, feats, unary


ITERATIONS, RELAX = 3, 0.9


def run_batch(case, b=None):
    """Build the case's frames on a BatchCRF (a new one of exactly the case's capacity, or `b`), read the plan, run the inference
    twice.  -> dict of arrays: plan [K][6], V [K][F], engine, locality [2], Q and map of either run."""
    pkg = importlib.import_module("lc-crf-slam_amd")
    npts, dims, feats, unary = batch_inputs(case)
    own = b is None
    if own:
        b = pkg.BatchCRF(case.F, case.max_points, 2, dims, [float(w) for w in case.weights])
    b.set_inputs_host(npts, feats, unary=unary)
    b.build()
    out = dict(plan=np.array([[b.splat_plan(k)[n] for n in PLAN_FIELDS] for k in range(len(dims))], np.int64))
    for rep in range(2):
        b.inference(ITERATIONS, True, RELAX)
        out["Q%d" % rep], out["map%d" % rep] = b.probability().copy(), b.map().copy()
    out["plan_after"] = np.array([[b.splat_plan(k)[n] for n in PLAN_FIELDS] for k in range(len(dims))], np.int64)
    out["V"] = np.array([b.lattice_sizes(k) for k in range(len(dims))], np.int64)
    out["engine"] = np.int64(b.engine())
    out["locality"] = np.array(b.locality_mode(), np.int64)
    if own:
        b.close()
    return out


if __name__ == "__main__":                      # child process: python splat_plan_cases.py <case> <out.npz>
    sys.path[:0] = [ROOT]
    np.savez(sys.argv[2], **run_batch(BY_NAME[sys.argv[1]]))

"""The two-label step's BLUR plan restated on the CPU, and the cases of tests/test_blur_plan.py (notes/blur_plan_tests.md).

The streaming engine runs the d + 1 blur passes of a two-label term on six routes -- in the splat, two per launch off the two-hop table
(k_blur2x2t) or without one (k_blur2x2), alone on 32-bit ids (k_blur2<NT>) or on the compact 16-bit table (k_blur2c), in the slice
(k_slice2<D1, true>) -- chosen by one host rule (csrc/engine.h: blur_plan) from the number of frames in flight, the largest lattice, the
tables the engine allocated and the build filled, and the passes the splat takes along.  All routes give the same bits, so a test sees a
wrong route only if it reaches that route.  This module derives the plan a case must report from its FEATURES alone:

  features -> the lattice (tests/splat_plan_cases.py: V per frame, neighbours, ids of the sorted build) -> which build the engine takes,
  which tables exist and hold (expected_plans) -> the splat's passes (splat_plan_cases.plan_of) -> the rule, written out again (route_counts).

The rule's constants and the tables' conditions are READ from the sources (constants()); nothing is taken from a device run.
tests/test_blur_plan_cases.py checks the case table without a GPU.
"""
import importlib
import os
import sys

import numpy as np

import splat_plan_cases as sp
from splat_plan_cases import ROOT, CSRC, _one

PLAN_FIELDS = ("in_splat", "paired_table", "paired_plain", "alone_32bit", "alone_compact", "in_slice", "nontemporal", "first_table_pair")
ROUTES = PLAN_FIELDS[:6]
# the A/B switches of the instrumented library that bear on the plan
SWITCHES = ("LCCRF_NO_PAIR_FUSE", "LCCRF_NO_2HOP_TABLE", "LCCRF_NO_COMPACT_NBR", "LCCRF_NBRC_SPAN", "LCCRF_FAST0_BREAK", "LCCRF_SPLAT_PASSES")

_constants = None


def constants():
    """the numbers and conditions of the route rule, from the code as it stands"""
    global _constants
    if _constants is None:
        src = {n: open(os.path.join(CSRC, n)).read() for n in ("engine.h", "host_engine.hip", "stream_build.hip", "build_small.hip")}
        c = {}
        for name in ("kSliceBlurMaxFrames", "kPairFuseMaxFrames", "kBlurNtMinFrames", "kNbrcMinFrames", "kNbrcMaxFrames", "kNbrcBlock"):
            c[name] = int(_one(r"constexpr int %s = (\d+);" % name, src["engine.h"], name))
        c["kPairFuseMaxVertices"] = int(_one(r"constexpr long kPairFuseMaxVertices = (\d+);", src["engine.h"], "the vertex bound"))
        _one(r"return F <= kPairFuseMaxFrames \|\| \(long\)F \* maxV <= kPairFuseMaxVertices;", src["engine.h"], "pair_fuse")
        lo, hi = _one(r"const bool in_slice = D1 <= (\d+) && j0 < D1 && \(pairs \? \(\(D1 - j0\) & 1\) && D1 >= (\d+) : F <= kSliceBlurMaxFrames\);",
                      src["engine.h"], "the slice rule")
        c["slice_max_D1"], c["slice_min_D1"] = int(lo), int(hi)
        c["demote_above_D1"] = sp.constants()["demote_above_D1"]                   # (single frames: two passes in the splat become one)
        hs = src["host_engine.hip"]
        # the two-hop table: engines of ONE frame, two labels; valid behind the streaming build
        _one(r"if \(Fcap == 1 && L == 2 && allow_perm && \(rc = mem\.alloc\(&k\.nbr2,", hs, "the two-hop table's condition")
        _one(r"kernels\[k\]\.dev\.nbr2_ok = kernels\[k\]\.dev\.nbr2 != nullptr;", hs, "nbr2_ok")
        _one(r"for \(int u = 0; u < m; \+\+u\) kernels\[k \+ u\]\.dev\.nbr2_ok = kernels\[k \+ u\]\.dev\.nbrc_ok = kernels\[k \+ u\]\.dev\.fast0_ok = ", hs,
             "the one-workgroup build leaves no table")
        _one(r"kernels\[k\]\.dev\.nbr2_first = kernels\[k\]\.dev\.fast0_ok;", hs, "nbr2_first")
        # the tables of the sorted build: engines for frames of the locality threshold and more; the compact one from kNbrcMinFrames frames
        _one(r"if \(L == 2 && allow_perm && maxN >= perm_min_points\(\)\) \{", hs, "the sorted build's tables")
        _one(r"if \(k\.tbl_bad && Fcap >= kNbrcMinFrames\) \{", hs, "the compact table's condition")
        _one(r"kernels\[k\]\.dev\.nbrc_ok = kernels\[k\]\.dev\.nbrc != nullptr && kernels\[k\]\.dev\.vorder && F >= kNbrcMinFrames && F <= kNbrcMaxFrames;", hs, "nbrc_ok")
        _one(r"kernels\[k\]\.dev\.fast0_ok = kernels\[k\]\.dev\.tbl_bad != nullptr && kernels\[k\]\.dev\.vorder;", hs, "fast0_ok")
        _one(r"const bool want = allow_perm && !no_perm && !perm_banned && \(!perm_scoped \|\| may_reorder\) && n > 0 && n == \(int\)kernels\.size\(\) && NAp >= perm_min_points\(\);",
             hs, "locality mode")
        _one(r"vorder_on = want && !vorder_broken && vo != 2;", hs, "the sorted build's condition")
        _one(r"const bool small_ok = !no_small && !perm_on;", hs, "the one-workgroup build's condition")
        c["span_limit"] = int(_one(r"int limit = (0x[0-9a-f]+);", src["stream_build.hip"], "the compact table's span"), 16)
        _one(r"if \(\(n\[u\]\.x >= 0 && o0 >= limit\) \|\| \(n\[u\]\.y >= 0 && o1 >= limit\)\) kd\.tbl_bad\[0\] = 1;", src["stream_build.hip"], "the span check")
        bs = src["build_small.hip"]
        c["kBT"] = int(_one(r"constexpr int kBT = (\d+);", bs, "kBT"))
        dmax, mult = _one(r"if \(kds\[k\]\.d != kds\[0\]\.d \|\| kds\[k\]\.d > (\d+) \|\| \(long\)\(\(NA \+ 3\) & ~3\) \* kds\[k\]\.D1 > (\d+) \* kBT \|\|", bs,
                          "the one-workgroup build's range")
        c["small_max_d"], c["small_max_entries"] = int(dmax), int(mult) * c["kBT"]
        c["perm_min"] = sp.constants()["kPermMinPointsDefault"]
        _constants = c
    return _constants


def route_counts(D1, j0, F, maxV, table, first, compact, no_pair_fuse=False):
    """The rule, in closed form.  table: the two-hop table exists, holds the lattices in HBM and is not switched off; first: the pass its
    first pair starts at; compact: the same for the compact table.  -> the dict lccrf_batch_get_blur_plan fills."""
    c = constants()
    assert c["slice_max_D1"] >= 9 and c["slice_min_D1"] == 3, "the closed form below is written for these"
    left = D1 - j0
    p = dict.fromkeys(PLAN_FIELDS, 0)
    p["in_splat"], p["first_table_pair"] = j0, -1
    pairs = not no_pair_fuse and (F <= c["kPairFuseMaxFrames"] or F * maxV <= c["kPairFuseMaxVertices"])
    if pairs:
        p["in_slice"] = int(left % 2 == 1 and D1 >= 3)
        own = left - p["in_slice"]
        # the pairs start at j0, j0 + 2 ...: all of them lie on the table's pairs (first, first + 1), (first + 2, first + 3) ... or none does
        on_table = table and j0 >= first and (j0 - first) % 2 == 0 and own >= 2
        p["paired_table" if on_table else "paired_plain"] = own - own % 2
        if on_table:
            p["first_table_pair"] = (j0 - first) // 2
        alone = own % 2                                                            # (d + 1 = 2 with pass 0 in the splat: one pass, no partner)
    else:
        p["in_slice"] = int(left > 0 and F <= c["kSliceBlurMaxFrames"])
        alone = left - p["in_slice"]
    p["alone_compact" if compact else "alone_32bit"] = alone
    p["nontemporal"] = int(p["alone_32bit"] > 0 and F >= c["kBlurNtMinFrames"])
    return p


def compact_table_holds(lat, limit):
    """k_nbr_compact's check on one frame: per axis and block of kNbrcBlock consecutive vertices, every present n1 (and every present
    n2) lies less than `limit` above the smallest one of the block"""
    B = constants()["kNbrcBlock"]
    V = lat.V
    blocks = np.arange(V) // B
    starts = np.arange(0, V, B)
    for n2 in lat.nbr:
        n1 = np.full(V, -1, np.int64)
        n1[n2[n2 >= 0]] = np.nonzero(n2 >= 0)[0]
        for n in (n1, n2):
            lo = np.minimum.reduceat(np.where(n >= 0, n, np.iinfo(np.int64).max), starts)
            if np.any((n >= 0) & (n - lo[blocks] >= limit)):
                return False
    return True


def small_build(d, n_active):
    """the one-workgroup build takes the term (below locality mode): d and the padded entries within its range, and its LDS plan fits
    (build_small.hip: small_plan -- 158 KB: far from these cases' frames, so only the first two are restated and the third is asserted)"""
    c = constants()
    live = ((n_active + 3) & ~3) * (d + 1)
    if d > c["small_max_d"] or live > c["small_max_entries"]:
        return False
    assert live <= 6144, "a frame this large may not fit the one-workgroup build's LDS: restate small_plan() before using it in a case"
    return True


def expected_plans(features, max_points, vertex_order=0, env=None):
    """features: per frame None (empty) or a list of per-term [n][d] arrays, of a BatchCRF(len(features), max_points, 2, dims, ...).
    -> per term dict(plan, state): the plan lccrf_batch_get_blur_plan must report behind build(), and what it was derived from."""
    c = constants()
    env = env or {}
    assert set(env) <= set(SWITCHES), env
    F = len(features)
    live = [fr for fr in features if fr is not None]
    n_active = max(len(fr[0]) for fr in live)
    locality = max_points >= c["perm_min"] and n_active >= c["perm_min"]
    out = []
    lats = [[sp.Lattice(fr[k]) if fr is not None else None for fr in features] for k in range(len(live[0]))]
    # (one order for the whole CRF: a frame the sorted build cannot take sends every term to the hash build)
    sorted_build = locality and vertex_order != 2 and all(l.sortable for ls in lats for l in ls if l)
    for ls in lats:
        lv = [l for l in ls if l]
        d = lv[0].d
        D1 = d + 1
        maxV = max(l.V for l in lv)
        tables = max_points >= c["perm_min"]                                       # fastn / nearoff / the pinned flags: KernelDev::tbl_bad
        streaming = locality or not small_build(d, n_active)
        nbr2 = F == 1                                                              # (Fcap = F in every case here)
        first = int(tables and sorted_build)                                       # fast0_ok as the build leaves it
        fast0 = bool(first) and "LCCRF_FAST0_BREAK" not in env
        j0 = 0
        if fast0:
            cap = int(env["LCCRF_SPLAT_PASSES"]) if "LCCRF_SPLAT_PASSES" in env else None
            j0 = sp.plan_of(ls, max_points, F, cap)["passes"]
        nbrc = tables and F >= c["kNbrcMinFrames"]
        limit = min(max(int(env.get("LCCRF_NBRC_SPAN", c["span_limit"])), 1), c["span_limit"])
        compact = (nbrc and sorted_build and c["kNbrcMinFrames"] <= F <= c["kNbrcMaxFrames"] and "LCCRF_NO_COMPACT_NBR" not in env
                   and all(compact_table_holds(l, limit) for l in lv))
        table = nbr2 and streaming and "LCCRF_NO_2HOP_TABLE" not in env
        plan = route_counts(D1, j0, F, maxV, table, first, compact, "LCCRF_NO_PAIR_FUSE" in env)
        out.append(dict(plan=plan, lattices=ls, state=dict(D1=D1, F=F, maxV=maxV, V=[l.V if l else 0 for l in ls], j0=j0, sorted_build=sorted_build,
                                              streaming=streaming, nbr2=nbr2, table=table, first=first, nbrc=nbrc, compact=compact,
                                              product=F * maxV)))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------

ITERATIONS, RELAX = 3, 0.9


class Case:
    """One row of the table.  terms: per term the sides of the box the features are uniform in (tests/splat_plan_cases.py: box);
    frames: per frame (n, seed) or None (empty); vertex_order: LCCRF_OPT_VERTEX_ORDER (2 = the hash build); env: switches of the
    instrumented library (the case then runs in a child process); routes: the routes the case is in the table for."""

    def __init__(self, name, terms, frames, routes, vertex_order=0, env=None, weights=None, classes=()):
        self.name, self.terms, self.frame_specs, self.routes = name, terms, frames, set(routes)
        self.vertex_order, self.env, self.classes = vertex_order, dict(env or {}), set(classes)
        self.weights = weights or [3.0 if i == 0 else 2.0 for i in range(len(terms))]
        self._frames = self._expected = None

    @property
    def F(self):
        return len(self.frame_specs)

    @property
    def max_points(self):
        return max(s[0] for s in self.frame_specs if s)

    @property
    def dims(self):
        return [len(t) for t in self.terms]

    def frames(self):
        """per frame: None or dict(N, L, unary, kernels=[(features, w) ...])"""
        if self._frames is None:
            self._frames = [None if not spec else
                            dict(N=spec[0], L=2, unary=sp.unary_of(*spec),
                                 kernels=[(sp.box(spec[0], t, spec[1] + 100 * k), np.float32(self.weights[k])) for k, t in enumerate(self.terms)])
                            for spec in self.frame_specs]
        return self._frames

    def expected(self):
        if self._expected is None:
            feats = [[f for f, _ in fr["kernels"]] if fr else None for fr in self.frames()]
            self._expected = expected_plans(feats, self.max_points, self.vertex_order, self.env)
        return self._expected

    def plan(self, k=0):
        return self.expected()[k]["plan"]


def _cube(side, d):
    return (float(side),) * d


HASH, SORTED = 2, 0
N0 = sp.N0
# d = 8, uniform in a cube of side 6: ~0.9 (d + 1) vertices per point and about every fourth neighbour present.  Two frames per batch,
# one with an odd and one with an even V and different N; the products F * maxV are stated in notes/blur_plan_tests.md.
BIG = _cube(6.0, 8)
CASES = [
    # ---- the hash build, one frame: the two-hop table from pass 0 on.  d + 1 = 2 .. 9; below d = 4 the frame has to be beyond the
    # one-workgroup build's range (12288 padded entries), which fills no table
    Case("hash1_D2", [(3000.0,)], [(6201, 2)], {"paired_table"}, HASH),
    Case("hash1_D3", [(70.0, 70.0)], [(4101, 3)], {"paired_table", "in_slice"}, HASH),
    Case("hash1_D4", [_cube(17.0, 3)], [(3081, 4)], {"paired_table"}, HASH),
    Case("hash1_D5", [_cube(4.5, 4)], [(301, 5)], {"paired_table", "in_slice"}, HASH),
    Case("hash1_D6", [_cube(3.5, 5)], [(302, 6)], {"paired_table"}, HASH),
    Case("hash1_D7", [_cube(3.0, 6)], [(303, 7)], {"paired_table", "in_slice"}, HASH),
    Case("hash1_D8", [_cube(2.5, 7)], [(305, 8)], {"paired_table"}, HASH),
    Case("hash1_D9", [_cube(2.5, 8)], [(306, 9)], {"paired_table", "in_slice"}, HASH),
    # ... and inside that range: the table is allocated but the one-workgroup build does not fill it
    Case("hash1_small_D3", [(20.0, 20.0)], [(301, 10)], {"paired_plain", "in_slice"}, HASH, classes={"table_not_filled"}),
    # ---- the hash build, several frames, a small launch: pairs without a table, with (d + 1 = 3) and without (d + 1 = 6) the left-over
    # pass in the slice; ragged, an empty frame, N % 4 != 0
    Case("hash4_ragged", [_cube(3.5, 5), (20.0, 20.0)], [(301, 11), None, (250, 12), (302, 13)], {"paired_plain", "in_slice"}, HASH,
         classes={"ragged"}),
    # ---- the sorted build, one frame (locality mode: from 8192 points; LCCRF_OPT_VERTEX_ORDER = 1 does not lower that)
    Case("sorted1_j1_D3", [(150.0, 87.0)], [(N0, 1)], {"in_splat", "paired_table"}, classes={"j0=1", "table_from_1"}),
    Case("sorted1_j1_D5", [(150.0, 4.0, 4.0, 5.5)], [(N0, 1)], {"in_splat", "paired_table"}, classes={"j0=1", "table_from_1"}),
    Case("sorted1_demoted_D4", [(40.0, 40.0, 80.0)], [(N0, 1)], {"in_splat", "paired_table", "in_slice"}, classes={"j0=1", "demoted"}),
    Case("sorted1_j3_D5", [(4.0, 4.0, 4.0, 3000.0)], [(N0, 7)], {"in_splat", "paired_table"}, classes={"j0=3", "first_pair_1"}),
    Case("sorted1_j3_D6", [(3.0, 3.0, 3.0, 3.0, 1500.0)], [(N0, 7)], {"in_splat", "paired_table", "in_slice"}, classes={"j0=3", "first_pair_1"}),
    Case("sorted1_j2_D3", [(60.0, 200.0)], [(N0, 1)], {"in_splat", "in_slice"}, classes={"j0=2", "no_launch"}),
    Case("sorted1_j3_D3", [(8.0, 1625.0)], [(N0, 1)], {"in_splat"}, classes={"j0=3", "no_launch", "all_in_splat"}),
    # ---- the sorted build, several frames, a small launch: no table
    Case("sorted3_j3_D5", [(4.0, 4.0, 4.0, 3000.0)], [(N0, 1), (N0 - 37, 2), (N0 - 74, 3)], {"in_splat", "paired_plain"}, classes={"j0=3"}),
    Case("sorted2_j3_D6", [(3.0, 3.0, 3.0, 3.0, 1500.0)], [(N0, 1), (N0 - 37, 2)], {"in_splat", "paired_plain", "in_slice"}, classes={"j0=3"}),
    # ---- above the vertex bound: a launch per pass
    Case("big_F2", [BIG], [(43006, 1), (43250, 2)], {"in_splat", "alone_32bit"}, classes={"above"}),
    Case("big_F3_sorted", [BIG], [(29001, 1), (29250, 2), (29001, 1)], {"in_splat", "alone_compact"}, classes={"above"}),
    Case("big_F5_sorted", [BIG], [(17501, 1), (17654, 2), (17501, 1), (17654, 2), (17501, 1)], {"in_splat", "alone_compact"}, classes={"above"}),
    Case("big_F4_hash", [BIG], [(21801, 1), (22000, 2), (21801, 1), (22000, 2)], {"alone_32bit"}, HASH, classes={"above", "compact_not_valid"}),
    Case("big_F6", [BIG], [(14601, 1), (14750, 2)] * 3, {"in_splat", "alone_32bit"}, classes={"above", "nontemporal"}),
    # ... and the F = 3 batch just below it: pairs again
    Case("below_F3_sorted", [BIG], [(27401, 1), (27550, 2), (27401, 1)], {"in_splat", "paired_plain"}, classes={"below"}),
    # ---- the instrumented library's switches (a child process each)
    Case("span_F3_sorted", [BIG], [(29001, 1), (29250, 2), (29001, 1)], {"in_splat", "alone_32bit"}, env={"LCCRF_NBRC_SPAN": "8"}, classes={"above", "abandoned"}),
    Case("nocompact_F3_sorted", [BIG], [(29001, 1), (29250, 2), (29001, 1)], {"in_splat", "alone_32bit"}, env={"LCCRF_NO_COMPACT_NBR": "1"}, classes={"above"}),
    Case("fast0_break_F3_sorted", [BIG], [(29001, 1), (29250, 2), (29001, 1)], {"alone_compact"}, env={"LCCRF_FAST0_BREAK": "1"}, classes={"above"}),
    Case("fast0_break_D5", [(4.0, 4.0, 4.0, 3000.0)], [(N0, 7)], {"paired_plain", "in_slice"}, env={"LCCRF_FAST0_BREAK": "1"}, classes={"table_never_used"}),
    Case("nopair_F1_D6", [_cube(3.5, 5)], [(302, 6)], {"alone_32bit", "in_slice"}, HASH, env={"LCCRF_NO_PAIR_FUSE": "1"}, classes={"slice_of_singles"}),
    Case("notable_F1_D6", [_cube(3.5, 5)], [(302, 6)], {"paired_plain"}, HASH, env={"LCCRF_NO_2HOP_TABLE": "1"}),
    Case("pass0_only_D2", [(27000.0,)], [(N0, 4)], {"in_splat", "alone_32bit"}, env={"LCCRF_SPLAT_PASSES": "1"}, classes={"single_in_pair_mode"}),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# what the table must hold, route by route, from the release library alone (tests/test_blur_plan_cases.py)
RELEASE_ROUTES = set(ROUTES)


# ---- the device side (tests/test_blur_plan.py; also run in a child process under a switch of the instrumented library) -----------

def batch_inputs(case):
    frames, F, maxN = case.frames(), case.F, case.max_points
    npts = [fr["N"] if fr else 0 for fr in frames]
    feats = [np.zeros((F, maxN, d), np.float32) for d in case.dims]
    unary = np.zeros((F, maxN, 2), np.float32)
    for f, fr in enumerate(frames):
        if fr:
            unary[f, :fr["N"]] = fr["unary"]
            for k in range(len(case.dims)):
                feats[k][f, :fr["N"]] = fr["kernels"][k][0]
    return npts, feats, unary


def plan_rows(b, K):
    return np.array([[b.blur_plan(k)[n] for n in PLAN_FIELDS] for k in range(K)], np.int64)


def run_batch(case):
    """A build, two inferences, a rebuild and a third inference of the case's frames on a BatchCRF of exactly the case's capacity, on the
    streaming engine.  -> dict of arrays: plan / plan_after / plan_rebuilt [K][8], splat [K] (the splat plan's passes), V [K][F], engine,
    Q0 .. Q2 and map0 .. map2."""
    pkg = importlib.import_module("lc-crf-slam_amd")
    npts, feats, unary = batch_inputs(case)
    K = len(case.dims)
    b = pkg.BatchCRF(case.F, case.max_points, 2, case.dims, [float(w) for w in case.weights])
    b.set_engine(1)
    b.set_option(pkg.OPT_VERTEX_ORDER, case.vertex_order)
    b.set_inputs_host(npts, feats, unary=unary)
    b.build()
    out = dict(plan=plan_rows(b, K), splat=np.array([b.splat_plan(k)["passes"] for k in range(K)], np.int64))
    for rep in range(3):
        if rep == 2:
            b.build()
            out["plan_rebuilt"] = plan_rows(b, K)
        b.inference(ITERATIONS, True, RELAX)
        out["Q%d" % rep], out["map%d" % rep] = b.probability().copy(), b.map().copy()
        if rep == 1:
            out["plan_after"] = plan_rows(b, K)
    out["V"] = np.array([b.lattice_sizes(k) for k in range(K)], np.int64)
    out["engine"] = np.int64(b.engine())
    b.close()
    return out


_oracle = {}


def oracle_frame(po, case, f):
    """(V per term, Q, map) of frame f after ITERATIONS at RELAX: computed once per distinct frame of the session and left unchanged"""
    key = (tuple(case.terms), tuple(case.weights), case.frame_specs[f])
    if key not in _oracle:
        cc = importlib.import_module("crf_cases")
        fr = case.frames()[f]
        o = cc.setup(po.OracleCRF, fr)
        o.inference_native(ITERATIONS, True, RELAX)
        _oracle[key] = ([o.kernel(k)["V"] for k in range(len(fr["kernels"]))], o.probability().copy(), o.map().copy())
        o.close()
    return _oracle[key]


_oracle_V = {}


def oracle_lattice_sizes(po, case, f):
    """V per term of frame f from the oracle's lattices alone (no inference), once per distinct frame"""
    key = (tuple(case.terms), case.frame_specs[f])
    if key not in _oracle_V:
        cc = importlib.import_module("crf_cases")
        fr = case.frames()[f]
        o = cc.setup(po.OracleCRF, fr)
        _oracle_V[key] = [o.kernel(k)["V"] for k in range(len(fr["kernels"]))]
        o.close()
    return _oracle_V[key]


if __name__ == "__main__":                      # child process: python blur_plan_cases.py <case> <out.npz>
    sys.path[:0] = [ROOT]
    np.savez(sys.argv[2], **run_batch(BY_NAME[sys.argv[1]]))

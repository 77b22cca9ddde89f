"""Frames whose appearance lattice is shaped for the chain rows -- the ordered row sums of the long rows of kernel 0 -- and the case table of
the 1024-lane loop's tests (tests/test_chain_rows.py; csrc/fused_loop.h: chain_wanted, layout_core, pst, chain_setup, chain_pads,
chain_rows, phase S of splat_blur).  tests/test_chain_lanes.py takes its frames from the same generator.

A frame's appearance features are built on the CPU: clusters of identical points -- a cluster of n points is three rows of n products --
and isolated points, cell after cell, that step the vertex count.  The vertex count V0 and the row lengths are always READ from the CPU
checker's lattice of the finished frame, never assumed: every claim a case makes is asserted from them before anything runs on a GPU."""
from collections import namedtuple

import numpy as np

TOP, MIN_ROW = 16, 64                                         # csrc/fused_loop.h: kChainTop, kChainMinRow
MAX_V = {1024: 464, 512: 208}                                 # chain_max_v(lanes)


def lattice(po, feat):
    """(vertex count, row lengths) of the checker's lattice of one kernel's features"""
    n = feat.shape[0]
    o = po.OracleCRF(n, 2)
    o.set_unary_from_label(np.zeros(n, np.int16), np.float32(0.7))
    o.add_pairwise(feat, 1.0)
    k = o.kernel(0)
    o.close()
    return k["V"], np.bincount(k["offset"].reshape(-1), minlength=k["V"])


def cell(c):
    """a lattice cell far from every other one (crf_cases.shaped_problem's `sparse` placement); cell(0) is the origin's, where the
    phantom points of N % 4 != 0 fall"""
    return np.array([c, (c * 7) % 1013], np.float32) * np.float32(9.0)


NEAR = np.float32([[0, 0], [0.3, 0], [0.6, 0.2], [0.9, 0], [1.2, 0.4], [0.3, 0.6], [0.6, 0.9], [0, 0.9]])
FIRST_ISOLATED = 400                                          # isolated points sit in cell(400), cell(401), ...
_BRINGS = {}


def _brings(po):
    """vertices a cell of isolated points brings -> the fewest of its points (the first k of NEAR) that do; measured beside four
    points at the origin, so that no count is off by the phantom points' vertices"""
    if not _BRINGS:
        base = np.stack([cell(0)] * 4)
        V = lattice(po, base)[0]
        for k in range(1, len(NEAR) + 1):
            _BRINGS.setdefault(lattice(po, np.concatenate([base, cell(FIRST_ISOLATED) + NEAR[:k]]))[0] - V, k)
    return _BRINGS


def shaped_frame(po, wl, clusters, v_target, seed, first_cell=0, n_mod4=None, max_isolated=80):
    """A frame whose appearance lattice has exactly `v_target` vertices (None: what the clusters bring): `clusters` of identical points,
    their points shuffled among each other, then isolated points: cell after cell, the first k of eight points a little apart (NEAR)
    -- the first brings its cell's vertices, the others share some of them, so a cell can bring 3, 4, 5 ... vertices: how many for
    which k is read from the checker, and the cells' counts are chosen to add up with the fewest points, at most `max_isolated`.

    clusters: point counts; an entry (n, m) is two clusters in ONE cell, n points at NEAR[0] and m at NEAR[1], which share some of their
    vertices (rows of n + m, n and m products).  Cluster i sits in cell(first_cell + i): with first_cell = 1 nothing real is in the
    origin's cell, and the phantom points of N % 4 != 0 bring three vertices whose rows are EMPTY.
    n_mod4: N % 4 of the finished frame, reached by repeating the first isolated point (the last point, if there is none) up to three
    times; it must be given with first_cell > 0, where it decides the vertex count.
    The smoothness features, labels and confidence are a SLAM frame's.  Returns (problem, V0, row lengths, longest first)."""
    rng = np.random.default_rng(seed)
    spots, sizes = [], []                                     # (cell, offset inside it) and point count of every cluster
    for i, c in enumerate(clusters):
        for n, off in zip(c, NEAR) if isinstance(c, tuple) else ((c, NEAR[0]),):
            spots.append(cell(first_cell + i) + off)
            sizes.append(n)
    assert first_cell + len(clusters) <= FIRST_ISOLATED and (first_cell == 0 or n_mod4 is not None)
    own = rng.permutation(np.repeat(np.arange(len(spots)), sizes))
    f0 = np.stack(spots)[own]
    # the clusters' vertices, counted without phantom points: repeated points add none
    V = lattice(po, np.concatenate([f0] + [f0[:1]] * (-len(f0) % 4)))[0]
    phantom = 3 if first_cell > 0 and n_mod4 else 0
    want = 0 if v_target is None else v_target - V - phantom
    brings = _brings(po)
    best = {0: []}                                            # vertices still wanted -> the cells' point counts (fewest points)
    for w in range(1, want + 1):
        ways = [best[w - d] + [k] for d, k in brings.items() if d > 0 and w - d in best]
        if ways:
            best[w] = min(ways, key=sum)
    assert want in best and sum(best[want]) <= max_isolated, (clusters, V, v_target, brings)
    f0 = np.concatenate([f0] + [cell(FIRST_ISOLATED + i) + NEAR[:k] for i, k in enumerate(best[want])])
    if n_mod4 is not None:
        at = len(own) if best[want] else len(f0) - 1
        f0 = np.concatenate([f0] + [f0[at:at + 1]] * ((n_mod4 - len(f0)) % 4))
        assert len(f0) % 4 == n_mod4
    V, rows = lattice(po, f0)
    assert v_target is None or V == v_target, (clusters, V, v_target)
    pb = wl.slam_problem(len(f0), seed=seed)
    pb["kernels"] = [(np.ascontiguousarray(f0, np.float32), pb["kernels"][0][1]), pb["kernels"][1]]
    return pb, V, np.sort(rows)[::-1]


def descending(n, total):
    """n cluster sizes, all different, that add up to at most `total`"""
    base = total // n
    return [base - 3 * i for i in range(n)]


# ---- the case table of the 1024-lane loop --------------------------------------------------------------------------------------
# A shape is (lanes per workgroup, points per lane).  The cluster budget is the smallest that puts a frame into its points-per-lane
# class with room for the isolated points (at most 160: 155 one-point cells reach 464 vertices from nothing).
SHAPES = [(1024, 1), (1024, 2), (1024, 3), (1024, 4), (512, 1)]
BUDGET = {(1024, 1): 200, (1024, 2): 1030, (1024, 3): 2055, (1024, 4): 3080, (512, 1): 200}
MAX_N = {(1024, 1): 1024, (1024, 2): 2048, (1024, 3): 2300, (1024, 4): 3300, (512, 1): 512}
RING = (1, 3, 4, 5, 7, 8, 9, 12, 13, 28, 31, 32, 33, 36, 60, 63, 64, 65, 68, 95, 96, 97, 100, 127, 128, 129)
RING_MORE = (2, 6, 30, 66)                                    # two pad slots, which no length of RING has: 4n + 2
TRIPS = (95, 96, 97, 127, 128, 129)                           # the frame's longest row around a ring trip of 32 products
ISOLATED = 160

Case = namedtuple("Case", "name pb V0 rows by_vertex V1")     # rows: longest first; by_vertex: in vertex order; V1: the other lattice


def v0_edges(lanes):
    return [3, 12] + [TOP + 64 * j + d for j in range(MAX_V[lanes] // 64 + 1) for d in (-1, 0, 1) if TOP + 64 * j + d <= MAX_V[lanes]]


def top_heavy(n, total):
    """n clusters that add up to `total`: one long one, the others short and all different"""
    rest = [20 - 3 * i for i in range(n - 1)]
    return [total - sum(rest)] + rest


def fill_below(total, fixed, cap):
    """`fixed` and then clusters of at most `cap` points until `total` points are reached (nothing where `fixed` has them already)"""
    out, i = list(fixed), 0
    left = total - sum(sum(c) if isinstance(c, tuple) else c for c in fixed)
    while left > 0:
        out.append(min(cap - i % 3, left))
        left -= out[-1]
        i += 1
    return out


def ring_groups(budget):
    """RING and RING_MORE in ascending order, cut into groups of at most `budget` points"""
    groups = [[]]
    for n in sorted(RING + RING_MORE):
        if sum(groups[-1]) + n > budget:
            groups.append([])
        groups[-1].append(n)
    return groups


def case_specs(shape):
    """name -> the arguments of shaped_frame (clusters, v_target, further keywords) of every case of one shape"""
    lanes, ppt = shape
    T = BUDGET[shape]
    small = T == 200                                          # one point per lane: frames of a few hundred points
    specs = {}
    first = {1: 0, 2: 1025, 3: 2049, 4: 3073}[ppt]             # the class's smallest frame

    def room(v):                                              # the isolated points take (v - 15) / 3 of it at least: a vertex each three
        return T if small else max(first - (v - 15) // 3, first - ISOLATED)
    for v in v0_edges(lanes):                                 # a longest row of at least 64 products in every one of them
        specs["V%d" % v] = ([room(v)] if v == 3 else top_heavy(4 if v < 18 else 5, room(v)), v, {})
    over = MAX_V[lanes] + 1                                   # one vertex more than the chain lanes take
    specs["V%d" % over] = (top_heavy(5, room(over)), over, {})
    for L in (63, 64, 65):                                    # the longest row on the threshold, V0 well inside the limit
        specs["row%d" % L] = (fill_below(T, [L], L - 1), None, {})
    for i, g in enumerate(ring_groups(500 if small else 4096)):
        if max(g) < MIN_ROW:
            g = g + [MIN_ROW + 6]
        specs["ring%d" % i] = (fill_below(T, g, 24), None, {})
    for L in TRIPS:
        specs["trip%d" % L] = (fill_below(T, [L, L - 2, L - 5] if lanes == 512 else [L, L - 1, L - 2, L - 3, L - 5, L - 7], L - 8), None, {})
    for L in (31, 32, 33):                                    # ranks 16 and 17 -- the second wavefront pair's longest rows
        specs["wave1_%d" % L] = (fill_below(T, [70, 69, 68, 67, 66, L], 24), 30 if small else None, {})
    if ppt >= 2:                                              # rows on the last bucket's boundary of the counting sort
        specs["buckets"] = (fill_below(T, [1005, 1004], 600), None, {})
    specs["tie"] = (fill_below(T, [69, 68, 67, 66, 65, 64], 40), 40 if small else None, {})           # ranks 15, 16, 17: one cluster
    specs["no_tie"] = (fill_below(T, [(70, 66), 74, 73, 72, 71, 50], 40), 40 if small else None, {})  # ranks 15 and 16 differ
    for r in (0, 1, 2, 3):                                    # rows of no products at all among the chain rows (none when N % 4 = 0)
        specs["empty%d" % r] = (top_heavy(5, T), 40, dict(first_cell=1, n_mod4=r))
    return specs


_CASES = {}


def cases(po, wl, shape):
    """name -> Case of one shape, built once per process"""
    if shape not in _CASES:
        out = {}
        for i, (name, (clusters, v, kw)) in enumerate(case_specs(shape).items()):
            pb, V0, rows = shaped_frame(po, wl, clusters, v, 7000 + 100 * SHAPES.index(shape) + i, max_isolated=ISOLATED, **kw)
            out[name] = Case(name, pb, V0, rows, lattice(po, pb["kernels"][0][0])[1], lattice(po, pb["kernels"][1][0])[0])
        _CASES[shape] = out
    return _CASES[shape]


def chain(c, lanes=1024):
    """csrc/fused_loop.h:95-98 chain_wanted for one frame on its own (the third condition cannot fail below 4096 points and 464 vertices)"""
    return int(c.rows[0]) >= MIN_ROW and c.V0 <= MAX_V[lanes]


# Frames of 3073 points and more: beyond this many appearance vertices the chain plane (14 slots per vertex and label beside the products)
# and the smoothness lattice's tables no longer fit the 160 KiB of LDS, and the fused engine leaves the frame to the streaming engine
# (tests/test_chain_rows.py: test_plans_of_every_frame_and_batch holds layout_core to both sides of it)
FITS_MAX_V = {4: 337}


def groups(table, lanes, ppt=1):
    """name -> (case names, the chain decision of a batch of them): the batches whose batch-wide decision is the intended one"""
    top = MAX_V[lanes]
    inside = [n for n, c in table.items() if c.V0 <= top and not n.startswith("row")]
    fits = [n for n in inside if table[n].V0 <= FITS_MAX_V.get(ppt, top)]
    out = {"edges": (fits, True),                              # the largest V0 that fits, a row >= 64: every V0 edge rides the chain
           "over": (["V%d" % (top + 1), "V%d" % top, "V16", "tie"], False),           # one frame one vertex over: nobody does
           "row63": (["row63", "row63"], False),
           "row64": (["row64", "row63"], True)}
    if len(fits) < len(inside):
        out["beyond"] = ([n for n in inside if n not in fits], True)                  # (what the fused plan has no room for)
    return out

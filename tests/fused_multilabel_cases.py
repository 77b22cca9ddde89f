"""What tests/test_fused_multilabel.py and tests/perf/fused_multilabel.py share: the problems of the fused engine's kernel for three to
eight labels (csrc/fused_multilabel.hip, LCCRF_OPT_FUSED_MULTILABEL), the case list with the instantiation class each case is there
for, and the class a frame's lattices put it in (csrc/fused_loop.h: layout_core)."""
import numpy as np

import crf_cases as cc

LANES = 1024
# the shipped range, as the header of csrc/fused_multilabel.hip states it: label count -> largest frame (active points)
PLAN = {3: 2048, 4: 2048, 5: 1024, 6: 1024, 7: 1024, 8: 1024}
TERMS = {"": [0, 1], "appearance": [0], "smooth": [1], "smooth_first": [1, 0]}


def problem(wl, N, L, unary="raw", terms="", seed=21, sparse=False):
    """The frame of workloads.slam_problem(N, seed) -- its appearance term (a hundred-odd vertices, rows of hundreds of products from
    ~1000 points on: chain rows) and its smooth term (about one vertex per two points: short rows), in the order `terms` names -- with
    L labels: raw unaries 1.5 N(0, 1) seeded by [seed, N, L], or label-derived ones, labels uniform in [-1, L) (-1: unknown) with a
    confidence per label in [0.55, 0.9].  sparse: crf_cases.shaped_problem(wl, N, "sparse", seed), every point of the first term in a
    lattice cell of its own."""
    base = cc.shaped_problem(wl, N, "sparse", seed) if sparse else wl.slam_problem(N, seed=seed)
    pb = dict(N=N, L=L, kernels=[base["kernels"][k] for k in TERMS[terms]])
    rng = np.random.default_rng([seed, N, L])
    if unary == "raw":
        pb["unary"] = (rng.standard_normal((N, L)) * 1.5).astype(np.float32)
    else:
        pb["label"] = rng.integers(-1, L, N).astype(np.int16)
        pb["conf"] = rng.uniform(0.55, 0.9, L).astype(np.float32)
    return pb


# name -> (arguments of problem(), (points per lane, kernel 0 on chain rows, a product buffer per term))
CASES = {
    # sizes at L = 3 and L = 4: phantom vertices and idle lanes; the last frame taken
    "L3/N5": (dict(N=5, L=3, unary="label"), (1, 0, 1)),
    "L4/N5": (dict(N=5, L=4), (1, 0, 1)),
    "L3/N7": (dict(N=7, L=3), (1, 0, 1)),
    "L4/N7": (dict(N=7, L=4, unary="label"), (1, 0, 1)),
    "L3/N2048": (dict(N=2048, L=3), (2, 1, 1)),
    "L4/N2048": (dict(N=2048, L=4, unary="label"), (2, 1, 1)),
    # lattices so large that both terms' products share ONE buffer in LDS
    "L3/sparse:N1100": (dict(N=1100, L=3, sparse=True, seed=5), (2, 0, 0)),
    # 1024 points: every lane has its point
    "L8/N1024/smooth": (dict(N=1024, L=8, terms="smooth"), (1, 0, 1)),
}
# ... and EVERY instantiation of the kernel on a frame that fills most lanes (a kernel that the compiler got wrong -- see `pad` in
# csrc/fused_multilabel.hip -- passed on the 5- and 7-point frames): label count x points per lane (N = 1001: one; N = 1025: lane 0
# alone has a second point) x the terms (both: K = 2, chain rows; smooth first: K = 2, short rows; each on its own: K = 1), raw and
# label-derived unaries taking turns
for _i, (_L, _N, _t) in enumerate((L, N, t) for L in sorted(PLAN) for N in (1001, 1025) if N <= PLAN[L]
                                  for t in ("", "smooth_first", "appearance", "smooth")):
    CASES["L%d/N%d%s" % (_L, _N, "/" + _t if _t else "")] = (
        dict(N=_N, L=_L, terms=_t, unary="label" if _i % 2 else "raw"),
        ((_N + LANES - 1) // LANES, int(_t in ("", "appearance")), 1))
# the case of the schedule tests
SCHEDULE_CASE = "L4/N1025"


def own_product_buffers(N, V, chain0):
    """csrc/fused_loop.h: layout_core -- does the plan with a product buffer per term fit the 160 KiB of LDS?  (bytes, 16-aligned)"""
    a16 = lambda b: (b + 15) & ~15
    total = 128 + 64
    for k, v in enumerate(V):
        floats = (N * 3 + (14 * v + 16 if k == 0 and chain0 else 0) + 63) & ~63
        total += 2 * a16((v + 1) * 8) + a16(3 * v * 4) + a16((v + 2) * 2) + a16(floats * 8)
    return total <= 160 * 1024


def instantiation_class(N, lattices):
    """(points per lane, kernel 0 on chain rows, a product buffer per term) of a frame of N points whose terms' lattices are
    `lattices` (OracleCRF.kernel(k) of each): csrc/fused_loop.h -- a lane owns ceil(N / 1024) points; kernel 0 takes chain rows when
    its longest splat row has at least 64 products and it has at most 464 vertices (chain_wanted; the u16 slot bound holds for every
    frame of this size)."""
    V = [k["V"] for k in lattices]
    row0 = int(np.bincount(lattices[0]["offset"].reshape(-1), minlength=V[0]).max())
    chain0 = int(row0 >= 64 and V[0] <= 464)
    return (N + LANES - 1) // LANES, chain0, int(own_product_buffers(N, V, chain0))


_PREPARED = {}


def prepared(name, po, wl):
    """(problem, its instantiation class from the oracle's lattices): computed once, shared by the tests, never changed"""
    if name not in _PREPARED:
        pb = problem(wl, **CASES[name][0])
        o = cc.setup(po.OracleCRF, pb)
        cls = instantiation_class(pb["N"], [o.kernel(k) for k in range(len(pb["kernels"]))])
        o.close()
        _PREPARED[name] = (pb, cls)
    return _PREPARED[name]


_EXPECTED = {}


def expected(name, po, wl, T, relax):
    """(Q, labels) of the oracle after T iterations: computed once per (case, T, relax)"""
    key = (name, T, relax)
    if key not in _EXPECTED:
        o = cc.setup(po.OracleCRF, prepared(name, po, wl)[0])
        o.inference_native(T, True, relax)
        _EXPECTED[key] = (o.probability(), o.map())
        o.close()
    return _EXPECTED[key]


def shape_word(word):
    """lccrf_get_engine's shape word -> (lanes, points per lane, kernel 0 on chain rows)"""
    return word & 0xffff, (word >> 16) & 15, (word >> 20) & 1

"""Deterministic frames for the table-free lattice build of the half-CU frame kernel (csrc/frame_build.h: grid_records / grid_build,
launched by csrc/frame_lean.hip), one kind per edge of its arithmetic -- the seeded twins of scripts/stress_frame_lean.py's clouds.

A problem is a wl.slam_problem(N, seed) with one or both feature arrays replaced (kernel 0: appearance, kernel 1: smoothness).
The d = 2 lattice in the build's coordinates: a key (x, y) has x = y (mod 3); u = (x - y) / 3, v = y.  A feature (f0, f1) is elevated
to (sqrt(3) f0 + f1, f1 - sqrt(3) f0, -2 f1) (permutohedral_cpu.h:249,282-285), so the remainder-0 vertex (u, v), v a multiple of 3,
is the image of f0 = sqrt(3) u / 2, f1 = (3 u + 2 v) / 2: `at_cell` below puts a point a little inside the simplex beside it.

expected_route(pb, po) classifies a problem from the ORACLE's lattice alone (never from the library): 'fit', 'flag' or 'plan'.
compare_batch() is what the GPU tests compare with; tests/test_frame_lean_cases.py shows that it rejects planted faults.
"""
import numpy as np

SQ3 = np.sqrt(3.0)

# the kernel's closed exits (csrc/frame_build.h, csrc/frame_lean.hip, csrc/fused_lean.h), restated
MAX_CELLS = 32768            # kGridMaxCells
MAX_V = 1344                 # lean_max_v(512) = 3 * (512 - 64)
MAX_V0 = 208                 # chain_max_v(512)
GUARD = 32000                # |rem0| of any point record, point_record2_grid
LDS = 80 * 1024              # half a CU
TOPS = (512, 1024, 1536, 2048)          # the batch's largest frame for 1, 2, 3, 4 points per lane
# scales of the SLAM features of kernel 0 / kernel 1 at N = 2048: (V0, V1) = (176, 1165), (195, 1165), (124, 1314), (124, 1333)
# (du, dv) of the two clusters:       Wp x Hp = cells
CELL_KINDS = {"cells_max": (177, 171),        # 182 x 180 = 32760: within one row of the id map's 32768 cells
              "cells_over": (178, 171),       # 183 x 180 = 32940
              "cells_max0": (177, 171), "cells_over0": (178, 171),      # the same two on kernel 0
              "cells_top": (122, 249),        # 127 x 258 = 32766
              "cells_tall": (0, 6543),        # 5 x 6552 = 32760: one column of u
              "cells_tall_over": (0, 6546),   # 5 x 6555 = 32775
              "cells_flat": (3635, 0),        # 3640 x 9 = 32760: one row of v
              "cells_flat_over": (3636, 0)}   # 3641 x 9 = 32769
PLAN_KINDS = {"plan_v0_in": (1.3, 1.0), "plan_v0_out": (1.4, 1.0), "plan_v1_in": (1.0, 1.07), "plan_v1_edge": (1.0, 1.08)}


def at_cell(u, v, off=(0.11, 0.23)):
    """features of points whose remainder-0 vertex is (u, v) (v: multiples of 3), `off` inside the simplex beside it"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return np.stack([SQ3 * u / 2 + off[0], (3 * u + 2 * v) / 2 + off[1]], -1).astype(np.float32)


def _with(pb, f0=None, f1=None):
    k = pb["kernels"]
    out = dict(pb)
    out["kernels"] = [(np.ascontiguousarray(f0, np.float32) if f0 is not None else k[0][0], k[0][1]),
                      (np.ascontiguousarray(f1, np.float32) if f1 is not None else k[1][0], k[1][1])]
    return out


def _two_clusters(n, du, dv, rng):
    """n points, half beside the cell (0, 3), half beside (du, 3 + dv), each cluster inside one simplex"""
    far = np.arange(n) % 2 == 1
    f = at_cell(np.where(far, du, 0), np.where(far, 3 + dv, 3))
    return f + rng.uniform(0, 0.02, f.shape).astype(np.float32)


def _isolated(n_cells, rng=None, reps=None):
    """points beside the cells of a 21-column grid spaced (3, 6): no two cells' simplices share a vertex.  reps[i] points in cell i."""
    idx = np.arange(n_cells)
    reps = np.ones(n_cells, np.int64) if reps is None else np.asarray(reps)
    idx = np.repeat(idx, reps)
    f = at_cell(3 * (idx % 21) - 30, 6 * (idx // 21) - 60)
    if rng is not None:
        f = f + rng.uniform(0, 0.02, f.shape).astype(np.float32)
    return f


def make(wl, kind, N, seed=0):
    """one problem of a kind; N is the wanted point count where the kind leaves it free"""
    rng = np.random.default_rng([abs(hash_name(kind)), int(N), int(seed)])
    pb = wl.slam_problem(N, seed=7000 + seed + N)
    f0, f1 = pb["kernels"][0][0], pb["kernels"][1][0]
    if kind == "slam":
        return pb
    if kind == "negative":                        # u < 0 and v < 0 on every point of kernel 1
        return _with(pb, f1=np.stack([f1[:, 0] - 40.0, f1[:, 1] - 120.0], 1))
    if kind == "straddle":                        # kernel 1's box has both signs of u and of v
        return _with(pb, f1=np.stack([f1[:, 0] - 17.0, f1[:, 1] - 28.0], 1))
    if kind == "negative0":
        return _with(pb, f0=np.stack([f0[:, 0] - 12.0, f0[:, 1] - 40.0], 1))
    if kind == "straddle0":
        return _with(pb, f0=np.stack([f0[:, 0] - 2.5, f0[:, 1] - 6.0], 1))
    if kind in ("far_near", "far_far"):           # a 20 x 20 cloud away from the origin
        off = 60.0 if kind == "far_near" else 230.0
        return _with(pb, f1=rng.uniform(0, 20, (N, 2)) + off)
    if kind in CELL_KINDS:
        # two clusters at opposite corners of the box: Wp = du + 5, Hp = dv + 9 (Hp is a multiple of 3, so 32766 is the most cells a
        # frame can have).  The twin of each box is one column or one row wider.
        du, dv = CELL_KINDS[kind]
        f = _two_clusters(N, du, dv, rng)
        return _with(pb, f0=f) if kind.endswith("0") else _with(pb, f1=f)
    if kind in ("v_max", "v_over", "v_over_by_1"):
        if kind == "v_max":
            f = _isolated(448)                    # 448 points, 3 vertices each: V = 1344
        elif kind == "v_over":
            f = _isolated(452)                    # V = 1356
        else:                                     # 452 points (no phantoms): 448 cells, three repeats, one point in the simplex across an edge: V = 1345
            f = np.concatenate([_isolated(448), _isolated(3), at_cell([-30], [-60], off=(0.35, -0.15))])
        return _with(wl.slam_problem(len(f), seed=7100), f1=f)
    if kind == "bitmap1_line":                    # a thin diagonal line: few vertices, many cells
        t = rng.uniform(-40, 40, N) * (N / 2048.0)           # (about 11 points per unit of length at every size: E >= 16 V)
        return _with(pb, f1=np.stack([t, 0.5 * t + rng.normal(0, 0.01, N)], 1))
    if kind == "bitmap1_cell":                    # every point of kernel 1 in one simplex: V = 3
        return _with(pb, f1=at_cell(np.full(N, -7), np.full(N, 9)) + rng.uniform(0, 0.02, (N, 2)).astype(np.float32))
    if kind == "list0":                           # kernel 0: one simplex of 70 points among 40 isolated ones -- E < 16 V, rows of 70
        f = _isolated(41, rng, reps=[70] + [1] * 40)
        return _with(wl.slam_problem(len(f), seed=7200), f0=f)
    if kind == "ties":                            # multiples of 0.5 and exact zeros: rank ties (Q3), round-half-even (Q2)
        f = rng.integers(-24, 24, (N, 2)).astype(np.float64) * 0.5
        f[rng.random(N) < 0.05] = 0.0
        return _with(pb, f1=f)
    if kind == "ties0":
        f = rng.integers(-5, 6, (N, 2)).astype(np.float64) * 0.5
        f[rng.random(N) < 0.05] = 0.0
        return _with(pb, f0=f)
    if kind == "rows8":                           # kernel 1's rows of 7 / 8 / 9 and 15 / 16 / 17 entries
        pat = [7, 8, 9, 15, 16, 17]
        reps = []
        while sum(reps) < N:
            reps.append(min(pat[len(reps) % 6], N - sum(reps)))
        return _with(pb, f1=_isolated(len(reps), rng, reps=reps))
    if kind in ("guard_in", "guard_in_neg", "guard_in_u", "guard_out", "guard_out_neg", "guard_out_u"):
        c = rng.uniform(0, 6, (N, 2))
        edge = 31985.0 if "_in" in kind else 32060.0          # the largest |rem0|: 31998 is the last multiple of 3 inside the guard
        if kind.endswith("_u"):                   # x = -y near the guard: the largest |u| the packed word has to carry
            c = np.stack([c[:, 0] + (edge - 18.0) / SQ3, c[:, 1]], 1)
        else:
            c = np.stack([c[:, 0], c[:, 1] + edge - 18.0], 1)
            if kind.endswith("_neg"):
                c = -c
        return _with(pb, f1=c)
    if kind in PLAN_KINDS:                        # full-size frames whose lattices bring the loop's LDS plan to its limit
        s0, s1 = PLAN_KINDS[kind]
        return _with(pb, f0=f0 * np.float32(s0), f1=f1 * np.float32(s1))
    if kind == "k0_wide":                        # kernel 0 on the smoothness features: V in the hundreds
        return _with(pb, f0=f1)
    if kind == "k0_short":                        # kernel 0 spread out: no row of 64 products
        return _with(pb, f0=f0 * np.float32(1.25))
    raise ValueError(kind)


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def cases(wl, top=2048):
    """[(name, problem)] of a batch whose largest frame has `top` points (TOPS: one instantiation of the kernel each); the kinds
    that leave N free are generated at `top` (N % 4 == 0), the far pair also at top - 1, the others at their own sizes"""
    out = [("slam", make(wl, "slam", top))]
    for kind in ("negative", "straddle", "negative0", "straddle0", "far_near", "far_far", "cells_max", "cells_over", "cells_max0",
                 "cells_over0", "cells_top", "cells_tall", "cells_tall_over", "cells_flat", "cells_flat_over", "bitmap1_line", "bitmap1_cell", "ties", "ties0", "rows8", "guard_in", "guard_in_neg", "guard_in_u",
                 "guard_out", "guard_out_neg", "guard_out_u", "k0_wide"):
        out.append((kind, make(wl, kind, top)))
    for kind in ("far_near", "far_far", "straddle"):            # the same clouds without their last point: phantom points at the origin
        pb = make(wl, kind, top)
        n = top - 1
        q = dict(pb, N=n, label=pb["label"][:n], truth=pb["truth"][:n], kernels=[(f[:n], w) for f, w in pb["kernels"]])
        q.pop("frame", None)
        out.append((kind + "_m1", q))
    for kind in ("v_max", "v_over", "v_over_by_1", "list0"):
        out.append((kind, make(wl, kind, 0)))
    out.append(("k0_short", make(wl, "k0_short", 300)))
    for n in range(6):
        out.append(("tiny%d" % n, make(wl, "negative", n, seed=n)))
    return out


def plan_cases(wl):
    """[(name, problem)]: full-size frames (N = 2048) that no closed rule rejects and whose LDS plan is at its limit"""
    return [(kind, make(wl, kind, 2048)) for kind in sorted(PLAN_KINDS)]


# ---- the oracle's lattice in the build's terms----------------------------------------------------------------------------------
def lattice_model(pb, po, ref=None):
    """per kernel: V, the remainder-0 vertices' (u, v) per point (+ the phantom point's (0, 0) when N % 4), Wp, Hp, cells, the
    longest row, E, the largest |coordinate| of a remainder-0 key"""
    import crf_cases as cc
    n = pb["N"]
    if n == 0:
        return [dict(V=0, u=np.zeros(0, int), v=np.zeros(0, int), Wp=0, Hp=0, cells=0, rowmax=0, E=0, rem0=0, rows=np.zeros(0, int))] * 2
    o = cc.setup(po.OracleCRF, pb)
    out = []
    for k in range(len(pb["kernels"])):
        kk = o.kernel(k)
        key = kk["keys"][kk["offset"][:, 0]].astype(np.int64)
        x, y = key[:, 0], key[:, 1]
        if n % 4:
            x, y = np.append(x, 0), np.append(y, 0)
        assert ((x - y) % 3 == 0).all() and (y % 3 == 0).all()
        u, v = (x - y) // 3, y
        Wp, Hp = int(u.max() - u.min()) + 5, int(v.max() - v.min()) + 9
        rows = np.bincount(kk["offset"].ravel(), minlength=kk["V"])
        out.append(dict(V=int(kk["V"]), u=u, v=v, Wp=Wp, Hp=Hp, cells=Wp * Hp, rowmax=int(rows.max()), E=3 * n,
                        rem0=int(max(np.abs(x).max(), np.abs(y).max())), rows=rows))
    o.close()
    return out


def plan_bound(n, V0, V1):
    """an upper bound of the bytes of fused_lean.h's LDS plan for a frame: both kernels' value arrays (2 x 8 (V + 1)), kernel 0's
    neighbour table (12 V0), the row starts (2 (V + 2)) and kernel 0's again for the chain lanes, the zero block, the shared product
    buffer (two planes of 3 n + 11 * 16 + 3 V0 + 16 floats rounded up to 64), and 15 bytes of rounding for each of the ten pieces"""
    return 128 + 16 * (V0 + 1) + 16 * (V1 + 1) + 12 * V0 + 2 * (V0 + 2) + 2 * (V1 + 2) + 2 * (V0 + 2) + 8 * (3 * n + 11 * 16 + 3 * V0 + 16 + 63) + 150


def expected_route(pb, po):
    """'fit': the kernel must take the frame; 'flag': it must leave it to the fallback; 'plan': no closed rule rejects it and the LDS
    plan, which this predicate only bounds, decides.  Returns (route, reason, model)."""
    m = lattice_model(pb, po)
    if pb["N"] == 0:
        return "fit", "empty", m
    for k in range(2):
        if m[k]["rem0"] >= GUARD:
            return "flag", "kernel %d: |rem0| = %d >= %d" % (k, m[k]["rem0"], GUARD), m
    # (the kernel builds kernel 0 first and leaves at the first exit; any exit flags the frame)
    for k in range(2):
        if m[k]["cells"] > MAX_CELLS:
            return "flag", "kernel %d: %d x %d = %d cells > %d" % (k, m[k]["Wp"], m[k]["Hp"], m[k]["cells"], MAX_CELLS), m
        if m[k]["V"] > (MAX_V0 if k == 0 else MAX_V):
            return "flag", "kernel %d: V = %d > %d" % (k, m[k]["V"], MAX_V0 if k == 0 else MAX_V), m
    if plan_bound(pb["N"], m[0]["V"], m[1]["V"]) > LDS:
        return "plan", "bound of the LDS plan %d > %d" % (plan_bound(pb["N"], m[0]["V"], m[1]["V"]), LDS), m
    return "fit", "", m


# ---- references and the comparison -------------------------------------------------------------------------------------------------
def reference(pb, po, n_iter=5, relax=1.0, cls=None):
    """dict(N, Q, map, V) of one problem from the oracle (or `cls`)"""
    import crf_cases as cc
    n = pb["N"]
    if n == 0:
        return dict(N=0, Q=np.zeros((0, 2), np.float32), map=np.zeros(0, np.int16), V=[0, 0])
    o = cc.setup(cls or po.OracleCRF, pb)
    o.inference_native(n_iter, True, relax)
    r = dict(N=n, Q=o.probability().copy(), map=o.map().copy(), V=[int(o.kernel(k)["V"]) for k in range(len(pb["kernels"]))])
    o.close()
    return r


def expected_bits(ref, words):
    """the label bits of a frame as the library packs them: bit i of the row = (label of point i == 1), zeros beyond the frame"""
    want = np.zeros(words * 64, np.uint8)
    want[:ref["N"]] = ref["map"] == 1
    return np.packbits(want, bitorder="little").view(np.uint64)


def compare_batch(got, refs, which):
    """got: dict(Q [F][maxN][2] f32, map [F][maxN] i16, bits [F][words] u64, V [K][F]) of a batch; refs: list of reference();
    which[f]: the reference of frame f.  EVERY frame: Q bit for bit, then the labels, the label bits (zeros beyond the frame
    included) and both lattice sizes.  A reference may carry its own 'bits' (else expected_bits)."""
    Q, M, bits, V = got["Q"], got["map"], got["bits"], got["V"]
    assert len(which) == Q.shape[0] == M.shape[0] == bits.shape[0]
    for f, r in enumerate(which):
        ref = refs[r]
        n = ref["N"]
        assert np.array_equal(np.ascontiguousarray(Q[f, :n]).view(np.uint32), np.ascontiguousarray(ref["Q"]).view(np.uint32)), \
            "frame %d (reference %d, %d points): Q differs" % (f, r, n)
        assert np.array_equal(M[f, :n], ref["map"]), "frame %d (reference %d): labels differ" % (f, r)
        want = ref["bits"] if "bits" in ref else expected_bits(ref, bits.shape[1])
        assert np.array_equal(bits[f], want), "frame %d (reference %d): label bits differ" % (f, r)
        for k in range(len(V)):
            assert int(V[k][f]) == ref["V"][k], "frame %d (reference %d): V of kernel %d is %d, reference %d" % (f, r, k, int(V[k][f]), ref["V"][k])


def fake_batch(refs, which, maxN, words=None):
    """the `got` of a batch that equals its references (for the comparison's own tests)"""
    F = len(which)
    words = words or (maxN + 63) // 64
    got = dict(Q=np.zeros((F, maxN, 2), np.float32), map=np.zeros((F, maxN), np.int16), bits=np.zeros((F, words), np.uint64),
               V=[np.zeros(F, np.int32) for _ in range(2)])
    for f, r in enumerate(which):
        ref = refs[r]
        got["Q"][f, :ref["N"]] = ref["Q"]
        got["map"][f, :ref["N"]] = ref["map"]
        got["bits"][f] = expected_bits(ref, words)
        for k in range(2):
            got["V"][k][f] = ref["V"][k]
    return got

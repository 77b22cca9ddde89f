"""Frames placed on either side of every size rule of the streaming build in locality mode (csrc/stream_build.hip), the rules restated
in numpy, and the case table of tests/test_sorted_build.py -- notes/sorted_build_tests.md.

A case's frames are built on the CPU from a background of scattered points and clusters of IDENTICAL points (a cluster of n points is
d + 1 vertices of n entries each).  What the build must then report (lccrf_build_report) is restated here from the oracle's lattice of
the finished frame -- its vertices' keys and every entry's vertex -- and from the features: expected_report().  Nothing is assumed about
where a frame lands: tests/test_sorted_build_cases.py asserts every case's CLAIM on that restatement without a GPU, and on the device
the library's own report must equal the restatement field by field and satisfy the claim, so a case can never silently test another
branch.  The restatement knows the rules (bucket bits, the box and its guard columns, multiply-high, the thresholds); it shares no code
with the library.
"""
from collections import namedtuple

import numpy as np

import sorted_build_checker as sc

LONG_BUCKET, BITMAP_MIN, BITMAP_WORDS, ESORT_GRID = 512, 1024, 15872, 64   # kLongBucket, k_esort_long's n >= 1024, kSortBitmapWords, its grid
LONG_ROW, POINT_BUCKET, SCAN_TILE, MAX_D = 128, 64, 4096, 8                 # kLongRow, k_sort_place's 64, kScanTile, LCCRF_MAX_DIMS
PERM_MIN = 8192                                                             # locality mode from this many points (the release threshold)
FIELDS = ("sorted_build", "direct_codes", "long_buckets", "long_by_bitmap", "long_by_network_uniform", "long_by_network_mixed",
          "long_by_network_wide", "max_buckets_per_workgroup", "phantom_entries", "empty_row_vertices", "long_rows",
          "point_buckets_over_64", "largest_point_bucket")
T, RELAX = 3, 0.9                                                           # the inference every case is compared after


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------
def elevation_scale(d):
    """Engine::add_kernel's scale factors and 1 / (d + 1), in its types (permutohedral_cpu.h:249,282-285)"""
    inv_std_dev = np.float32(np.sqrt(2.0 / 3.0) * (d + 1))
    scale = np.array([np.float32(1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std_dev)) for i in range(d)], np.float32)
    return scale, np.float32(np.float32(1.0) / np.float32(d + 1))


def point_cells(feat, row_major):
    """k_sort_cells: the cell every point rounds to (float32, no fused multiply-add), in the lattice's own basis for the sorted build"""
    feat = np.asarray(feat, np.float32)
    n, d = feat.shape
    scale, inv = elevation_scale(d)
    el = np.zeros((n, d + 1), np.float32)
    sm = np.zeros(n, np.float32)
    for j in range(d, 0, -1):
        cf = feat[:, j - 1] * scale[j - 1]
        el[:, j] = sm - np.float32(j) * cf
        sm = sm + cf
    el[:, 0] = sm
    cell = np.rint(inv * el).astype(np.int64)            # (round half to even, as __float2int_rn)
    return (cell[:, d:] - cell[:, :d]) if row_major else cell[:, :d]


def point_buckets(feat, max_points, row_major):
    """k_sort_plan / k_sort_code: the bucket of the point sort every real point falls in, and the number of buckets"""
    bits = 8
    while bits < 16 and (1 << bits) < 2 * max_points:
        bits += 1
    n, d = np.asarray(feat).shape
    if n == 0:
        return np.zeros(0, np.int64), 1 << bits
    cell = point_cells(feat, row_major)
    lo, span = cell.min(0), cell.max(0) - cell.min(0) + 1
    if row_major:
        code, rng = np.zeros(n, object), 1
        for j in range(d):
            code = code + (cell[:, j] - lo[j]).astype(object) * rng
            rng *= int(span[j])
        assert rng < 1 << 64
        b = code // ((rng >> bits) + 1) if rng >> bits else code
        return np.minimum(b.astype(np.int64), (1 << bits) - 1), 1 << bits
    rem, nb = [int(s) for s in span], [0] * d             # the code bits dealt to the dimensions: the widest remaining span takes the next
    for _ in range(bits):
        best = max(range(d), key=lambda j: (rem[j], -j))
        nb[best] += 1
        rem[best] = (rem[best] + 1) >> 1
    q = [((cell[:, j] - lo[j]) << nb[j]) // int(span[j]) for j in range(d)]
    code, pos = np.zeros(n, np.int64), 0
    for level in range(bits):
        for j in range(d):
            if nb[j] > level and pos < bits:
                code |= ((q[j] >> level) & 1) << pos
                pos += 1
    return code, 1 << bits


def vertex_plan(ref, vcap):
    """k_vsort_plan on the oracle's vertices: (code of every vertex, bucket of every vertex, direct, usable)"""
    d, V = ref["d"], ref["V"]
    vbits = 10
    while vbits < 21 and (1 << vbits) < 4 * vcap:
        vbits += 1
    if V == 0:
        return np.zeros(0, object), np.zeros(0, np.int64), 2 ** d <= 1 << vbits, True
    c = sc.grid_coords(ref["keys"])
    lo, span = c.min(0), c.max(0) - c.min(0) + 2         # (one empty guard column per dimension)
    code, rng = np.zeros(V, object), 1
    for j in range(d):
        assert int(span[j]) <= (1 << 62) // rng, "the box overflows 62 bits: the library would fall back to the hash"
        code = code + (c[:, j] - lo[j]).astype(object) * rng
        rng *= int(span[j])
    if rng <= 1 << vbits:
        return code, code.astype(np.int64), True, True
    scale = (((1 << 64) - 1) // rng) << vbits
    return code, np.array([(int(x) * scale) >> 64 for x in code], np.int64), False, True


def int16_guard_holds(feat):
    """k_points<D, true>: no point may come near the int16 range of the keys (else the frame goes to the hash build)"""
    feat = np.asarray(feat, np.float64)
    if feat.size == 0:
        return True
    scale, _ = elevation_scale(feat.shape[1])
    return float(((2.0 + np.abs(feat * scale).sum(1)) * (feat.shape[1] + 1)).max()) < 31000.0


def expected_report(ref, feat, max_points, vcap, sorted_build):
    """What lccrf_batch_get_build_report must say for one frame: ref = sorted_build_checker.reference_tables of its lattice."""
    N, d, V = ref["N"], ref["d"], ref["V"]
    D1, Np = d + 1, ref["offset"].shape[0]
    r = dict.fromkeys(FIELDS, 0)
    pb, _ = point_buckets(feat, max_points, sorted_build)
    sizes = np.bincount(pb) if pb.size else np.zeros(1, np.int64)
    r["point_buckets_over_64"], r["largest_point_bucket"] = int((sizes > POINT_BUCKET).sum()), int(sizes.max())
    real = np.bincount(ref["offset"][:N].reshape(-1), minlength=V)
    if not sorted_build:
        r["long_rows"] = int((real > LONG_ROW).sum())
        return r
    code, bucket, direct, _ = vertex_plan(ref, vcap)
    r["sorted_build"], r["direct_codes"] = 1, int(direct)
    r["phantom_entries"], r["empty_row_vertices"] = (Np - N) * D1, int((real == 0).sum())
    ev = ref["offset"].reshape(-1)                        # vertex of every entry, the phantom points' included; entry id = point * (d+1) + remainder
    eb = bucket[ev] if V else np.zeros(0, np.int64)
    order = np.argsort(eb, kind="stable")
    ub, start, count = np.unique(eb[order], return_index=True, return_counts=True)
    for b, s, n in zip(ub, start, count):
        if n <= LONG_BUCKET:
            continue
        ids = order[s:s + n]
        r["long_buckets"] += 1
        words = (int(ids.max()) - int(ids.min())) // 32 + 1
        mixed = np.unique(ev[ids]).size > 1
        r["long_by_network_mixed" if mixed else "long_by_network_uniform" if n < BITMAP_MIN else
          "long_by_bitmap" if words <= BITMAP_WORDS else "long_by_network_wide"] += 1
    r["max_buckets_per_workgroup"] = -(-r["long_buckets"] // ESORT_GRID)
    return r


def bucket_entries(ref, vcap):
    """entries per bucket of the entry sort, the phantom points' included, largest first"""
    if ref["V"] == 0:
        return np.zeros(0, np.int64)
    return np.sort(np.bincount(vertex_plan(ref, vcap)[1][ref["offset"].reshape(-1)]))[::-1]


def first_vertex_is_phantoms_alone(ref, last=False):
    """position 0 of the sorted order belongs to a run of phantom entries: the vertex of the smallest (last: largest) code has no real entry"""
    first = sc.row_major_order(ref)[-1 if last else 0]
    return ref["V"] > 0 and not np.any(ref["offset"][:ref["N"]] == first)


def bitmap_words(ref, n_min=BITMAP_MIN):
    """words the LDS bitmap spans for every uniform vertex of at least n_min entries (one word per lane up to 256)"""
    ev = ref["offset"].reshape(-1)
    out = []
    for v in np.flatnonzero(np.bincount(ev, minlength=ref["V"]) >= n_min):
        ids = np.flatnonzero(ev == v)
        out.append((int(ids.max()) - int(ids.min())) // 32 + 1)
    return out


# ---- the frames -----------------------------------------------------------------------------------------------------------------------
def frame(seed, N, d, clusters=(), box=(6.0, 22.0), where=None, origin=0, sign=None):
    """N points of d features: `origin` points at feature 0, clusters of identical points -- (size, place) with the place a feature
    vector, or a number for a spot of its own left of the box along the first feature -- and a background of points scattered over
    the box (mirrored along the features whose `sign` is -1).  where: "head" puts the clusters' points first, "spread" through the frame by index (default: shuffled)."""
    rng = np.random.default_rng(seed)
    f = (rng.random((N, d)) * (box[1] - box[0]) + box[0]).astype(np.float32)
    if sign is not None:
        f *= np.float32(sign)
    idx = np.arange(N) if where == "head" else rng.permutation(N)
    n_cl = sum(c[0] for c in clusters)
    if where == "spread":
        idx = np.concatenate([np.arange(0, N, N // n_cl)[:n_cl], np.setdiff1d(np.arange(N), np.arange(0, N, N // n_cl)[:n_cl])])
    at = 0
    for size, place in clusters:
        spot = np.full(d, box[0] + 2.0, np.float32)
        if np.ndim(place) == 0:
            spot[0] = np.float32(box[0] - 4.0 - 3.0 * place)
        else:
            spot = np.asarray(place, np.float32)
        f[idx[at:at + size]] = spot
        at += size
    f[idx[at:at + origin]] = 0.0
    return f


Case = namedtuple("Case", "name branch d frames claim hash_claim twice")
CASES = []


def case(name, branch, d, frames, claim, hash_claim=None, twice=False):
    """frames: a list of zero-argument functions, one per frame, each returning [N][d] features"""
    CASES.append(Case(name, branch, d, frames, claim, hash_claim, twice))


def features(c):
    """(the features of every frame, the batch's max_points: its largest frame)"""
    fs = [np.ascontiguousarray(f(), np.float32).reshape(-1, c.d) for f in c.frames]
    return fs, max(f.shape[0] for f in fs)


def only(**want):
    """the report has these values, and no long bucket went any other way"""
    ways = ("long_by_bitmap", "long_by_network_uniform", "long_by_network_mixed", "long_by_network_wide")

    def claim(rs):
        r = rs[0]
        ok = all(r[k] == v if not callable(v) else v(r[k]) for k, v in want.items())
        return ok and all(r[w] == 0 for w in ways if w not in want) and sum(r[w] for w in ways) == r["long_buckets"]
    return claim


N0 = PERM_MIN
at_least = lambda n: (lambda x: x >= n)

# point buckets: 64 / 65 points of one cell, every other cell far below
case("point_bucket_64", "k_sort_place: a bucket of 64 points is put in index order", 2, [lambda: frame(1, N0, 2, [(64, 0)], box=(6.0, 150.0))],
     only(largest_point_bucket=64, point_buckets_over_64=0, long_buckets=0), only(largest_point_bucket=64, point_buckets_over_64=0))
case("point_bucket_65", "k_sort_place: a bucket of 65 points keeps its arrival order", 2, [lambda: frame(1, N0, 2, [(65, 0)], box=(6.0, 150.0))],
     only(largest_point_bucket=65, point_buckets_over_64=1, long_buckets=0), only(largest_point_bucket=65, point_buckets_over_64=1), twice=True)
# uniform long buckets: a cluster of n points is d + 1 buckets of n entries of one code (direct codes)
case("uniform_512", "k_eorder: a bucket of 512 entries is ranked in place", 2, [lambda: frame(2, N0, 2, [(512, 0)])],
     only(direct_codes=1, long_buckets=0))
case("uniform_513", "k_esort_long: a uniform bucket of 513 entries takes the network", 2, [lambda: frame(2, N0, 2, [(513, 0)])],
     only(direct_codes=1, long_buckets=3, long_by_network_uniform=3, max_buckets_per_workgroup=1))
case("uniform_1023", "k_esort_long: a uniform bucket of 1023 entries takes the network", 2, [lambda: frame(2, N0, 2, [(1023, 0)])],
     only(direct_codes=1, long_buckets=3, long_by_network_uniform=3))
case("uniform_1024", "k_esort_long: a uniform bucket of 1024 entries takes the bitmap, a word per lane", 2,
     [lambda: frame(2, N0, 2, [(1024, 0)], where="head")], only(direct_codes=1, long_buckets=3, long_by_bitmap=3))
case("bitmap_over_256_words", "k_esort_long: a bitmap of more than 256 words, several per lane", 2,
     [lambda: frame(2, N0, 2, [(1024, 0)], where="spread")], only(direct_codes=1, long_buckets=3, long_by_bitmap=3))
# a mixed long bucket: a tight cluster of DIFFERENT points inside a wide box, multiply-high buckets of many codes
case("mixed_long_bucket", "k_esort_long: a bucket of several codes takes the network, ordered by (code, id)", 2,
     [lambda: tight_cluster(3, N0, 2, 700)], only(direct_codes=0, long_buckets=at_least(1), long_by_network_mixed=at_least(1)))
# more than 64 long buckets: 17 clusters at d = 3 are 68 buckets, bitmap and network ones mixed
case("over_64_long_buckets", "k_esort_long: a workgroup takes a second bucket", 3,
     [lambda: frame(4, 11200, 3, [(1024 if i % 6 == 0 else 520 + i, i) for i in range(17)], box=(6.0, 14.0))],
     only(long_buckets=68, long_by_bitmap=12, long_by_network_uniform=56, max_buckets_per_workgroup=2), lambda rs: rs[0]["long_rows"] == 68)
# direct codes or multiply-high: a narrow and a wide box at the same N
case("box_narrow", "k_vsort_plan: the code is its own bucket", 3, [lambda: frame(5, N0, 3, box=(6.0, 16.0))], only(direct_codes=1, long_buckets=0))
case("box_wide", "k_vsort_plan: multiply-high buckets", 3, [lambda: frame(5, N0, 3, box=(6.0, 900.0))], only(direct_codes=0, long_buckets=0))
# phantom points: N % 4 = 1, 2, 3, 0, with nothing real at the origin (their vertices have empty rows) and with real points there
for m in (1, 2, 3, 0):
    ph = ((4 - m) % 4) * 3
    case("phantoms_mod%d_alone" % m, "k_eflag / k_eoffsets: %d phantom entries make vertices with empty rows" % ph, 2,
         [lambda m=m: frame(6, N0 + 4 + m, 2)], only(phantom_entries=ph, empty_row_vertices=3 if ph else 0, long_buckets=0))
    case("phantoms_mod%d_at_origin" % m, "k_eflag / k_eoffsets: %d phantom entries end real runs" % ph, 2,
         [lambda m=m: frame(6, N0 + 4 + m, 2, origin=5)], only(phantom_entries=ph, empty_row_vertices=0, long_buckets=0))
case("phantoms_in_bitmap", "k_esort_long: a giant origin vertex takes the phantom entries into a bitmap bucket", 2,
     [lambda: frame(7, N0 + 5, 2, origin=1100)], only(phantom_entries=9, empty_row_vertices=0, long_buckets=3, long_by_bitmap=3))
case("phantoms_first", "k_eflag: position 0 of the sorted order belongs to a phantom run", 2,
     [lambda: frame(8, N0 + 5, 2, sign=(1, -1))], only(phantom_entries=9, empty_row_vertices=3, long_buckets=0))
case("phantoms_last", "k_eoffsets: the last runs of the sorted order are the phantom points' alone", 2,
     [lambda: frame(8, N0 + 5, 2, sign=(-1, 1))], only(phantom_entries=9, empty_row_vertices=3, long_buckets=0))
# ragged batches: an empty frame (a plan of span 2), a frame of one point, frames of different sizes
ragged = [lambda: frame(9, N0, 2), lambda: np.zeros((0, 2), np.float32), lambda: frame(10, 1, 2), lambda: frame(11, N0 - 37, 2)]
case("ragged", "frames of N, 0, 1 and N - 37 points", 2, ragged,
     lambda rs: [r["phantom_entries"] for r in rs] == [0, 0, 9, 3] and rs[1]["direct_codes"] == 1 and rs[2]["empty_row_vertices"] == 3)
case("ragged_empty_first", "the same with the empty frame first", 2, [ragged[1], ragged[0], ragged[2], ragged[3]],
     lambda rs: [r["phantom_entries"] for r in rs] == [0, 0, 9, 3] and rs[0]["direct_codes"] == 1)
# the scans' tile of 4096: n = Epad + 1 is always 1 mod 4 -- 4096 k + 1 (every case of 8192 points at d = 2) and 4096 k - 3
case("scan_tile_one_over", "scan_frames: Epad + 1 = 6 tiles and one element", 2, [lambda: frame(12, N0, 2)],
     lambda rs: (N0 * 3 + 1) % SCAN_TILE == 1 and rs[0]["phantom_entries"] == 0)
case("scan_tile_three_short", "scan_frames: Epad + 1 = 7 tiles less three elements", 2, [lambda: frame(12, 9556, 2)],
     lambda rs: (9556 * 3 + 1) % SCAN_TILE == SCAN_TILE - 3 and rs[0]["phantom_entries"] == 0)
# the hash build's rows (the sorted build meets no long bucket here)
case("rows_128", "k_csr_order: a row of 128 entries is ranked in place", 2, [lambda: frame(13, N0, 2, [(128, 0)])],
     only(long_buckets=0), lambda rs: rs[0]["long_rows"] == 0)
case("rows_129_and_777", "k_csr_sort_long: rows of 129 and of 777 entries (no power of two)", 2,
     [lambda: frame(13, N0, 2, [(129, 0), (777, 1)])], only(long_buckets=3, long_by_network_uniform=3), lambda rs: rs[0]["long_rows"] == 6)
# the one large case: ids spanning more than the bitmap holds (15872 words = 507 904 ids need 56 434 points at d = 8)
case("wide_id_span", "k_esort_long: a uniform bucket whose ids span more than the bitmap takes the network", 8,
     [lambda: wide_span(14, 56500)],
     lambda rs: rs[0]["long_by_network_wide"] >= 1 and rs[0]["long_by_bitmap"] >= 1 and rs[0]["max_buckets_per_workgroup"] >= 3
     and 56500 * 9 > BITMAP_WORDS * 32)


def tight_cluster(seed, N, d, n):
    """a wide box (multiply-high buckets of many codes) with n different points inside one cell"""
    rng = np.random.default_rng(seed)
    f = frame(seed, N, d, box=(6.0, 900.0))
    f[rng.permutation(N)[:n]] = (np.float32(300.0) + rng.random((n, d)) * 0.8).astype(np.float32)
    return f


def wide_span(seed, N):
    """d = 8: 1100 identical points, the first and the last of the frame among them; every other point within a few cells"""
    rng = np.random.default_rng(seed)
    f = (rng.random((N, 8)) * 1.5 + 6.0).astype(np.float32)
    idx = np.concatenate([[0, N - 1], 1 + rng.permutation(N - 2)[:1098]])
    f[idx] = np.float32(6.5)
    return f


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def unary(seed, n):
    return (np.random.default_rng(1000 + seed).random((n, 2)) * 3.0).astype(np.float32)


_ORACLE = {}


def oracle(po, c):
    """per frame of the case: (reference tables, Q and labels after T iterations at RELAX, features, unary) -- computed once"""
    if c.name not in _ORACLE:
        fs, _ = features(c)
        out = []
        for i, f in enumerate(fs):
            n = f.shape[0]
            u = unary(i, n)
            if n == 0:
                ref = dict(d=c.d, N=0, V=0, offset=np.zeros((0, c.d + 1), np.int32), bary=np.zeros((0, c.d + 1), np.float32),
                           nbr=np.zeros((c.d + 1, 0, 2), np.int32), keys=np.zeros((0, c.d), np.int16))
                out.append((ref, np.zeros((0, 2), np.float32), np.zeros(0, np.int16), f, u))
                continue
            o = po.OracleCRF(n, 2)
            o.set_unary(u)
            o.add_pairwise(f, 1.0)
            ref = sc.reference_tables(o, 0)
            o.inference_native(T, True, RELAX)
            out.append((ref, o.probability(), o.map(), f, u))
            o.close()
        _ORACLE[c.name] = out
    return _ORACLE[c.name]


def expected(po, c, sorted_build):
    fs, max_points = features(c)
    vcap = ((max_points + 3) & ~3) * (c.d + 1)
    return [expected_report(ref, f, max_points, vcap, sorted_build) for (ref, _, _, f, _) in oracle(po, c)]

"""Frames that drive the three HASH lattice builds where seeded random frames never go -- long probe chains, chains over the end of the
table, nearly full and overfull tables, every step of the capacity rules, the reserved key -- with the hashes and the capacity rules
restated in numpy and a linear-probing MODEL that says, without a GPU, what each frame reaches (notes/hash_build_tests.md).

    build                                        table                          hash                       capacity
    k_frame and the kernels on frame_body.inc    LDS, the packed 32-bit keys    hash32   (frame_build.h)   frame_hcap(NA)    1024 .. 8192
    k_build_small<D>, d <= 3 (build_small.hip)   LDS, entry ids (lowest wins)   hash_key (device_math.h)   small_hcap(NA, d) >= 1.5 live
    k_insert / find_vertex (stream_build.hip)    HBM, entry ids, one per frame  hash_key                   stream_cap(maxN, d) >= 2 Epad

The hashes are fixed functions, so a frame that reaches a given slot can be CONSTRUCTED: windowed_frame() keeps, out of a pool of
candidate points, those with a vertex whose home slot lies in a window of W slots at the end (or the start) of the table the build
will use.  A few hundred keys homing in 16 slots are one cluster that runs over the end of the table and on from slot 0.

The model (Table) knows the occupied slot SET, which does not depend on the insertion order, and so the path of every lookup of an
ABSENT key; for the keys that are there it uses one legal placement, the oracle's first-occurrence order.  FAULTS are planted on the
model alone (neighbours()); tests/test_hash_build_cases.py shows that each changes the lattice on the cases built for it.  The
constants of the restated rules are READ from the sources as well (constants()): a rule that changes fails that test instead of
silently moving the cases.
"""
import os
import re
from collections import namedtuple

import numpy as np

import frame_lean_cases as fc
import sorted_build_checker as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lc-crf-slam_amd", "csrc")
M32 = 0xffffffff
T, RELAX = 3, 1.0                                        # the inference every case is compared after

# ---- the rules, restated -------------------------------------------------------------------------------------------------------------
EMPTY_KEY = 0x80008000                                   # kEmptyKey: (-32768, -32768) packed
HASH32 = (2654435761, 15, 2246822519, 13)                # fb::hash32: multiply, xor-shift, multiply, xor-shift
HASH_KEY = (1664525, 15, 2246822519, 13)                 # hash_key<D>: per coordinate add and multiply, then the same tail
FRAME_HCAP = (3, 1024, 8192)                             # frame_hcap: live = 3 * Npad; from 1024, doubled while < live, at most 8192
SMALL_HCAP = (1024, 2)                                   # small_plan: from 1024, doubled while < live + live / 2
SMALL_LIMITS = (3, 12, 1024)                             # build_small_supported: d <= 3 and Npad * (d + 1) <= 12 * 1024
STREAM_CAP = (2, 16)                                     # Engine::add_kernel: next_pow2(2 * Epad), next_pow2 starts at 16
FRAME_LDS, FRAME_HDR, DUAL_VCAP = 160 * 1024, 512, 8192  # kLdsLimit, kHdr, kDualVcap


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: %d matches of %r (the rule's code changed shape: restate it here)" % (what, len(m), pattern)
    return m[0]


def constants():
    """the numbers of the hashes and the capacity rules, from the code as it stands"""
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("frame_build.h", "frame_body.h", "device_math.h", "build_small.hip",
                                                            "host_engine.hip", "host_engine.h", "fused_loop.h")}
    ints = lambda t: tuple(int(x, 0) for x in t)
    c = {}
    c["EMPTY_KEY"] = int(_one(r"constexpr unsigned kEmptyKey = (0x[0-9a-fA-F]+)u;", src["frame_build.h"], "kEmptyKey"), 16)
    c["HASH32"] = ints(_one(r"unsigned h = key \* (\d+)u;\s+h \^= h >> (\d+);\s+h \*= (\d+)u;\s+h \^= h >> (\d+);\s+return h;",
                            src["frame_build.h"], "hash32"))
    c["HASH_KEY"] = ints(_one(r"unsigned h = 0;\s+#pragma unroll\s+for \(int i = 0; i < D; \+\+i\) \{\s+h \+= \(unsigned\)\(int\)key\[i\];\s+"
                              r"h \*= (\d+)u;\s+\}\s+h \^= h >> (\d+);\s+h \*= (\d+)u;\s+h \^= h >> (\d+);\s+return h;",
                              src["device_math.h"], "hash_key"))
    c["FRAME_HCAP"] = ints(_one(r"const int live = (\d+) \* \(\(NA \+ 3\) & ~3\);\s+int h = (\d+);\s+while \(h < live && h < (\d+)\) h <<= 1;\s+return h;",
                                src["frame_body.h"], "frame_hcap"))
    _one(r"const long live = \(long\)\(\(NA \+ 3\) & ~3\) \* kd\.D1;", src["build_small.hip"], "small_plan's live")
    c["SMALL_HCAP"] = ints(_one(r"p\.hcap = (\d+);\s+while \(p\.hcap < live \+ live / (\d+)\) p\.hcap <<= 1;", src["build_small.hip"], "small_plan"))
    c["SMALL_LIMITS"] = ints(_one(r"kds\[k\]\.d > (\d+) \|\| \(long\)\(\(NA \+ 3\) & ~3\) \* kds\[k\]\.D1 > (\d+) \* kBT", src["build_small.hip"],
                                  "build_small_supported")) + (int(_one(r"constexpr int kBT = (\d+);", src["build_small.hip"], "kBT")),)
    _one(r"k\.Epad = maxNpad \* k\.D1;", src["host_engine.hip"], "Epad")
    c["STREAM_CAP"] = (int(_one(r"k\.cap = next_pow2\((\d+)L \* k\.Epad\);", src["host_engine.hip"], "the streaming cap")),
                       int(_one(r"inline int next_pow2\(long v\)\s+\{\s+long p = (\d+);\s+while \(p < v\) p <<= 1;", src["host_engine.h"], "next_pow2")))
    c["FRAME_LDS"] = int(_one(r"constexpr size_t kLdsLimit = (\d+) \* 1024;", src["fused_loop.h"], "kLdsLimit")) * 1024
    c["FRAME_HDR"] = int(_one(r"constexpr int kHdr = (\d+);", src["frame_build.h"], "kHdr"))
    c["DUAL_VCAP"] = int(_one(r"constexpr int kDualVcap = (\d+);", src["frame_body.h"], "kDualVcap"))
    return c


RESTATED = dict(EMPTY_KEY=EMPTY_KEY, HASH32=HASH32, HASH_KEY=HASH_KEY, FRAME_HCAP=FRAME_HCAP, SMALL_HCAP=SMALL_HCAP,
                SMALL_LIMITS=SMALL_LIMITS, STREAM_CAP=STREAM_CAP, FRAME_LDS=FRAME_LDS, FRAME_HDR=FRAME_HDR, DUAL_VCAP=DUAL_VCAP)


def _tail(h, s1, m2, s2):
    h ^= h >> np.uint64(s1)
    h = (h * np.uint64(m2)) & np.uint64(M32)
    h ^= h >> np.uint64(s2)
    return h


def pack2(keys):
    """[V][2] int16 keys as k_frame's table holds them: x | y << 16, both halves as unsigned 16-bit"""
    k = np.asarray(keys, np.int64).reshape(-1, 2) & 0xffff
    return (k[:, 0] | (k[:, 1] << 16)).astype(np.uint64)


def unpack2(packed):
    p = np.asarray(packed, np.uint64).astype(np.int64)
    return np.stack([p & 0xffff, p >> 16], -1).astype(np.uint16).view(np.int16)


def hash32(packed):
    m1, s1, m2, s2 = HASH32
    h = (np.asarray(packed, np.uint64) * np.uint64(m1)) & np.uint64(M32)
    return _tail(h, s1, m2, s2)


def hash_key(keys):
    """[V][d] int16 keys: uint32 arithmetic, every coordinate sign-extended to 32 bits"""
    m1, s1, m2, s2 = HASH_KEY
    k = np.asarray(keys, np.int64)
    h = np.zeros(k.shape[0], np.uint64)
    for i in range(k.shape[1]):
        h = (h + (k[:, i] & M32).astype(np.uint64)) & np.uint64(M32)
        h = (h * np.uint64(m1)) & np.uint64(M32)
    return _tail(h, s1, m2, s2)


def frame_hcap(NA):
    per, lo, hi = FRAME_HCAP
    live, h = per * ((NA + 3) & ~3), lo
    while h < live and h < hi:
        h <<= 1
    return h


def small_hcap(NA, d):
    lo, div = SMALL_HCAP
    live, h = ((NA + 3) & ~3) * (d + 1), lo
    while h < live + live // div:
        h <<= 1
    return h


def small_supported(NA, d):
    dmax, mul, bt = SMALL_LIMITS
    return d <= dmax and ((NA + 3) & ~3) * (d + 1) <= mul * bt


def stream_cap(max_points, d):
    mul, p = STREAM_CAP
    while p < mul * ((max_points + 3) & ~3) * (d + 1):
        p <<= 1
    return p


def hcap_steps():
    """[(largest padded count below the step, smallest above it, capacity below, capacity above)] of frame_hcap"""
    per, lo, hi = FRAME_HCAP
    out, h = [], lo
    while h < hi:
        below = (h // per) & ~3
        out.append((below, below + 4, h, 2 * h))
        assert frame_hcap(below) == h and frame_hcap(below + 4) == 2 * h
        h <<= 1
    return out


def frame_plan_fits(N, V, rowmax0, hcap, lds=FRAME_LDS, dual=False):
    """csrc/frame_body.inc's LDS plan for lattices of V[k] vertices (phase C's scratch beside the hash table, then the loop's product
    buffers; dual: the two-workgroup form, kernel 1 built by the helper): does the kernel keep the frame?"""
    a16 = lambda b: (b + 15) & ~15
    K, Npad, E = len(V), (N + 3) & ~3, 3 * N
    W = (((Npad + 31) >> 5) + 3) & ~3
    ido_off = lds - 6 * hcap
    tables = lambda v: 2 * a16(8 * (v + 1)) + a16(12 * v) + a16(2 * (v + 2))
    plane = lambda v, chain: ((E + 14 * v + 16 if chain else E) + 63) & ~63
    chain0 = rowmax0 >= 64 and V[0] <= 16 + (1024 // 128 - 1) * 64 and E + 14 * V[0] + 64 < 65535

    def build(cursor, v):
        vs = cursor + tables(v) + a16(4 * v) + a16(4 * (v + 1))
        bitmap = E >= 16 * v and vs + 5 * v * W + 64 <= ido_off
        list_cap = (E + 7 * v + 8) & ~7
        in_hash = not bitmap and 2 * list_cap <= lds - ido_off
        end = vs + 4 * v * W + v * W // 2 if bitmap else vs if in_hash else vs + 2 * list_cap
        return end <= ido_off and v < 32767 and E + 7 * v < 65535 and v <= hcap

    if dual:
        assert K == 2
        helper = build(FRAME_HDR, V[1]) and V[1] <= DUAL_VCAP and FRAME_HDR + tables(V[1]) + 8 * plane(0, False) <= lds
        cursor = FRAME_HDR + tables(V[0]) + a16(8 * max(plane(V[0], chain0), plane(0, False)))
        return helper and build(FRAME_HDR, V[0]) and cursor <= lds and cursor + tables(V[1]) <= lds
    cursor = FRAME_HDR
    for v in V:
        if not build(cursor, v):
            return False
        cursor += tables(v)
    planes = [a16(8 * plane(v, k == 0 and chain0)) for k, v in enumerate(V)]
    return cursor + min(sum(planes), max(planes)) <= lds


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
FAULTS = ("no_wrap", "stop_at_first_foreign_key", "id_from_home_slot", "reserved_key_found")
ABSENT, GARBAGE = -1, -2                                 # a neighbour that is not there; an id read from a slot nobody wrote


def n2_keys(keys):
    """[d + 1][V][d]: the blur neighbour n2 of every vertex along every axis (permutohedral_cpu.h:408-421: key + 1, coordinate `axis`
    key - d; axis d touches the implied last coordinate only), wrapped to int16 as the reference's short arithmetic wraps"""
    k = np.asarray(keys, np.int64)
    V, d = k.shape
    out = np.repeat((k + 1)[None], d + 1, 0)
    for j in range(d):
        out[j, :, j] = k[:, j] - d
    return out.astype(np.int16)


class Table:
    """An open-addressing table with linear probing, `cap` slots (a power of two): the distinct keys [V][d] in the order of their ids
    (the oracle's: first occurrence), `home` [V] their home slots.  keys_in_slots: the slots hold the packed keys themselves
    (k_frame's table: EMPTY_KEY is reserved) and not entry ids."""

    def __init__(self, keys, home, cap, hashf, keys_in_slots=False, wrap=True):
        self.keys, self.cap, self.hashf, self.keys_in_slots, self.wrap = np.asarray(keys, np.int16), int(cap), hashf, keys_in_slots, wrap
        self.home = np.asarray(home, np.int64)
        V = self.V = self.keys.shape[0]
        assert cap & (cap - 1) == 0 and self.home.shape == (V,) and (V == 0 or (0 <= self.home.min() and self.home.max() < cap))
        nxt = list(range(cap + 1))                       # first empty slot at or behind a slot (cap: off the end), path-compressed

        def find(h):
            r = h
            while nxt[r] != r:
                r = nxt[r]
            while nxt[h] != r:
                nxt[h], h = r, nxt[h]
            return r
        self.slot = np.full(V, -1, np.int64)             # slot of every key, -1: not inserted (the table was full, or no_wrap ran off its end)
        for v in range(V):
            s = find(int(self.home[v]))
            if s == cap and wrap:
                s = find(0)
            if s == cap:
                continue
            self.slot[v] = s
            nxt[s] = s + 1
        self.owner = np.full(cap, -1, np.int64)          # slot -> id of the key in it
        ok = self.slot >= 0
        self.owner[self.slot[ok]] = np.flatnonzero(ok)
        self.occupied = self.owner >= 0
        self.dropped = int((~ok).sum())
        self.load = float(self.occupied.sum()) / cap
        # distance from every slot to the first empty one at or behind it, cyclically (cap: there is none)
        empty = np.flatnonzero(~self.occupied)
        if empty.size:
            nxt_e = empty[np.searchsorted(empty, np.arange(cap)) % empty.size]
            self.to_empty = (nxt_e - np.arange(cap)) % cap
        else:
            self.to_empty = np.full(cap, cap, np.int64)
        self.index = {k.tobytes(): i for i, k in enumerate(self.keys)}

    def past_wrap(self):
        """occupied slots from slot 0 onwards that belong to the cluster running over the end of the table (0: slot cap - 1 is empty)"""
        if not self.occupied[self.cap - 1]:
            return 0
        return int(self.to_empty[0]) if self.to_empty[0] < self.cap else self.cap

    def displaced_across_wrap(self):
        """keys that sit in a slot BELOW their home slot: their probe chain ran over the end of the table"""
        ok = self.slot >= 0
        return int((self.slot[ok] < self.home[ok]).sum())

    def longest_chain(self):
        ok = self.slot >= 0
        return int((((self.slot[ok] - self.home[ok]) % self.cap) + 1).max()) if ok.any() else 0

    def lookups(self):
        """every (axis, vertex) blur query: dict of [d + 1][V] arrays -- id (the id found, ABSENT), home, length (slots read), wraps
        (the path crosses from slot cap - 1 to slot 0), ends_empty (it ends at an empty slot), reserved (the query is EMPTY_KEY)"""
        q = n2_keys(self.keys)
        D1, V, d = q.shape
        flat = q.reshape(-1, d)
        home = (self.hashf(flat).astype(np.int64) & (self.cap - 1)).reshape(D1, V)
        ident = np.array([self.index.get(k.tobytes(), ABSENT) for k in flat], np.int64).reshape(D1, V)
        there = ident >= 0
        there[there] = self.slot[ident[there]] >= 0
        ident = np.where(there, ident, ABSENT)
        length = np.where(there, (self.slot[np.maximum(ident, 0)] - home) % self.cap + 1, np.minimum(self.to_empty[home] + 1, self.cap))
        reserved = pack2(flat).reshape(D1, V) == EMPTY_KEY if d == 2 else np.zeros((D1, V), bool)
        return dict(id=ident, home=home, length=length, wraps=home + length - 1 >= self.cap,
                    ends_empty=~there & (self.to_empty[home] < self.cap), reserved=reserved)

    def neighbours(self, fault=None):
        """(V, n2 [d + 1][V]) as a build with the planted fault would leave them -- ids, ABSENT, or GARBAGE for an id taken from an
        empty slot.  None: the right answer."""
        assert fault is None or fault in FAULTS
        if fault == "no_wrap":                           # h + 1 without the mask: an insert that runs off the end is lost, a lookup stops there
            t = Table(self.keys, self.home, self.cap, self.hashf, self.keys_in_slots, wrap=False)
            lk = t.lookups()
            found = (lk["id"] >= 0) & ~lk["wraps"]
            renum = np.cumsum(t.slot >= 0) - 1           # the ids of the keys that made it
            return int((t.slot >= 0).sum()), np.where(found, renum[np.maximum(lk["id"], 0)], ABSENT)
        lk = self.lookups()
        n2 = lk["id"].copy()
        if fault == "stop_at_first_foreign_key":         # one probe: a key that is not in its home slot is reported absent
            n2[(n2 >= 0) & (lk["length"] > 1)] = ABSENT
        elif fault == "id_from_home_slot":               # the key is found down the chain, the id is read at the home slot
            n2 = np.where(n2 >= 0, self.owner[lk["home"]], n2)
        elif fault == "reserved_key_found" and self.keys_in_slots:   # the probe for EMPTY_KEY ends at an empty slot -- which holds EMPTY_KEY
            n2[lk["reserved"] & lk["ends_empty"]] = GARBAGE
        return int((self.slot >= 0).sum()), n2

    def summary(self):
        lk = self.lookups()
        absent = lk["id"] < 0
        return dict(cap=self.cap, V=self.V, load=round(self.load, 4), past_wrap=self.past_wrap(), displaced_across_wrap=self.displaced_across_wrap(),
                    longest_insert=self.longest_chain(), longest_lookup=int(lk["length"].max()) if self.V else 0,
                    absent_over_wrap=int((absent & lk["wraps"] & lk["ends_empty"]).sum()), found_over_wrap=int((~absent & lk["wraps"]).sum()),
                    reserved_queries=int(lk["reserved"].sum()), dropped=self.dropped)


def frame_table(keys, NA, wrap=True):
    """k_frame's table for a d = 2 lattice in a launch whose largest frame has NA points"""
    cap = frame_hcap(NA)
    return Table(keys, hash32(pack2(keys)).astype(np.int64) & (cap - 1), cap, lambda k: hash32(pack2(k)), True, wrap)


def small_table(keys, NA):
    cap = small_hcap(NA, np.asarray(keys).shape[1])
    return Table(keys, hash_key(keys).astype(np.int64) & (cap - 1), cap, hash_key)


def stream_table(keys, max_points):
    cap = stream_cap(max_points, np.asarray(keys).shape[1])
    return Table(keys, hash_key(keys).astype(np.int64) & (cap - 1), cap, hash_key)


# ---- the oracle's lattices ---------------------------------------------------------------------------------------------------------------
def lattice(po, feat):
    """the oracle's lattice of a feature array with the phantom points' rows (sorted_build_checker.reference_tables): dict(d, N, V,
    offset [Npad][d + 1], bary, nbr, keys [V][d])"""
    f = np.ascontiguousarray(feat, np.float32)
    o = po.OracleCRF(f.shape[0], 2)
    o.set_unary(np.zeros((f.shape[0], 2), np.float32))
    o.add_pairwise(f, 1.0)
    ref = sc.reference_tables(o, 0)
    ref["norm"] = o.kernel(0)["norm"]
    o.close()
    return ref


# ---- the constructor ---------------------------------------------------------------------------------------------------------------------
OFFS = ((0.11, 0.23), (0.13, 0.26), (0.09, 0.21))        # places inside ONE simplex beside a cell (frame_lean_cases.at_cell)
_POOLS = {}


def pool(po, d, size, seed=0):
    """(features [P][d], the oracle's keys [V][d], offset [P][d + 1]) of the candidate points: d = 2 the cells of a size x size grid
    (frame_lean_cases.at_cell: one point per cell, every vertex shared by three cells), else `size` seeded random points"""
    key = (d, size, seed)
    if key not in _POOLS:
        if d == 2:
            g = np.arange(size) - size // 2
            u, v = np.meshgrid(g, 3 * g, indexing="ij")
            f = fc.at_cell(u.ravel(), v.ravel(), OFFS[0])
        else:
            box = {1: 25000.0, 3: 60.0}.get(d, 30.0)          # (d = 1: keys up to +-29000, 29000 vertices in all)
            f = (np.random.default_rng([77, d, size, seed]).random((size, d)) * box).astype(np.float32)
        ref = lattice(po, f)
        assert ref["offset"].shape[0] == f.shape[0], "pools are multiples of four points: no phantom point among the candidates"
        _POOLS[key] = (f, ref["keys"], ref["offset"])
    return _POOLS[key]


def windowed_frame(po, d, N, cap, hashf, W=16, where="end", per_cell=1, pool_size=None, seed=0, distinct=False):
    """N points of d features, each with at least one vertex whose home slot (hashf(key) & (cap - 1)) lies in the last -- where="start":
    the first -- W slots of a table of `cap` slots; per_cell points in every chosen cell (d = 2).  distinct: no two chosen points share
    a vertex (the lattice gets (d + 1) vertices per point)."""
    size = pool_size or (POOL2 if d == 2 else 60000)
    f, keys, off = pool(po, d, size, seed)
    home = hashf(keys).astype(np.int64) & (cap - 1)
    inwin = home >= cap - W if where == "end" else home < W
    cand = np.flatnonzero(inwin[off].any(1))
    cells = -(-N // per_cell)
    if distinct:
        seen, keep = set(), []
        for p in cand:
            vs = set(off[p].tolist())
            if not (vs & seen):
                keep.append(p)
                seen |= vs
        cand = np.array(keep, np.int64)
    assert cand.size >= cells, "the pool of %d candidates holds %d of the %d wanted: take a larger one" % (f.shape[0], cand.size, cells)
    # every stride-th candidate, not the first ones: a neighbour key that homes in the window belongs to a candidate as well, and among
    # a PREFIX of the candidates it would nearly always be there -- spread out, the frame also looks up ABSENT keys inside the cluster
    pick = cand[::cand.size // cells][:cells]
    if d == 2 and per_cell > 1:
        g = size
        u, v = np.divmod(pick, g)
        out = np.concatenate([fc.at_cell(u - g // 2, 3 * (v - g // 2), OFFS[r]) for r in range(per_cell)])
        out = out.reshape(per_cell, cells, 2).transpose(1, 0, 2).reshape(-1, 2)       # the points of a cell side by side
        return np.ascontiguousarray(out[:N])
    assert per_cell == 1
    return np.ascontiguousarray(f[pick])


def isolated(n):
    """n points in cells of their own on a grid spaced (3, 6): no two share a vertex, V = 3 n"""
    idx = np.arange(n)
    side = int(np.ceil(np.sqrt(n)))
    return fc.at_cell(3 * (idx % side) - 3 * (side // 2), 6 * (idx // side) - 6 * (side // 2))


# ---- the cases of the frame body (d = 2, two labels) ----------------------------------------------------------------------------------------
RESERVED_VERTEX, RESERVED_NEIGHBOUR = (0.11, 32767.23), (0.11, 32766.23)
# route: "fit" (the kernel must keep the frame), "fallback" (it must flag exactly this frame), "any" (the oracle's bits by either route)
POOL2 = 300                                              # d = 2: the cells of a 300 x 300 grid, three vertices each, none shared
# name -> (points, window, points per cell).  One point per cell is 3 N vertices: the table all but full, the run past the wrap nearly
# the whole table.  From 1364 points on 3 N vertices no longer fit the kernel's LDS beside the table: three points per cell.
WINDOWS = {"wrap_1024": (340, 16, 1), "wrap_2048": (680, 16, 1), "wrap_4096": (1364, 32, 3),
           "nearly_full_1024": (340, 64, 1), "nearly_full_2048": (680, 64, 1), "shared_cells": (339, 16, 3)}
STEP_WINDOW = 24


def _slam(N, seed):
    import importlib
    return importlib.import_module("lc-crf-slam_amd.workloads").slam_problem(N, seed=seed)


def frame_features(po, name):
    """the features [N][2] a case puts on ONE kernel of a SLAM frame"""
    hf = lambda k: hash32(pack2(k))
    if name.startswith("hcap_step_"):
        N = int(name.rsplit("_", 1)[1])
        return windowed_frame(po, 2, N, frame_hcap(N), hf, W=STEP_WINDOW * max(frame_hcap(N) // 4096, 1), per_cell=3 if N > 1024 else 1, pool_size=POOL2)
    if name in WINDOWS:
        N, W, per = WINDOWS[name]
        return windowed_frame(po, 2, N, frame_hcap(N), hf, W=W, per_cell=per, pool_size=POOL2)
    if name == "overfull_8192":
        return isolated(4096)
    if name in ("reserved_vertex", "reserved_neighbour"):
        f = np.array(_slam(300, 41)["kernels"][1][0], np.float32)
        f[150] = RESERVED_VERTEX if name == "reserved_vertex" else RESERVED_NEIGHBOUR
        return f
    raise ValueError(name)


def _steps_names():
    out = []
    for below, above, _, _ in hcap_steps():
        out += ["hcap_step_%d" % below, "hcap_step_%d" % above]
    return out


FRAME_CASES = {
    "wrap_1024": ("fit", "a cluster of the 1024-slot table runs over its end: inserts and neighbour lookups wrap"),
    "wrap_2048": ("fit", "the same in the 2048-slot table"),
    "wrap_4096": ("fit", "the same in the 4096-slot table"),
    "nearly_full_1024": ("fit", "load >= 0.99 at 1024 slots: nearly every lookup walks a long chain"),
    "nearly_full_2048": ("fit", "load >= 0.99 at 2048 slots"),
    "overfull_8192": ("fallback", "more distinct keys than the largest table has slots: the insert gives up after hcap probes"),
    "reserved_vertex": ("fallback", "a vertex IS the reserved key (-32768, -32768): phase B flags the frame"),
    "reserved_neighbour": ("any", "the reserved key is a neighbour QUERY and no vertex: the lookup must report it absent"),
    "shared_cells": ("fit", "three points per cell and a phantom point: every vertex is claimed by several entries at once"),
}
for _n in _steps_names():
    FRAME_CASES[_n] = ("fit", "frame_hcap's step: %s points take %d slots" % (_n.rsplit("_", 1)[1], frame_hcap(int(_n.rsplit("_", 1)[1]))))
FITTING = [n for n, (r, _) in FRAME_CASES.items() if r == "fit"]
_FRAME = {}


def frame_case(po, name):
    """(features [N][2], lattice of those features, table as k_frame builds it for a launch whose largest frame is this one)"""
    if name not in _FRAME:
        f = frame_features(po, name)
        f.setflags(write=False)
        ref = lattice(po, f)
        _FRAME[name] = (f, ref, frame_table(ref["keys"], f.shape[0]))
    return _FRAME[name]


def frame_problem(po, name, where):
    """a two-label SLAM frame of the case's point count with the case's features as kernel `where` (0, 1), as both ("both"), or
    alone ("alone": K = 1)"""
    f = frame_case(po, name)[0]
    pb = _slam(f.shape[0], 500 + fc.hash_name(name) % 97)
    (f0, w0), (f1, w1) = pb["kernels"]
    if where == "alone":
        return dict(pb, kernels=[(f, w1)])
    return dict(pb, kernels=[(f if where in (0, "both") else f0, w0), (f if where in (1, "both") else f1, w1)])


def neighbour_problem(N, seed=0):
    """an ordinary SLAM frame to sit beside a case in a batch: NO larger than the case, or the launch would take another capacity"""
    return _slam(N, 900 + seed)


# ---- the cases of the entry-id tables (k_build_small: d = 1, 2, 3; the streaming build: d = 5, 8 and d = 2 beyond 4096 points) -------------
SmallCase = namedtuple("SmallCase", "name d frames claim")
SMALL_N = {1: 340, 2: 224, 3: 168}                       # the most points of a 1024-slot table: (d + 1) Npad * 1.5 <= 1024


def small_cases(po):
    """[(name, d, [features per frame])]: every frame of a case has at most SMALL_N[d] points, so that small_plan takes 1024 slots"""
    out = []
    for d in (1, 2, 3):
        n, cap = SMALL_N[d], small_hcap(SMALL_N[d], d)
        assert cap == 1024 and small_hcap(n + 4, d) == 2048
        size = {1: 40000, 2: POOL2, 3: 40000}[d]
        # (d = 1: a vertex's neighbours are the next keys along the line -- only points apart from each other look up absent ones)
        wrap = windowed_frame(po, d, n - 40, cap, hash_key, W=32 if d == 1 else 8, pool_size=size, distinct=d == 1)
        full = windowed_frame(po, d, n, cap, hash_key, W=16, pool_size=size, distinct=True)
        start = windowed_frame(po, d, n - 41, cap, hash_key, W=8, where="start", pool_size=size)
        out.append(("small_wrap_d%d" % d, d, [wrap, start]))
        out.append(("small_two_thirds_d%d" % d, d, [full]))
    shared = windowed_frame(po, 2, 222, 1024, hash_key, W=16, per_cell=3)
    out.append(("small_shared_cells_d2", 2, [shared, shared[::-1].copy()]))
    return out


def stream_cases(po):
    """[(name, d, max_points, [features per frame])] for engine 1: frame 0's cluster runs over the end of ITS table, frame 1's keys home
    in the first slots of its own, a ragged third frame of ordinary points"""
    out = []
    for d, n, size in ((5, 600, 60000), (8, 400, 40000)):
        cap = stream_cap(n, d)
        rng = np.random.default_rng([5, d])
        ragged = (rng.random((n - 123, d)) * 8.0).astype(np.float32)
        out.append(("stream_two_frames_d%d" % d, d, n, [windowed_frame(po, d, n, cap, hash_key, W=16, pool_size=size),
                                                         windowed_frame(po, d, n - 100, cap, hash_key, W=16, where="start", pool_size=size),
                                                         ragged]))
    n, cap = 4100, stream_cap(4100, 2)
    assert not small_supported(n, 2) and small_supported(4096, 2)
    rng = np.random.default_rng(6)
    fill = lambda m: (rng.random((m, 2)) * 40.0 - 20.0).astype(np.float32)
    f0 = np.concatenate([windowed_frame(po, 2, 600, cap, hash_key, W=64, per_cell=3), fill(n - 600)])
    f1 = np.concatenate([fill(n - 700), windowed_frame(po, 2, 597, cap, hash_key, W=64, where="start", per_cell=3)])
    out.append(("stream_two_frames_d2_4100", 2, n, [f0, f1, fill(n - 1357)]))
    return out


def unary(seed, n):
    return (np.random.default_rng(2000 + seed).random((n, 2)) * 3.0).astype(np.float32)


_REFS = {}


def table_reference(po, key, feats):
    """per frame of an entry-id case: (lattice, Q and labels after T iterations, features, unary) -- computed once, read-only"""
    if key not in _REFS:
        out = []
        for i, f in enumerate(feats):
            n = f.shape[0]
            u = unary(i, n)
            o = po.OracleCRF(n, 2)
            o.set_unary(u)
            o.add_pairwise(f, 1.0)
            ref = sc.reference_tables(o, 0)
            ref["norm"] = o.kernel(0)["norm"]
            o.inference_native(T, True, RELAX)
            q, m = o.probability(), o.map()
            o.close()
            for a in (q, m, u):
                a.setflags(write=False)
            out.append((ref, q, m, f, u))
        _REFS[key] = out
    return _REFS[key]

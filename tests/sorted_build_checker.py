"""A numpy checker of the lattice tables AS BUILT by the streaming build in locality mode (csrc/stream_build.hip: the sorted build and,
with the points permuted, the hash build) against the oracle's lattice of the same features -- notes/sorted_build_tests.md.

Written apart from the library: nothing here knows how the tables are made, only what they must say.  The build's contract: "the same
arrays as after the hash build, with other ids; a vertex's row in ascending ORIGINAL point order; ids in row-major order of the code".

    ref    the oracle's lattice (reference numbering, caller's point order): reference_tables(OracleCRF, k)
           dict(d, N, V, offset [Npad][d+1], bary [Npad][d+1], nbr [d+1][V][2], keys [V][d]) -- the phantom points' rows included
    built  the probe's tables (BatchCRF.built_lattice): internal point order, the build's ids
           dict(perm [Npad], offset / bary [Npad][d+1], rowptr [V+1], csr_pt / csr_w [N (d+1)], nbr [d+1][V][2], fastn [V] or None, V)

check(ref, built, sorted_build) raises TableFault(kind, detail); the kinds are the keys of KINDS.  Every comparison is exact.
tests/test_sorted_build_checker.py shows without a GPU that a right table passes and that each kind of fault is caught by name.
"""
import numpy as np

KINDS = {
    "perm": "the internal point order is no permutation of the real points followed by the phantom points in place",
    "renumbering": "built id -> reference id is not a bijection on the V vertices (ids merged, split or out of range)",
    "bary": "a barycentric weight differs from the reference's bits",
    "neighbour redirected": "a blur neighbour is not the reference's under the renumbering",
    "neighbours exchanged": "n1 and n2 of a vertex are exchanged on one axis",
    "rowptr": "the rows' bounds do not count the real entries of every vertex",
    "phantom in a row": "a row lists a phantom point",
    "row content": "a row lists an entry of another vertex, or an entry twice",
    "row order": "a row is not strictly ascending in ORIGINAL point index",
    "row weight": "csr_w is not the entry's barycentric weight, bit for bit",
    "fastn": "fastn[v] != (n2 of v along axis 0 == v + 1)",
    "row-major ids": "the ids do not ascend in row-major order of the vertices' grid coordinates",
}


class TableFault(AssertionError):
    def __init__(self, kind, detail=""):
        assert kind in KINDS, kind
        super().__init__("%s: %s%s" % (kind, KINDS[kind], (" -- " + detail) if detail else ""))
        self.kind = kind


def reference_tables(o, k):
    """The oracle's lattice of term k with the rows of the phantom points (the frame padded to a multiple of four, at feature 0)."""
    lat = o.h.contents.pw[k].contents.lat
    D1, V, N, Np = lat.d + 1, lat.V, max(lat.N, 0), max(lat.Npad, 0)
    arr = lambda p, n, shape: np.ctypeslib.as_array(p, (max(n, 1),))[:n].reshape(shape).copy()
    return dict(d=lat.d, N=N, V=V, offset=arr(lat.offset, Np * D1, (Np, D1)), bary=arr(lat.bary, Np * D1, (Np, D1)),
                nbr=arr(lat.nbr, D1 * V * 2, (D1, V, 2)), keys=arr(lat.keys, V * lat.d, (V, lat.d)))


def grid_coords(keys):
    """c_j = (x_d - x_j) / (d + 1) of the lattice points with the given first d coordinates (x_d = -sum): the integer grid whose unit steps
    are the blur directions.  Exact: a lattice point's coordinates are congruent mod d + 1."""
    keys = np.asarray(keys, np.int64)
    d = keys.shape[1]
    xd = -keys.sum(1, keepdims=True)
    assert np.all((xd - keys) % (d + 1) == 0)
    return (xd - keys) // (d + 1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def renumbering(ref, built):
    """phi[id_built] = id_ref over every entry, the phantom points' included."""
    N, V = ref["N"], ref["V"]
    perm = np.asarray(built["perm"], np.int64)
    Np = perm.size
    if Np != ref["offset"].shape[0] or built["V"] != V:
        raise TableFault("renumbering", "Npad %d / V %d against the reference's %d / %d" % (Np, built["V"], ref["offset"].shape[0], V))
    if not (np.array_equal(np.sort(perm[:N]), np.arange(N)) and np.array_equal(perm[N:], np.arange(N, Np))):
        raise TableFault("perm")
    ob = np.asarray(built["offset"], np.int64).reshape(-1)
    orf = np.asarray(ref["offset"], np.int64)[perm].reshape(-1)
    if ob.size and (ob.min() < 0 or ob.max() >= V):
        raise TableFault("renumbering", "an id outside [0, %d)" % V)
    pairs = np.unique(ob * max(V, 1) + orf)
    b, r = pairs // max(V, 1), pairs % max(V, 1)
    if pairs.size != V or np.unique(b).size != V or np.unique(r).size != V:
        raise TableFault("renumbering", "%d (built, reference) pairs over %d built and %d reference ids, V = %d"
                         % (pairs.size, np.unique(b).size, np.unique(r).size, V))
    phi = np.empty(V, np.int64)
    phi[b] = r
    return phi


def check(ref, built, sorted_build):
    N, V, d = ref["N"], ref["V"], ref["d"]
    D1 = d + 1
    phi = renumbering(ref, built)
    perm = np.asarray(built["perm"], np.int64)
    inv = np.empty(V + 1, np.int64)                      # (inv[-1]: absent stays absent)
    inv[phi] = np.arange(V)
    inv[V] = -1

    if not np.array_equal(_bits(built["bary"]), _bits(ref["bary"][perm])):
        p, r = np.argwhere(_bits(built["bary"]) != _bits(ref["bary"][perm]))[0]
        raise TableFault("bary", "position %d (point %d), remainder %d" % (p, perm[p], r))

    want = inv[np.asarray(ref["nbr"], np.int64)[:, phi, :]]          # [D1][V][2] in the build's ids (-1 -> index V -> -1)
    got = np.asarray(built["nbr"], np.int64)
    if not np.array_equal(want, got):
        j, v = np.argwhere((want != got).any(2))[0]
        kind = "neighbours exchanged" if np.array_equal(want[j, v], got[j, v, ::-1]) else "neighbour redirected"
        raise TableFault(kind, "axis %d, vertex %d: (n1, n2) = %s, the reference's %s" % (j, v, got[j, v].tolist(), want[j, v].tolist()))

    rowptr = np.asarray(built["rowptr"], np.int64)
    ids = np.asarray(built["offset"], np.int64)
    counts = np.bincount(ids[:N].reshape(-1), minlength=V)          # real entries per vertex: 0 for a vertex only phantoms touch
    if rowptr.size != V + 1 or rowptr[0] != 0 or rowptr[V] != N * D1 or not np.array_equal(np.diff(rowptr), counts):
        bad = np.flatnonzero(np.diff(rowptr) != counts)[:1] if rowptr.size == V + 1 else []
        raise TableFault("rowptr", "rowptr[V] = %d for %d real entries; first wrong row %s" % (rowptr[-1], N * D1, list(bad)))
    pt = np.asarray(built["csr_pt"], np.int64)
    row = np.repeat(np.arange(V), counts)                 # the vertex of every CSR slot
    if pt.size and (pt.min() < 0 or pt.max() >= N):
        s = np.flatnonzero((pt < 0) | (pt >= N))[0]
        raise TableFault("phantom in a row", "slot %d of vertex %d lists position %d, N = %d" % (s, row[s], pt[s], N))
    hit = ids[pt] == row[:, None]                         # [N D1][D1]: the remainder under which the listed point touches the row's vertex
    if not np.all(hit.sum(1) == 1):
        s = np.flatnonzero(hit.sum(1) != 1)[0]
        raise TableFault("row content", "slot %d of vertex %d lists position %d, which does not touch it" % (s, row[s], pt[s]))
    rem = hit.argmax(1)
    if np.unique(pt * D1 + rem).size != N * D1:
        raise TableFault("row content", "an entry is listed twice")
    orig = perm[pt]
    same = row[1:] == row[:-1]
    if np.any(same & (orig[1:] <= orig[:-1])):
        s = np.flatnonzero(same & (orig[1:] <= orig[:-1]))[0]
        raise TableFault("row order", "vertex %d (row of %d): original points %d, %d at slots %d, %d" % (row[s], counts[row[s]], orig[s], orig[s + 1], s, s + 1))
    if not np.array_equal(_bits(built["csr_w"]), _bits(built["bary"])[pt, rem]):
        s = np.flatnonzero(_bits(built["csr_w"]) != _bits(built["bary"])[pt, rem])[0]
        raise TableFault("row weight", "slot %d of vertex %d" % (s, row[s]))

    if sorted_build:
        if built.get("fastn") is not None:
            nxt = got[0, :, 1] == np.arange(V) + 1
            fastn = np.asarray(built["fastn"])
            if not np.array_equal(fastn.astype(bool), nxt) or (fastn.size and fastn.max() > 1):
                v = np.flatnonzero((fastn != nxt.astype(fastn.dtype)))[0]
                raise TableFault("fastn", "vertex %d: fastn %d, n2 along axis 0 is %d" % (v, fastn[v], got[0, v, 1]))
        c = grid_coords(ref["keys"])[phi]                 # the grid coordinates of the build's vertices 0, 1, 2, ...
        if V > 1:
            diff = c[1:] - c[:-1]                         # row-major, coordinate 0 fastest: the LAST differing coordinate decides
            last = (d - 1) - np.argmax(diff[:, ::-1] != 0, axis=1)
            step = diff[np.arange(V - 1), last]
            if np.any(step <= 0):
                v = np.flatnonzero(step <= 0)[0]
                raise TableFault("row-major ids", "vertices %d, %d at %s, %s" % (v, v + 1, c[v].tolist(), c[v + 1].tolist()))
    return phi


def tables_from_reference(ref, vertex_order, point_order):
    """What a right build would leave for the reference's lattice: vertex_order[i] = the reference id that gets id i, point_order = the
    internal order of the real points (position -> original point).  The CPU test's stand-in for the device (and its faults' victim)."""
    N, V, d = ref["N"], ref["V"], ref["d"]
    D1 = d + 1
    Np = ref["offset"].shape[0]
    perm = np.concatenate([np.asarray(point_order, np.int64), np.arange(N, Np)])
    inv = np.empty(V + 1, np.int64)
    inv[np.asarray(vertex_order)] = np.arange(V)
    inv[V] = -1
    offset = inv[ref["offset"][perm]]
    bary = ref["bary"][perm].copy()
    nbr = inv[np.asarray(ref["nbr"], np.int64)[:, vertex_order, :]]
    # rows: the real entries of every vertex in ascending original point index
    e_pos, e_rem = np.divmod(np.arange(N * D1), D1)
    e_id = offset[:N].reshape(-1)
    order = np.lexsort((perm[e_pos], e_id))
    counts = np.bincount(e_id, minlength=V)
    rowptr = np.concatenate([[0], np.cumsum(counts)])
    fastn = (nbr[0, :, 1] == np.arange(V) + 1).astype(np.uint8)
    return dict(d=d, N=N, V=V, perm=perm.astype(np.int32), offset=offset.astype(np.int32), bary=bary, rowptr=rowptr.astype(np.int32),
                csr_pt=e_pos[order].astype(np.int32), csr_w=bary[e_pos[order], e_rem[order]].copy(), nbr=nbr.astype(np.int32), fastn=fastn)


def row_major_order(ref):
    """The reference ids in row-major order of their grid coordinates (coordinate 0 fastest): the numbering of the sorted build."""
    c = grid_coords(ref["keys"])
    return np.lexsort(tuple(c[:, j] for j in range(c.shape[1])))

"""The float64 checker of tests/meanfield_f64.py with the barycentric weights as a FUNCTION of the features, for the tests of
lccrf_inference_backward_features (include/lccrf.h section 1d).

The topology is the oracle's and is held fixed (offset, nbr, V of pyoracle.OracleCRF.kernel(k); the simplex of a point from the
key of its remainder-0 corner; the ranks from the keys of its other corners, so that a point ON a float32 rank tie keeps the oracle's
side); inside it the weights are linear in the features
(permutohedral_cpu.h:304-366) and the norm 1 / (Phi(1) + 1e-20) is part of the graph.  torch.autograd through
meanfield_f64.forward with these lattices gives the reference dL/d features.  The file also holds the hand-written reverse sweep
the kernels implement (no autograd) and a small float64 lattice builder of its own, for the finite-difference test.
Not product code."""
import numpy as np
import torch

import meanfield_f64 as mf

D = torch.float64


def scale_factors(d):
    """permutohedral_cpu.h:282-285 as the library forms them (float32 values)."""
    inv_std_dev = np.float32(np.sqrt(2.0 / 3.0) * (d + 1))
    return np.array([np.float32(1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std_dev)) for i in range(d)], np.float32)


def elevate(f, scale):
    """el [N, d+1] of features f [N, d] (tensor): el_0 = sum_m cf_m, el_j = sum_{m >= j} cf_m - j cf_{j-1}"""
    d = f.shape[1]
    cf = f * scale
    cols = [cf.sum(1)] + [cf[:, j:].sum(1) - j * cf[:, j - 1] for j in range(1, d + 1)]
    return torch.stack(cols, 1)


def ranks_of(diff):
    """rank_i = how many coordinates of el - rem0 are larger, ties as permutohedral_cpu.h:326-336 breaks them (strict '<')"""
    N, D1 = diff.shape
    rank = np.zeros((N, D1), np.int64)
    for i in range(D1 - 1):
        for j in range(i + 1, D1):
            c = diff[:, i] < diff[:, j]
            rank[:, i] += c
            rank[:, j] += ~c
    return rank


def ranks_of_corners(keys, off, rem0):
    """The ranks of the ORACLE's simplex, read off its corners' keys: corner c has the key rem0_i + c where rank_i <= d - c, else
    rem0_i + c - (d + 1) (permutohedral_cpu.h:274-279,373), so coordinate i < d keeps the offset +c on d + 1 - rank_i of the d + 1
    corners; the ranks are a permutation, which gives the last one.  At an exact float32 rank tie the float64 order of el - rem0 is
    not the build's (ranks_of would pick the simplex across the boundary, whose one-sided derivative is another); rows whose keys
    wrapped int16 give no permutation here and are returned as -1."""
    N, D1 = off.shape
    d = D1 - 1
    cnt = np.zeros((N, d), np.int64)
    for c in range(D1):
        cnt += (keys[off[:, c]] - rem0[:, :d]) == c
    rank = np.concatenate([D1 - cnt, (d * D1 // 2 - (D1 - cnt).sum(1))[:, None]], 1)
    ok = (np.sort(rank, 1) == np.arange(D1)).all(1)
    rank[~ok] = -1
    return rank


def bary_of(f, scale, rem0, rank):
    """b [N, d+1] of features f [N, d] inside the simplex (rem0, rank): corner q receives +v of the coordinate with
    p = d - rank = q and -v of the one with p = q - 1 (cell d+1 folds into corner 0), v = (el - rem0) / (d+1)"""
    N, d = f.shape
    D1 = d + 1
    v = (elevate(f, torch.as_tensor(scale).to(f.dtype)) - torch.as_tensor(rem0).to(f.dtype)) / D1
    p = torch.as_tensor(d - rank)
    bb = torch.zeros(N, D1 + 1, dtype=f.dtype).scatter_add(1, p, v).scatter_add(1, p + 1, -v)
    b = bb[:, :D1].clone()
    b[:, 0] = b[:, 0] + 1 + bb[:, D1]
    return b


def corner_keys(rem0, rank, c):
    """first d key coordinates of the corner with remainder c (permutohedral_cpu.h:274-279,373)"""
    D1 = rem0.shape[1]
    d = D1 - 1
    return (rem0 + np.where(rank <= d - c, c, c - D1))[:, :d]


class FeatureLattice(mf.Lattice):
    """meanfield_f64.Lattice whose bary and norm are functions of a feature tensor (bind())."""

    def __init__(self, kern, feat32):
        super().__init__(kern)
        self.feat32 = np.ascontiguousarray(feat32, np.float32)
        self.oracle_bary = np.asarray(kern["bary"], np.float64)
        self.scale = scale_factors(self.d)
        keys = np.asarray(kern["keys"], np.int64).reshape(self.V, self.d)
        off = np.asarray(kern["offset"], np.int64)
        r0 = keys[off[:, 0]] if len(off) else np.zeros((0, self.d), np.int64)
        self.rem0 = np.concatenate([r0, -r0.sum(1, keepdims=True)], 1)
        el = elevate(torch.as_tensor(self.feat32.astype(np.float64)), torch.as_tensor(self.scale.astype(np.float64))).numpy()
        self.el64 = el
        self.rank = ranks_of_corners(keys, off, self.rem0) if len(off) else np.zeros((0, self.d + 1), np.int64)
        lost = (self.rank < 0).any(1)                            # (wrapped keys: the order of el - rem0, tie-free there)
        self.rank[lost] = ranks_of(el - self.rem0)[lost]
        self.keys, self.off0 = keys, off
        # The oracle's weights are the linear form ROUNDED in float32 (v = (el - rem0) / (d+1) with |el| up to a few hundred: a few
        # 1e-6 of b).  The rounding does not move with the features, so it enters as a constant: at the case's own features the
        # checker's b is the oracle's bary to the last bit of float32 -- the weights the library's filters really use -- and its
        # derivative is the linear form's.
        f0 = torch.as_tensor(self.feat32.astype(np.float64))
        self.linear_bary = bary_of(f0, self.scale, self.rem0, self.rank).numpy()
        self.residual = torch.as_tensor(self.oracle_bary - self.linear_bary)
        self.bind(f0)

    def topology_agrees(self):
        """every corner's key, formed from (rem0, rank), is the key of the oracle's vertex for that corner; ranks a permutation"""
        ok = np.array_equal(np.sort(self.rank, 1), np.broadcast_to(np.arange(self.d + 1), self.rank.shape))
        for c in range(self.d + 1):
            ok = ok and np.array_equal(corner_keys(self.rem0, self.rank, c), self.keys[self.off0[:, c]])
        return bool(ok)

    def bind(self, f):
        self.bary = bary_of(f, self.scale, self.rem0, self.rank) + self.residual.to(f.dtype)
        ones = torch.ones(f.shape[0], 1, dtype=f.dtype)
        self.norm = 1.0 / (self.apply(ones)[:, 0] + 1e-20)
        return self

    def values(self, x, reverse=False):
        """the blurred vertex values before the slice: row v + 1 = (B S x)[v] (reverse: B^T S x), row 0 the absent vertex"""
        N, L = x.shape
        D1 = self.d + 1
        contrib = (self.bary.to(x.dtype)[:, :, None] * x[:, None, :]).reshape(N * D1, L)
        val = torch.zeros(self.V + 1, L, dtype=x.dtype).index_add(0, self.offset.reshape(-1), contrib)
        for j in (reversed(range(D1)) if reverse else range(D1)):
            val = torch.cat([val[:1] * 0, val[1:] + 0.5 * (val[self.n1[j]] + val[self.n2[j]])], 0)
        return val


def lattices(crf, pb):
    return [FeatureLattice(crf.kernel(k), f) for k, (f, _) in enumerate(pb["kernels"])]


def feature_gradients(U, w, lats, n_iterations, relax, G, dtype=D, feats=None, at=None):
    """(dL/dU, dL/dw, [dL/df_k]) of L = <G, Q_T> by autograd, the topology fixed, as float64 numpy arrays.  dtype=torch.float32
    runs the same computation in single precision.  feats: float64 features to evaluate at (default: the lattices' own)."""
    U = torch.as_tensor(np.asarray(U, np.float64)).to(dtype).clone().requires_grad_(True)
    w = torch.as_tensor(np.asarray(w, np.float64)).to(dtype).clone().requires_grad_(True)
    fs = []
    for k, lat in enumerate(lats):
        f = np.asarray(lat.feat32 if feats is None else feats[k], np.float64)
        fs.append(torch.as_tensor(f).to(dtype).clone().requires_grad_(True))
        lat.bind(fs[-1])
    Q = mf.forward(U, w, lats, n_iterations, relax, at)
    loss = (Q * torch.as_tensor(np.asarray(G, np.float64)).to(dtype)).sum()
    loss.backward()
    for lat in lats:                                             # leave the lattices bound to plain float64 features
        lat.bind(torch.as_tensor(lat.feat32.astype(np.float64)))
    zero = lambda t: np.zeros(tuple(t.shape))
    return (U.grad.double().numpy(), w.grad.double().numpy() if w.grad is not None else np.zeros(len(lats)),
            [f.grad.double().numpy() if f.grad is not None else zero(f) for f in fs], float(loss.detach()))


def corner_to_feature(gb, scale, rank):
    """step 4: dL/df [N, d] from dL/db [N, d+1] (numpy float64)"""
    N, D1 = gb.shape
    d = D1 - 1
    p = d - rank
    gv = np.take_along_axis(gb, p, 1) - np.take_along_axis(gb, (p + 1) % D1, 1)     # dL/dv_j
    gel = gv / D1
    gf = np.zeros((N, d))
    for m in range(d):
        gf[:, m] = (gel[:, 0] + gel[:, 1:m + 1].sum(1) - (m + 1) * gel[:, m + 1]) * float(scale[m])
    return gf


def sweep_feature_gradients(U, w, lats, n_iterations, relax, G):
    """The reverse sweep the kernels run (include/lccrf.h section 1d), float64, no autograd: [dL/df_k]."""
    with torch.no_grad():
        U = torch.as_tensor(np.asarray(U, np.float64))
        w = [float(x) for x in np.asarray(w, np.float64)]
        Gt = torch.as_tensor(np.asarray(G, np.float64))
        T, K = n_iterations, len(lats)
        hist = [torch.softmax(-U, 1)]
        for _ in range(T):
            Q = hist[-1]
            x = -U
            for k, lat in enumerate(lats):
                x = x + w[k] * lat.norm[:, None] * lat.apply(Q)
            P = torch.softmax(x, 1)
            hist.append(P if relax == 1.0 else (1.0 - relax) * Q + relax * P)
        gb = [torch.zeros(U.shape[0], lat.d + 1, dtype=D) for lat in lats]
        gn = [torch.zeros(U.shape[0], dtype=D) for lat in lats]
        for t in range(T, 0, -1):
            Q = hist[t - 1]
            res = [lat.values(Q) for lat in lats]                                     # (B S Q_{t-1}) of every term
            phi = [lat.alpha * (lat.bary[:, :, None] * r[lat.offset]).sum(1) for lat, r in zip(lats, res)]
            x = -U
            for k, lat in enumerate(lats):
                x = x + w[k] * lat.norm[:, None] * phi[k]
            P = torch.softmax(x, 1)
            gamma = relax * P * (Gt - (Gt * P).sum(1, keepdim=True))
            Gt = (1.0 - relax) * Gt
            for k, lat in enumerate(lats):
                y = lat.norm[:, None] * gamma
                gn[k] += w[k] * (gamma * phi[k]).sum(1)
                gb[k] += lat.alpha * w[k] * (y[:, None, :] * res[k][lat.offset]).sum(2)          # slice side
                rt = lat.values(y, reverse=True)
                gb[k] += lat.alpha * w[k] * (Q[:, None, :] * rt[lat.offset]).sum(2)              # splat side
                Gt = Gt + w[k] * lat.alpha * (lat.bary[:, :, None] * rt[lat.offset]).sum(1)
        out = []
        for k, lat in enumerate(lats):
            a = (-lat.norm * lat.norm * gn[k])[:, None]
            ones = torch.ones_like(a)
            gb[k] += lat.alpha * (a * lat.values(ones)[lat.offset][:, :, 0])
            gb[k] += lat.alpha * lat.values(a, reverse=True)[lat.offset][:, :, 0]
            out.append(corner_to_feature(gb[k].numpy(), lat.scale, lat.rank))
        return out


# ---- a float64 lattice builder of the file's own: the topology as a function of the features ------------------------------------
def build_kern(f):
    """The dictionary pyoracle.OracleCRF.kernel(k) returns (d, V, offset, nbr, keys; bary and norm are left to FeatureLattice),
    built in float64 from features f [N, d]: the enclosing simplex of every point (permutohedral_cpu.h:304-345), a vertex id per
    distinct key in order of first appearance, the blur neighbours by key (:663-679)."""
    f = np.asarray(f, np.float64)
    N, d = f.shape
    D1 = d + 1
    el = elevate(torch.as_tensor(f), torch.as_tensor(scale_factors(d).astype(np.float64))).numpy()
    v = np.rint(el / D1)
    rem0 = v * D1
    rank = ranks_of(el - rem0) + v.sum(1, keepdims=True).astype(np.int64)
    adj = (rank < 0) * D1 - (rank >= D1) * D1
    rank, rem0 = rank + adj, (rem0 + adj).astype(np.int64)
    ids, off = {}, np.zeros((N, D1), np.int64)
    for c in range(D1):
        kc = corner_keys(rem0, rank, c)
        for i in range(N):
            off[i, c] = ids.setdefault(tuple(kc[i]), len(ids))
    # (ids in order of first appearance over corners-then-points here; the oracle numbers point by point -- the same set)
    V = len(ids)
    keys = np.array(list(ids), np.int64).reshape(V, d)
    nbr = np.full((D1, V, 2), -1, np.int64)
    for vi, k in enumerate(map(tuple, keys)):
        for j in range(D1):
            a, b = [x - 1 for x in k], [x + 1 for x in k]
            if j < d:
                a[j], b[j] = k[j] + d, k[j] - d
            nbr[j, vi] = ids.get(tuple(a), -1), ids.get(tuple(b), -1)
    return dict(d=d, V=V, offset=off, nbr=nbr, keys=keys, bary=np.zeros((N, D1)), norm=np.zeros(N))


class BuiltLattice(FeatureLattice):
    """FeatureLattice over build_kern's topology at float64 features f (nothing of the oracle)."""

    def __init__(self, f):
        f = np.asarray(f, np.float64)
        kern = build_kern(f)
        mf.Lattice.__init__(self, kern)
        self.feat32 = f                                          # (float64 here: the point the lattice was built at)
        self.scale = scale_factors(self.d)
        keys, off = kern["keys"], kern["offset"]
        r0 = keys[off[:, 0]]
        self.rem0 = np.concatenate([r0, -r0.sum(1, keepdims=True)], 1)
        el = elevate(torch.as_tensor(f), torch.as_tensor(self.scale.astype(np.float64))).numpy()
        self.el64 = el
        self.rank = ranks_of_corners(keys, off, self.rem0) if len(off) else np.zeros((0, self.d + 1), np.int64)
        lost = (self.rank < 0).any(1)                            # (wrapped keys: the order of el - rem0, tie-free there)
        self.rank[lost] = ranks_of(el - self.rem0)[lost]
        self.keys, self.off0 = keys, off
        self.residual = torch.zeros(f.shape[0], self.d + 1, dtype=D)
        self.bind(torch.as_tensor(f))


def rebuilt_loss(U, w, feats, n_iterations, relax, G):
    """L = <G, Q_T> with every lattice REBUILT at float64 features feats[k]"""
    lats = [BuiltLattice(f) for f in feats]
    Q = mf.forward(torch.as_tensor(np.asarray(U, np.float64)), torch.as_tensor(np.asarray(w, np.float64)), lats, n_iterations, relax)
    return float((Q * torch.as_tensor(np.asarray(G, np.float64))).sum())

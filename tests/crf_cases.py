"""Helpers shared by the parity tests: fixture decoding and a backend-agnostic runner.

A "backend" is any class with the reference's operator surface on numpy arrays
(oracle.pyoracle.OracleCRF / RefCRF, or the HIP mirror DenseCRFHIP):
  cls(N, L); set_unary | set_unary_from_label; add_pairwise(features, w);
  start_inference(); step_inference(relax); build_map(); probability(); map(); kernel(k)
"""
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTR_LIB = os.path.join(ROOT, "lc-crf-slam_amd", "liblccrf_hip_instr.so")


def switch_env(env=None, **more):
    """Environment for a child process that sets A/B / cross-check switches: they exist in the INSTRUMENTED library only
    (csrc/engine.h: ab_env), so a non-empty set of switches also selects that library through LCCRF_LIB."""
    sw = dict(env or {}, **more)
    out = dict(os.environ, **sw)
    if sw:
        out["LCCRF_LIB"] = INSTR_LIB
    return out


def bits(a):
    """Bit pattern view, so float comparisons are bit-exact (and NaN-safe)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def case_problem(z, prefix):
    """Decode one fixture case (tests/golden/make_golden.py: pack())."""
    p = prefix + "_"
    pb = dict(N=int(z[p + "N"]), L=int(z[p + "L"]))
    K = int(z[p + "K"])
    if p + "unary" in z.files:
        pb["unary"] = z[p + "unary"]
    else:
        pb["label"] = z[p + "label"]
        pb["conf"] = np.float32(z[p + "conf"])
    pb["kernels"] = [(z[p + "feat%d" % k], np.float32(z[p + "w%d" % k])) for k in range(K)]
    return pb


def case_expected(z, prefix):
    p = prefix + "_"
    exp = dict(V=[], norm=[], Q={}, map={})
    K = int(z[p + "K"])
    for k in range(K):
        exp["V"].append(int(z[p + "V%d" % k]))
        exp["norm"].append(z[p + "norm%d" % k])
    for name in z.files:
        if name.startswith(p + "Q"):
            exp["Q"][int(name[len(p) + 1:])] = z[name]
        if name.startswith(p + "map"):
            exp["map"][int(name[len(p) + 3:])] = z[name]
    exp["relax"] = float(z[p + "relax"]) if p + "relax" in z.files else 1.0
    return exp


def setup(cls, pb, **kw):
    c = cls(pb["N"], pb["L"], **kw)
    if "unary" in pb:
        c.set_unary(pb["unary"])
    else:
        c.set_unary_from_label(pb["label"], pb["conf"])
    for f, w in pb["kernels"]:
        c.add_pairwise(f, w)
    return c


def check_against_expected(c, exp, q_tol=None):
    """Step a prepared CRF and compare with the reference's recorded outputs.

    q_tol=None  -> Q must be bit-identical;  q_tol=x -> max|dQ| <= x.
    Labels and lattice sizes must always be identical.
    """
    for k, V in enumerate(exp["V"]):
        kv = c.kernel(k)
        assert kv["V"] == V, "kernel %d: V=%d, reference M_=%d" % (k, kv["V"], V)
        if q_tol is None:
            assert same_bits(kv["norm"], exp["norm"][k]), "kernel %d: norm differs" % k
        else:
            np.testing.assert_allclose(kv["norm"], exp["norm"][k], rtol=1e-5, atol=0)
    iters = sorted(exp["Q"])
    c.start_inference()
    for t in range(max(iters) + 1):
        if t:
            c.step_inference(exp["relax"])
        if t in exp["Q"]:
            q = c.probability()
            if q_tol is None:
                assert same_bits(q, exp["Q"][t]), "Q differs after %d iterations (max %g)" % (
                    t, np.abs(q - exp["Q"][t]).max() if q.size else 0.0)
            else:
                assert q.shape == exp["Q"][t].shape
                if q.size:
                    assert np.abs(q - exp["Q"][t]).max() <= q_tol
            c.build_map()
            assert np.array_equal(c.map(), exp["map"][t]), "labels differ after %d iterations" % t


def label_problem(N, L, dims, seed, label=False, spread=3.0):
    """A generic frame for any label count (tests/golden/make_golden_labels.py, tests/test_labels.py): terms of the given feature
    dimensions, with points on lattice-cell boundaries; raw unaries whose first and last columns are equal (Q's columns 0 and L-1
    then stay equal bit for bit: exact ties for the argmax, taken on about half of the rows) or, with label=True, labels in
    [-1, L) with one confidence.  The weights sum to about 6.5 whatever the number of terms, so that even eight terms leave most
    rows unsaturated."""
    rng = np.random.default_rng([int(seed), int(N), int(L)] + [int(d) for d in dims])
    kernels = []
    for d in dims:
        f = rng.normal(0.0, spread, (N, d)).astype(np.float32)
        q = rng.random(N) < 0.5
        f[q] = np.round(f[q] * 2) / 2
        f[rng.random(N) < 0.1] = 0.0
        kernels.append((f, np.float32(rng.uniform(1.0, 12.0) / len(dims))))
    pb = dict(N=N, L=L, kernels=kernels)
    if label:
        assert L >= 2, "setUnaryEnergyFromLabel divides by L - 1"
        pb["label"] = rng.integers(-1, L, N).astype(np.int16)
        pb["conf"] = np.float32(rng.uniform(0.4, 0.8))
    else:
        u = (np.round(rng.uniform(0.05, 3.0, (N, L)) * 256) / 256).astype(np.float32)
        low = rng.random(N) < 0.5
        u[low, 0] = u[low].min(1) - np.float32(0.5)
        u[:, L - 1] = u[:, 0]
        pb["unary"] = u
    return pb


def shaped_problem(wl, N, shape, seed):
    """SLAM-shaped frames whose lattices stress one code path of the fused engine each."""
    pb = wl.slam_problem(N, seed=seed)
    rng = np.random.default_rng(seed)
    f0, f1 = pb["kernels"][0][0].copy(), pb["kernels"][1][0].copy()
    if shape == "one_cell":            # every point in one lattice cell: 3 vertices, rows of N products
        f0[:] = f0[0]
        f1[:] = f1[0]
    elif shape == "two_clusters":      # two very long rows per kernel plus stragglers
        half = N // 2
        f0[:half], f0[half:] = f0[0], f0[-1] + np.float32(7.5)
        f0[::97] += rng.normal(0, 3, f0[::97].shape).astype(np.float32)
    elif shape == "rows_of_8":         # row lengths around the 8-product units of chain_rows
        cells = max(N // 8, 1)
        f0 = (np.stack([np.arange(N) % cells, np.arange(N) % cells], 1) * np.float32(4.0)).astype(np.float32)
    elif shape == "sparse":            # every point its own cell: V = 3N, far beyond the chain's vertex limit
        f0 = (np.stack([np.arange(N), (np.arange(N) * 7) % 1013], 1) * np.float32(9.0)).astype(np.float32)
    pb["kernels"] = [(f0, pb["kernels"][0][1]), (f1, pb["kernels"][1][1])]
    return pb


def large_case(z, name):
    """(problem, iterations, relax) of one case of tests/golden/large.npz"""
    pb = dict(N=int(z[name + "_features"].shape[0]), L=int(z[name + "_Q"].shape[1]),
              kernels=[(z[name + "_features"], np.float32(z[name + "_w"]))])
    if name + "_unary" in z.files:
        pb["unary"] = z[name + "_unary"]
    else:
        pb["label"], pb["conf"] = z[name + "_label"], np.float32(z[name + "_conf"])
    return pb, int(z[name + "_iters"]), float(z[name + "_relax"])


def golden_problem(golden, name):
    group, case = name.split(":")
    if group == "labels":                                       # (not among conftest's fixtures)
        return case_problem(np.load(os.path.join(os.path.dirname(__file__), "golden", "labels.npz")), case)
    z = golden[group]
    if group == "large":
        pb, _, _ = large_case(z, case)
        return pb
    return case_problem(z, case)


def crop_problem(golden, po, x0=0, y0=0):
    """64 x 48 crop of the reference's image example (the window at pixel (x0, y0)): 21 labels, the position and RGB image terms."""
    z = golden["example_im1"]
    W, H = 64, 48
    im = np.ascontiguousarray(z["im"][y0:y0 + H, x0:x0 + W], np.uint8)
    lab = np.ascontiguousarray(z["label"].reshape(240, 320)[y0:y0 + H, x0:x0 + W].reshape(-1), np.int16)
    pb = dict(N=W * H, L=21, label=lab, conf=np.float32(0.5),
              kernels=[(po.oracle_image_features(W, H, 3.0), np.float32(3.0)),
                       (po.oracle_image_features(W, H, 60.0, im, 20.0), np.float32(10.0))])
    return pb, (W, H, im)


# the cases of test_gradients_match_the_checker (tests/test_meanfield_backward.py)
CASES = ["slam:N5", "slam:N1001", "slam:C3", "generic:d1_L3", "generic:d3_L21", "generic:d5_L2", "generic:d6_L3", "generic:multi",
         "bilateral:c5", "large:c5", "image64x48", "c2"]


def case(name, golden, po, wl):
    """(problem, image or None)"""
    if name == "image64x48":
        return crop_problem(golden, po)
    if name.startswith("K8_L"):                                  # eight terms of d = 1 .. 8
        return label_problem(900, int(name[4:]), list(range(1, 9)), seed=6), None
    if name == "c2":
        return wl.slam_problem(2000, seed=12), None
    return golden_problem(golden, name), None


# The gradient tests' stand-ins for cases whose float32 checker is too far from float64 for a bar to mean anything, or on which a
# planted fault stays inside the bars (tests/test_gradient_bars.py, notes/gradient_bars.md): the same generator, point count,
# dimensions, label count and ties under another seed.  name -> f(golden, po, wl) -> (problem, image or None).  The fixtures of these
# names stay in every forward, bits, determinism and state test (case()).
GRADIENT_TWINS = {
    "generic:d5_L2": lambda golden, po, wl: (wl.generic_problem(257, [5], 2, seed=2, lattice_ties=True), None),
    "generic:multi": lambda golden, po, wl: (wl.generic_problem(301, [2, 5, 3], 4, seed=14), None),
    "slam:N1001": lambda golden, po, wl: (wl.slam_problem(1001, seed=16), None),
    "slam:C3": lambda golden, po, wl: (wl.slam_problem(2000, seed=16, obs_cap=10), None),
    "c2": lambda golden, po, wl: (wl.slam_problem(2000, seed=16), None),
    "bilateral:c5": lambda golden, po, wl: (wl.bilateral_problem(4096, seed=17), None),
    "nt:d4_L5": lambda golden, po, wl: (wl.generic_problem(257, [4], 5, seed=35, spread=1.5), None),
    "nt:d7_L2": lambda golden, po, wl: (wl.generic_problem(257, [7], 2, seed=27, spread=1.5), None),
    "image64x48": lambda golden, po, wl: crop_problem(golden, po, 64, 80),     # the window at pixel (64, 80) of example_im1
}


def gradient_case(name, golden, po, wl):
    """(problem, image or None) of a case of the gradient lists: its twin where it has one, else case()"""
    twin = GRADIENT_TWINS.get(name)
    return twin(golden, po, wl) if twin else case(name, golden, po, wl)


def batch_of(pbs, maxN=None, use_unary=False):
    """two-label SLAM frames as one BatchCRF with its inputs set"""
    pkg = importlib.import_module("lc-crf-slam_amd")
    F = len(pbs)
    maxN = maxN or max(max(pb["N"] for pb in pbs), 1)
    K = len(pbs[0]["kernels"])
    feats = [np.zeros((F, maxN, 2), np.float32) for _ in range(K)]
    label = np.full((F, maxN), -1, np.int16)
    unary = np.zeros((F, maxN, 2), np.float32)
    for f, pb in enumerate(pbs):
        n = pb["N"]
        if "label" in pb:
            label[f, :n] = pb["label"]
        if "unary" in pb:
            unary[f, :n] = pb["unary"]
        for k in range(K):
            feats[k][f, :n] = pb["kernels"][k][0]
    b = pkg.BatchCRF(F, maxN, 2, [2] * K, [float(pbs[0]["kernels"][k][1]) for k in range(K)])
    if use_unary:
        b.set_inputs_host([pb["N"] for pb in pbs], feats, unary=unary)
    else:
        b.set_inputs_host([pb["N"] for pb in pbs], feats, label=label, conf=pbs[0].get("conf", 0.7))
    return b


def raw_unary(pb):
    """raw unary energies [N][L] of a problem (from its labels by the formula of densecrf3d.h:109-129 where it has no raw ones)"""
    if "unary" in pb:
        return np.ascontiguousarray(pb["unary"], np.float32).reshape(pb["N"], pb["L"])
    N, L, c = pb["N"], pb["L"], np.float32(pb["conf"])
    lab = np.asarray(pb["label"], np.int64)
    U = np.full((N, L), -np.log((np.float32(1) - c) / np.float32(L - 1)), np.float32)
    has = lab >= 0
    U[np.nonzero(has)[0], lab[has]] = -np.log(c)
    U[~has] = -np.log(np.float32(1.0) / np.float32(L))
    return U


def empty_problem(L, dims):
    return dict(N=0, L=L, unary=np.zeros((0, L), np.float32), kernels=[(np.zeros((0, d), np.float32), 1.0) for d in dims])

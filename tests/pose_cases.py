"""The scenes the pose-optimisation kernel (csrc/pose_opt.hip) is held to the restatement on (oracle/lccrf_oracle.c:
orc_pose_optimization), by shape class.  tests/test_pose_cases.py, which needs no GPU, checks the list before the GPU tests
(tests/test_pose_optimization.py) rely on it: that over the list the restatement takes every branch of its schedule
(pyoracle.POSE_TRACE), and that on each scene the restatement itself does not care in which order the edges are summed -- it sums
them in index order, the kernel in a tree over lanes, so only such a scene can be compared flag for flag.  A scene that fails that
is replaced in TWINS by the same shape under another seed; none is dropped.

The classes (notes/pose_tests.md has the branch counts of every scene):
  unstaged   more than 4096 keypoints: k_pose_opt<false>, edges read from global memory in every sweep, up to the 16384 cap
  staged     the thresholds of the schedule (n_init < 3, < 10) and of compact_level0's four chunks rounded to 64 lanes
  few        many points of which 2 .. 11 are valid: n_init apart from n, and chunks of compact_level0 without a level-0 edge
  far        initial poses 0.8 .. 3.1 rad from the truth: the quaternion of a matrix of trace <= 0 (three cases), a 6x6 system that
             is not positive definite, rho == 0 stops, rounds of ten iterations
  behind     map points behind the camera: edges flagged after one round and re-admitted after a later one
  nonfinite  a keypoint at infinity: an LM trial whose chi2 is not finite although its system could be solved"""
import importlib

import numpy as np

# Copies of csrc/pose_opt.hip's kWaves (= kPT / 64) and kStageMax: they decide which scenes sit on a boundary and must follow the kernel
WAVES, STAGE_MAX = 4, 4096


def rot(axis, angle):
    """the rotation by `angle` (rad) about `axis` (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def with_init(scene, axis, angle, dt):
    """the scene started from rot(axis, angle) . R_true and t_true + dt"""
    T0 = np.eye(4)
    T0[:3, :3] = rot(axis, angle) @ scene["T_true"][:3, :3]
    T0[:3, 3] = scene["T_true"][:3, 3] + dt
    return dict(scene, T_init=T0.astype(np.float32))


def scattered(n, k):
    """k indices over the whole of [0, n), both ends included"""
    return np.unique(np.round(np.linspace(0, n - 1, k)).astype(np.int64))


def chunks_without_an_edge(n, valid):
    """how many of compact_level0's per-wavefront chunks hold points but no edge (staged frames only)"""
    chunk = (n + WAVES * 64 - 1) // (WAVES * 64) * 64
    return sum(1 for w in range(WAVES) if min(n, w * chunk) < min(n, (w + 1) * chunk) and not valid[w * chunk:(w + 1) * chunk].any())


UNSTAGED = [4097, 5000, 8191, 16384]
STAGED = [3, 4, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095]
FEW_N, FEW_VALID = [700, 5000], [2, 3, 9, 10, 11]
FAR_N, FAR_SEED = [500, 5000], 5
FAR = [(0.8, (1, 1, 0), 0.5), (1.5, (0, 0, 1), 0.2), (2.5, (0, 1, 0), 1.0), (3.1, (1, 0, 0), 0.0), (3.1, (0, 1, 0), 0.0),
       (3.1, (0, 0, 1), 0.0)]                                     # angle (rad), axis, dt
BEHIND_N, BEHIND_SEED, BEHIND = 600, 8, [5, 50]                   # per cent of the points, from index 0, with Xw z negated

# name -> seed, where a scene's own seed leaves the restatement's answer dependent on the order of its sums (none so far:
# notes/pose_tests.md, reordering spread)
TWINS = {}


def _few(wl, n, k, seed):
    s = wl.pose_scene(n, seed=seed)
    on = scattered(n, k)
    s["valid"][:] = 0
    s["valid"][on] = 1
    if k >= 10:                                                   # a gross outlier among the valid ones, as in
        s["kp"][on[k // 2]] += 40.0                               # test_oracle_fewer_than_ten_edges_run_one_round
    return s


def _behind(wl, pct, seed):
    s = wl.pose_scene(BEHIND_N, seed=seed)
    s["Xw"][:BEHIND_N * pct // 100, 2] *= -1.0
    return s


def _nonfinite(wl, seed):
    s = wl.pose_scene(300, seed=seed, outlier_frac=0.0)
    s["kp"][150, 0] = np.inf
    return s


def _build():
    c = {}
    for n in UNSTAGED:
        c["unstaged:%d" % n] = lambda wl, seed, n=n: wl.pose_scene(n, seed=seed, n_invalid=n // 7), n + 1
    c["unstaged:4097:all_valid"] = lambda wl, seed: wl.pose_scene(4097, seed=seed), 4098
    for n in STAGED:
        c["staged:%d" % n] = lambda wl, seed, n=n: wl.pose_scene(n, seed=seed), n + 1
    for n in FEW_N:
        for k in FEW_VALID:
            c["few:%d:valid%d" % (n, k)] = lambda wl, seed, n=n, k=k: _few(wl, n, k, seed), n + 1
    for n in FAR_N:
        for angle, axis, dt in FAR:
            c["far:%d:%g:%d%d%d:dt%g" % ((n, angle) + axis + (dt,))] = \
                lambda wl, seed, n=n, angle=angle, axis=axis, dt=dt: with_init(wl.pose_scene(n, seed=seed), axis, angle, dt), FAR_SEED
    for pct in BEHIND:
        c["behind:%d:%dpct" % (BEHIND_N, pct)] = lambda wl, seed, pct=pct: _behind(wl, pct, seed), BEHIND_SEED
    c["nonfinite:300:kp_inf"] = _nonfinite, 301
    return c


_CASES = _build()
NAMES = list(_CASES)
FAR_NAMES = [n for n in NAMES if n.startswith("far:")]
CLASSES = ("unstaged", "staged", "few", "far", "behind", "nonfinite")
_SCENES, _ORACLE = {}, {}


def scene(name):
    """the scene of a name: built once, shared by the tests, never changed"""
    if name not in _SCENES:
        wl = importlib.import_module("lc-crf-slam_amd.workloads")
        make, seed = _CASES[name]
        s = make(wl, TWINS.get(name, seed))
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SCENES[name] = s
    return _SCENES[name]


def run_oracle(po, s, valid=None, trace=False):
    return po.oracle_pose_optimization(s["Xw"], s["kp"], s["u_right"], s["inv_sigma2"], s["valid"] if valid is None else valid,
                                       s["K4"], s["bf"], s["T_init"], trace=trace)


def oracle(po, name):
    """(Tcw, outlier, n_inliers, n_initial, branch counts) of the restatement on a scene: computed once"""
    if name not in _ORACLE:
        _ORACLE[name] = run_oracle(po, scene(name), trace=True)
    return _ORACLE[name]


def reordered(s, perm):
    """the scene with its points in the order perm"""
    return dict(s, **{k: s[k][perm] for k in ("Xw", "kp", "u_right", "inv_sigma2", "valid")})


def reorderings(name, n):
    """the three orders a scene must not care about: reversed, and two seeded permutations"""
    rng = np.random.default_rng([len(name), n, 4242])
    return [("reversed", np.arange(n)[::-1].copy()), ("perm1", rng.permutation(n)), ("perm2", rng.permutation(n))]


def pose_distance(Ta, Tb):
    """(ulps, absolute difference) of two float32 poses, the worst entry of each"""
    Ta, Tb = np.ascontiguousarray(Ta, np.float32), np.ascontiguousarray(Tb, np.float32)
    ulp = np.abs(Ta.view(np.int32).astype(np.int64) - Tb.view(np.int32).astype(np.int64))
    return int(ulp.max()), float(np.abs(Ta - Tb).max())


def pose_within_bar(Ta, Tb):
    """the bar of test_hip_pose_optimization_matches_the_restatement: 2 ulp, or 1e-7 absolute"""
    ulp, dist = pose_distance(Ta, Tb)
    return ulp <= 2 or dist < 1e-7

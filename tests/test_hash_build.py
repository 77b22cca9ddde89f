"""The three hash lattice builds on the device where seeded random frames never take them (tests/hash_build_cases.py, which
tests/test_hash_build_cases.py proves without a GPU; notes/hash_build_tests.md): probe chains hundreds of slots long, chains over the
end of the table, nearly full and overfull tables, both sides of every capacity step, the reserved key as a vertex and as a
neighbour query, a chain in one frame's HBM table next to the following frame's.

  * the frame body (csrc/frame_body.inc): every d = 2 case through lccrf_batch_run with one term and with two (two workgroups per
    frame, and one), the cases of up to 512 points in the 512-lane shape, every case through the object API; two cases through the
    converged form, the general form with matrices, and both together;
  * k_build_small (d = 1, 2, 3) through lccrf_batch_build and the lattice probe, then lccrf_batch_inference;
  * the streaming hash build (d = 5, 8; d = 2 beyond 4096 points) on engine 1.
Every comparison is bit for bit against the oracle: V, offset, bary, nbr and norm where a probe exposes them, Q after 3 iterations,
the labels, the label bits.  A case meant to fit must report no fallback frame: one that silently took the other path proves nothing.
"""
import importlib

import numpy as np
import pytest

import compat_checker as ck
import converge_cases as cv
import crf_cases as cc
import frame_lean_cases as fc
import hash_build_cases as hb
import normalization_checker as nc
import sorted_build_checker as sc
import test_fused_general as fg

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

F32 = np.float32
T, RELAX = hb.T, hb.RELAX
HALF_LDS = hb.FRAME_LDS // 2
_REFS = {}


def _reference(po, key, pb):
    """the oracle's results of one problem, computed once and shared, read-only: dict(N, Q, map, V, kernels)"""
    if key not in _REFS:
        o = cc.setup(po.OracleCRF, pb)
        ks = [o.kernel(k) for k in range(len(pb["kernels"]))]
        o.inference_native(T, True, RELAX)
        r = dict(N=pb["N"], Q=o.probability().copy(), map=o.map().copy(), V=[int(k["V"]) for k in ks], kernels=ks)
        o.close()
        for a in (r["Q"], r["map"]):
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _case(po, name, where):
    pb = hb.frame_problem(po, name, where)
    return pb, _reference(po, (name, where), pb)


def _neighbour(po, N, K):
    pb = hb.neighbour_problem(N)
    if K == 1:
        pb = dict(pb, kernels=pb["kernels"][1:])
    return pb, _reference(po, ("neighbour", N, K), pb)


def _download(b):
    b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
    return dict(Q=b.probability(), map=b.map(), bits=b.wait_download()["bits"], V=[b.lattice_sizes(k) for k in range(len(b.dims))])


def _run(frames, single_workgroup=False):
    """frames: [(problem, reference)] -> the batch after lccrf_batch_run, every frame compared with its reference"""
    b = cc.batch_of([pb for pb, _ in frames])
    if single_workgroup:
        b.set_option(pkg.OPT_SINGLE_WORKGROUP, 1)
    b.run(T, True, relax=RELAX)
    fc.compare_batch(_download(b), [r for _, r in frames], list(range(len(frames))))
    return b


# ---- the frame body: lccrf_batch_run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hb.FRAME_CASES))
def test_frame_body_in_small_batches(po, name):
    """k_frame<1024, points per lane, K> for K = 1 and K = 2, and the two-workgroup form (a batch of up to 64 two-term frames): the case
    twice -- on either term where there are two -- and an ordinary frame of the same size, so that the launch takes the case's capacity"""
    route = hb.FRAME_CASES[name][0]
    N = hb.frame_case(po, name)[0].shape[0]
    one = [_case(po, name, "alone"), _neighbour(po, N, 1), _case(po, name, "alone")]
    two = [_case(po, name, 1), _case(po, name, 0), _neighbour(po, N, 2)]
    for frames, single in ((one, False), (two, False), (two, True)):
        b = _run(frames, single)
        tag = (name, len(frames[0][0]["kernels"]), single, b.engine(), b.fused_shape(), b.fallback_frames())
        print(tag)
        assert b.engine() == 3 and b.fused_shape() == (1024, 1), tag
        if route == "fit":
            assert b.fallback_frames() == 0, tag
        elif route == "fallback":
            assert b.fallback_frames() == 2, tag                         # exactly the case's two frames, never the ordinary one
        else:
            assert b.fallback_frames() in (0, 2), tag
        b.close()


def _tiled(po, names, NA, F=256, ordinary=1):
    cases = [_case(po, n, "alone") for n in names] + [_neighbour(po, NA, 1)] * ordinary
    return [cases[f % len(cases)] for f in range(F)], len(cases)


@pytest.mark.parametrize("names,NA", [(("wrap_1024", "nearly_full_1024", "hcap_step_340", "shared_cells"), 340), (("hcap_step_344",), 344)])
def test_frame_body_in_the_512_lane_shape(po, names, NA):
    """k_frame<512, 1, 1>: 256 one-term frames of up to 512 points, two per CU in half the LDS each (two-term batches of that many frames
    are the table-free kernel's).  The model says these cases fit half the LDS: none may leave for the fallback."""
    for n in names:
        f, ref, tb = hb.frame_case(po, n)
        rows = int(np.bincount(ref["offset"][:f.shape[0]].ravel(), minlength=ref["V"]).max())
        assert tb.cap == hb.frame_hcap(NA) and hb.frame_plan_fits(f.shape[0], [ref["V"]], rows, tb.cap, lds=HALF_LDS), n
    frames, _ = _tiled(po, names, NA)
    b = _run(frames)
    assert b.engine() == 3 and b.fused_shape() == (512, 2) and b.fallback_frames() == 0, (b.engine(), b.fused_shape(), b.fallback_frames())
    b.close()


def test_reserved_key_in_the_512_lane_shape(po):
    frames, per = _tiled(po, ("reserved_vertex", "reserved_neighbour"), 300, ordinary=6)
    copies = 256 // per                                                  # 32 frames of either case among 192 ordinary ones
    b = _run(frames)
    print("reserved, 512 lanes:", b.fallback_frames(), "of", copies, "+", copies)
    assert b.engine() == 3 and b.fused_shape() == (512, 2) and b.fallback_frames() in (copies, 2 * copies), b.fallback_frames()
    b.close()


# ---- the frame body: the object API (two workgroups for one frame) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hb.FRAME_CASES))
def test_frame_body_through_the_object_api(po, name):
    route = hb.FRAME_CASES[name][0]
    for where in (1, 0):
        pb, ref = _case(po, name, where)
        h = cc.setup(pkg.DenseCRFHIP, pb)
        h.inference(T, True, RELAX)
        assert np.array_equal(h.map(), ref["map"]), (name, where)
        assert cc.same_bits(h.probability(), ref["Q"]), (name, where)
        eng = h.engine()[0]
        print(name, where, "engine", eng)
        assert route == "any" or (eng == 3) == (route == "fit"), (name, where, eng)
        # the probes build the lattices in HBM (k_build_small, or the streaming build beyond its range): the oracle's numbering, verbatim
        for k in range(2):
            ko, kh = ref["kernels"][k], h.kernel(k)
            assert ko["V"] == kh["V"], (name, where, k)
            for what in ("offset", "bary", "nbr", "norm"):
                assert cc.same_bits(ko[what], kh[what]), (name, where, k, what)
        h.close()


# ---- the other kernels on the frame body ------------------------------------------------------------------------------------------------------
CRIT, TOL, CAP = cv.BOTH, F32(1e-3), 8


def _check_converged(b, traces, tag):
    q, m, rep = b.probability(), b.map(), b.convergence()
    for f, tr in enumerate(traces):
        want = cv.expect(tr, CRIT, TOL, CAP)
        n = tr[0].shape[0]
        assert cv.same_report({k: v[f] for k, v in rep.items()}, want), (tag, f, {k: v[f] for k, v in rep.items()}, want)
        assert cc.same_bits(q[f, :n], tr[want[0]]) and np.array_equal(m[f, :n], ck.map_of(tr[want[0]])), (tag, f)


@pytest.mark.parametrize("name", ["wrap_1024", "wrap_2048"])
def test_the_converged_form_on_wrapped_tables(po, name):
    """k_frame_converge (one workgroup per frame): every frame stops where the oracle's trace says"""
    N = hb.frame_case(po, name)[0].shape[0]
    pbs = [hb.frame_problem(po, name, 1), hb.frame_problem(po, name, 0), hb.neighbour_problem(N)]
    traces = [cv.oracle_trace(po, pb, RELAX, CAP) for pb in pbs]
    b = cc.batch_of(pbs)
    b.run_converged(CAP, CRIT, TOL, True, RELAX)
    _check_converged(b, traces, name)
    assert b.engine() == 3 and b.fallback_frames() == 0, (b.engine(), b.fallback_frames())
    b.close()
    h = cc.setup(pkg.DenseCRFHIP, pbs[0])
    h.run_converged(CAP, CRIT, TOL, True, RELAX)
    want = cv.expect(traces[0], CRIT, TOL, CAP)
    assert np.array_equal(h.map(), ck.map_of(traces[0][want[0]])) and cv.same_report(h.convergence(), want) and h.engine()[0] == 3
    assert cc.same_bits(h.probability(), traces[0][want[0]])
    h.close()


@pytest.mark.parametrize("name", ["wrap_1024", "wrap_2048"])
def test_the_general_form_on_wrapped_tables(po, name):
    """k_frame_general and k_frame_general_converge (LCCRF_OPT_FRAME_GENERAL): a matrix on either term, against the float32
    restatement tests/test_frame_general.py compares those kernels with"""
    N = hb.frame_case(po, name)[0].shape[0]
    pbs = [hb.frame_problem(po, name, 1), hb.frame_problem(po, name, 0), hb.neighbour_problem(N)]
    w = [F32(x) for _, x in pbs[0]["kernels"]]
    mats, modes = fg._dense(2, 2), [nc.AFTER, nc.AFTER]
    U, traces = [], []
    for pb in pbs:
        o = cc.setup(po.OracleCRF, pb)
        U.append(o.unary())
        nrm = [o.kernel(k)["norm"] for k in range(2)]
        o.close()
        traces.append(nc.restate_trace_f32(U[-1], nc.feats(pb), w, mats, modes, CAP, RELAX, nrm))
    b = pkg.BatchCRF(len(pbs), N, 2, [2, 2], [float(x) for x in w])
    b.set_option(pkg.BatchCRF.OPT_FRAME_GENERAL, 1)
    for k, m in enumerate(mats):
        b.set_pairwise_compatibility(k, m)
    b.set_inputs_host([N] * len(pbs), [np.stack([pb["kernels"][k][0] for pb in pbs]) for k in range(2)], unary=np.stack(U))
    b.run(T, True, RELAX)
    q, m = b.probability(), b.map()
    for f, tr in enumerate(traces):
        assert cc.same_bits(q[f], tr[T]) and np.array_equal(m[f], ck.map_of(tr[T])), (name, f)
    assert b.engine() == 3 and b.fused_shape() == (1024, 1) and b.fallback_frames() == 0, (b.engine(), b.fused_shape(), b.fallback_frames())
    b.run_converged(CAP, CRIT, TOL, True, RELAX)
    _check_converged(b, traces, name)
    assert b.engine() == 3 and b.fallback_frames() == 0, (b.engine(), b.fallback_frames())
    b.close()


# ---- the tables of entry ids ----------------------------------------------------------------------------------------------------------------------
def _check_built(b, refs, tag):
    """the lattice probe of every frame against the oracle's lattice: the reference's numbering VERBATIM (first occurrence in entry
    order), the rows by the checker of the streaming build's tables, the norm"""
    sizes, norm = b.lattice_sizes(0), b.norm(0)
    for i, (ref, _, _, f, _) in enumerate(refs):
        n = f.shape[0]
        t = b.built_lattice(0, i)
        assert int(sizes[i]) == t["V"] == ref["V"], (tag, i, int(sizes[i]), t["V"], ref["V"])
        assert t["N"] == n and np.array_equal(t["perm"], np.arange(ref["offset"].shape[0])) and t["fastn"] is None, (tag, i)
        assert np.array_equal(t["offset"], ref["offset"]), (tag, i, "offset")
        assert cc.same_bits(t["bary"], ref["bary"]), (tag, i, "bary")
        assert np.array_equal(t["nbr"], ref["nbr"]), (tag, i, "nbr")
        sc.check(ref, t, False)
        assert cc.same_bits(norm[i, :n], ref["norm"]), (tag, i, "norm")


def _check_inference(b, refs, tag):
    b.inference(T, True, relax=RELAX)
    q, m = b.probability(), b.map()
    for i, (_, qo, mo, f, _) in enumerate(refs):
        n = f.shape[0]
        assert cc.same_bits(q[i, :n], qo) and np.array_equal(m[i, :n], mo), (tag, i)


def _entry_batch(d, max_points, refs):
    F = len(refs)
    feat, un = np.zeros((F, max_points, d), F32), np.zeros((F, max_points, 2), F32)
    for i, (_, _, _, f, u) in enumerate(refs):
        feat[i, :f.shape[0]], un[i, :f.shape[0]] = f, u
    b = pkg.BatchCRF(F, max_points, 2, [d], [1.0])
    return b, [f.shape[0] for _, _, _, f, _ in refs], feat, un


SMALL = ["small_%s_d%d" % (kind, d) for d in (1, 2, 3) for kind in ("wrap", "two_thirds")] + ["small_shared_cells_d2"]


@pytest.mark.parametrize("name", SMALL)
def test_one_workgroup_build_on_wrapped_and_two_thirds_full_tables(po, name):
    """k_build_small<D>: the LDS table of entry ids, atomicMin and first-occurrence numbering"""
    _, d, frames = next(c for c in hb.small_cases(po) if c[0] == name)
    refs = hb.table_reference(po, name, frames)
    NA = max(f.shape[0] for f in frames)
    assert hb.small_supported(NA, d)
    b, ns, feat, un = _entry_batch(d, NA, refs)
    b.set_inputs_host(ns, [feat], unary=un)
    b.build()
    assert b.locality_mode() == (False, False)
    assert all(not any(b.build_report(0, i).values()) for i in range(len(frames))), name     # (all 0: the one-workgroup build)
    _check_built(b, refs, name)
    _check_inference(b, refs, name)
    b.close()


STREAM = ["stream_two_frames_d5", "stream_two_frames_d8", "stream_two_frames_d2_4100"]


@pytest.mark.parametrize("name", STREAM)
def test_streaming_hash_build_with_a_chain_next_to_the_following_table(po, name):
    """k_insert / k_first_flag / find_vertex: one HBM table per frame at slot + f * cap; frame 0's cluster runs over the end of its own
    -- into frame 1's, were the mask wrong -- and frame 1's keys home in the first slots of its own; a ragged third frame"""
    _, d, max_points, frames = next(c for c in hb.stream_cases(po) if c[0] == name)
    refs = hb.table_reference(po, name, frames)
    b, ns, feat, un = _entry_batch(d, max_points, refs)
    b.set_engine(1)
    b.set_option(pkg.OPT_VERTEX_ORDER, 0)
    b.set_inputs_host(ns, [feat], unary=un)
    b.build()
    assert b.locality_mode() == (False, False)
    assert all(b.build_report(0, i)["sorted_build"] == 0 for i in range(len(frames))), name
    _check_built(b, refs, name)
    _check_inference(b, refs, name)
    assert b.engine() == 1, b.engine()
    b.close()

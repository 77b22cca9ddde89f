"""The label-code form of the two-frames-per-CU inference kernel (csrc/fused_lean_label.hip: k_fused_lean_lbl).  When a batch's unaries
come from labels, the third inference on unchanged lattices runs from prepared records AND from one code byte per point (0, 1, or 2
for unknown / out of range) plus three energy pairs, instead of the unary array.  Nothing may move by a bit: every batch is compared
with the same batch bound to the equivalent RAW unary array (which keeps k_fused_lean) and with the CPU checker, frame by frame.

Batches have 256 frames: the lean plan starts there (fused_loop.h: kSmallMinFrames); with the 64 of kPrepMinFrames a batch keeps the
1024-lane kernel and would never reach the kernel under test.  One batch per points-per-lane shape (2, 3, 4: the largest frame
decides), each with a frame that is no multiple of 64, an empty frame, a frame of unknowns only, and labels -1 and 7 sprinkled over
the others.  notes/r9_experiments.md.
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import crf_cases as cc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

F = 256
BATCHES = {2: (1024, [513, 1024, 700, 0]), 3: (1536, [1025, 1536, 1100, 0]), 4: (2048, [1537, 2000, 2048, 0, 1999])}
_BASE, _REFS = {}, {}


def _base(wl, ppt):
    """the distinct frames of a batch: labels -1 and an out-of-range 7 among the real ones, the last real frame all unknown"""
    if ppt not in _BASE:
        _, sizes = BATCHES[ppt]
        pbs = []
        for i, n in enumerate(sizes):
            pb = wl.slam_problem(n, seed=9300 + 10 * ppt + i)
            lab = np.array(pb["label"], np.int16)
            lab[3::11] = -1
            lab[5::13] = 7
            pb["label"] = lab
            pbs.append(pb)
        alone = dict(pbs[0], label=np.full(pbs[0]["N"], -1, np.int16))
        _BASE[ppt] = pbs + [alone]
    return _BASE[ppt]


def _pairs(conf):
    """the library's three energy pairs (label 0, label 1, unknown) for a confidence: read back from a three-point handle, so that
    the raw arrays below are built from the SAME table (host logf), whatever numpy's log rounds to"""
    h = pkg.DenseCRFHIP(3, 2)
    h.set_unary_from_label(np.array([0, 1, -1], np.int16), conf)
    u = h.unary().copy()
    h.close()
    return u


def _with_raw(pb, conf):
    lab = np.asarray(pb["label"], np.int64)
    code = np.where((lab < 0) | (lab > 1), 2, lab)
    q = {k: v for k, v in pb.items() if k != "label"}
    q["unary"] = np.ascontiguousarray(_pairs(conf)[code], np.float32).reshape(pb["N"], 2)
    return q


def _reference(po, ppt, i, pb, conf, n_iter, relax):
    """the CPU checker on one distinct frame (out-of-range labels as unknown: the library's rule); computed once, read-only"""
    key = (ppt, i, float(conf), n_iter, relax)
    if key not in _REFS:
        lab = np.array(pb["label"], np.int16)
        lab[(lab < 0) | (lab > 1)] = -1
        o = cc.setup(po.OracleCRF, dict(pb, label=lab, conf=np.float32(conf)))
        o.inference_native(n_iter, True, relax)
        r = (o.probability().copy(), o.map().copy())
        o.close()
        for a in r:
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _tiled(base):
    return [base[f % len(base)] for f in range(F)]


def _results(b, with_map=True):
    Q = b.probability()
    if not with_map:
        return dict(Q=Q)
    b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
    return dict(Q=Q, map=b.map(), bits=b.wait_download()["bits"])


def _same(r, w, tag):
    for k in w:
        assert cc.same_bits(r[k], w[k]), (tag, k)


def _against_checker(po, ppt, base, conf, r, n_iter, relax, tag):
    for i, pb in enumerate(base):
        n = pb["N"]
        wq, wm = _reference(po, ppt, i, pb, conf, n_iter, relax)
        for f in (i, i + len(base) * ((F - 1 - i) // len(base))):            # (its first and its last copy)
            assert cc.same_bits(r["Q"][f, :n], wq), (tag, f, n)
            if "map" in r:
                assert np.array_equal(r["map"][f, :n], wm), (tag, f, n)
                want = np.zeros(r["bits"].shape[1] * 64, np.uint8)
                want[:n] = wm
                assert np.array_equal(np.unpackbits(r["bits"][f].view(np.uint8), bitorder="little"), want), (tag, f, n)


def _three(b, n_iter=5, relax=1.0):
    """self-contained, prepare + run, run from the records: the third one's results"""
    runs0 = b.last_prepare()[1]
    for _ in range(3):
        b.inference(n_iter, True, relax=relax)
    assert b.engine() == 2 and b.fused_shape() == (512, 2), (b.engine(), b.fused_shape())
    assert b.last_prepare()[1] == runs0 + 1
    return _results(b)


@pytest.mark.parametrize("ppt", sorted(BATCHES))
def test_codes_give_the_bits_of_raw_unaries_and_of_the_checker(po, wl, ppt):
    """every points-per-lane shape; 0, 1, 2 and 5 iterations, relax 0.5, no map -- all from the records (the third inference on)"""
    maxN, _ = BATCHES[ppt]
    base = _base(wl, ppt)
    conf = base[0]["conf"]
    bl = cc.batch_of(_tiled(base), maxN=maxN)
    bu = cc.batch_of(_tiled([_with_raw(pb, conf) for pb in base]), maxN=maxN, use_unary=True)
    for b in (bl, bu):
        b.build()
    rl, ru = _three(bl), _three(bu)
    _same(rl, ru, ("raw", ppt, 5))
    _against_checker(po, ppt, base, conf, rl, 5, 1.0, ("checker", ppt, 5))
    for n_iter, relax, with_map in ((0, 1.0, True), (1, 1.0, True), (2, 1.0, True), (5, 0.5, True), (2, 0.5, True), (5, 1.0, False)):
        for b in (bl, bu):
            b.inference(n_iter, with_map, relax=relax)
        rl, ru = _results(bl, with_map), _results(bu, with_map)
        _same(rl, ru, ("raw", ppt, n_iter, relax, with_map))
        _against_checker(po, ppt, base, conf, rl, n_iter, relax, ("checker", ppt, n_iter, relax, with_map))
    assert bl.last_prepare()[1] == 1 and bu.last_prepare()[1] == 1
    bl.close()
    bu.close()


def test_equal_energies_tie_to_label_0(po, wl):
    """conf = 0.5: both energies of every pair are equal, Q0 is a tie everywhere and the map takes label 0"""
    ppt = 4
    maxN, _ = BATCHES[ppt]
    base = _base(wl, ppt)
    conf = np.float32(0.5)
    p = _pairs(conf)
    assert (p[:, 0] == p[:, 1]).all()
    bl = cc.batch_of(_tiled([dict(pb, conf=conf) for pb in base]), maxN=maxN)
    bu = cc.batch_of(_tiled([_with_raw(pb, conf) for pb in base]), maxN=maxN, use_unary=True)
    for b in (bl, bu):
        b.build()
    rl, ru = _three(bl), _three(bu)
    _same(rl, ru, "raw, conf 0.5")
    _against_checker(po, ppt, base, conf, rl, 5, 1.0, "checker, conf 0.5")
    for b in (bl, bu):
        b.inference(0, True)
    rl, ru = _results(bl), _results(bu)
    _same(rl, ru, "raw, conf 0.5, no iteration")
    for f, pb in enumerate(_tiled(base)[:len(base)]):
        assert (rl["Q"][f, :pb["N"]] == np.float32(0.5)).all() and not rl["map"][f, :pb["N"]].any() and not rl["bits"][f].any(), f
    bl.close()
    bu.close()


def _inputs(pbs, maxN):
    feats = [np.stack([np.pad(pb["kernels"][k][0], ((0, maxN - pb["N"]), (0, 0))) for pb in pbs]) for k in range(2)]
    label = np.stack([np.pad(pb["label"], (0, maxN - pb["N"]), constant_values=-1) for pb in pbs]).astype(np.int16)
    return [pb["N"] for pb in pbs], feats, label


def test_the_codes_follow_the_unaries(po, wl):
    """labels, raw unaries, labels again; another confidence on the same labels; other labels behind a build(): every step gives
    the bits of a fresh handle"""
    ppt = 4
    maxN, _ = BATCHES[ppt]
    base = _base(wl, ppt)
    conf = base[0]["conf"]
    pbs = _tiled(base)
    raws = _tiled([_with_raw(pb, np.float32(0.8)) for pb in base])
    other = _tiled([dict(pb, label=np.roll(pb["label"], 1)) for pb in base])

    def fresh(pbs, use_unary=False):
        b = cc.batch_of(pbs, maxN=maxN, use_unary=use_unary)
        b.build()
        r = _three(b)
        b.close()
        return r

    want_labels, want_raw = fresh(pbs), fresh(raws, True)
    want_conf, want_other = fresh([dict(pb, conf=np.float32(0.9)) for pb in pbs]), fresh(other)
    assert not cc.same_bits(want_labels["Q"], want_raw["Q"]) and not cc.same_bits(want_labels["Q"], want_conf["Q"])
    assert not cc.same_bits(want_labels["Q"], want_other["Q"])

    b = cc.batch_of(pbs, maxN=maxN)
    b.build()
    _same(_three(b), want_labels, "labels")
    n, feats, label = _inputs(pbs, maxN)
    unary = np.stack([np.pad(pb["unary"], ((0, maxN - pb["N"]), (0, 0))) for pb in raws]).astype(np.float32)
    b.set_inputs_host(n, feats, unary=unary)
    b.build()
    _same(_three(b), want_raw, "raw unaries behind labels")
    b.set_inputs_host(n, feats, label=label, conf=conf)
    b.build()
    _same(_three(b), want_labels, "labels again")
    b.set_inputs_host(n, feats, label=label, conf=0.9)          # (the same labels and features; the batch API refuses an inference
    b.build()                                                   #  on new inputs before lccrf_batch_build: there is no state without one)
    _same(_three(b), want_conf, "another confidence")
    n, feats, label = _inputs(other, maxN)
    b.set_inputs_host(n, feats, label=label, conf=conf)
    b.build()
    _same(_three(b), want_other, "other labels behind a build")
    b.close()


def test_one_launch_frame_kernel_matches_the_streaming_engine(wl):
    """k_frame_lean shares the loop's text (mean_field_lean, whose label-code form it does not take): run() against engine 1"""
    ppt = 4
    maxN, _ = BATCHES[ppt]
    pbs = _tiled(_base(wl, ppt))
    b = cc.batch_of(pbs, maxN=maxN)
    b.run(5, True)
    assert b.engine() == 3 and b.fused_shape() == (512, 2) and b.fallback_frames() == 0, (b.engine(), b.fused_shape())
    r = _results(b)
    b.close()
    s = cc.batch_of(pbs, maxN=maxN)
    s.set_engine(1)
    s.build()
    s.inference(5, True)
    assert s.engine() == 1
    _same(r, _results(s), "frame kernel against the streaming engine")
    s.close()


def test_switch_runs_both_routes_on_one_handle():
    """LCCRF_NO_LABEL_CODES (instrumented library, read at every launch): the same handle on k_fused_lean and on k_fused_lean_lbl,
    equal bits; the kernel trace of profiles/r9_fused_c2 shows which kernel a launch is"""
    code = r"""
import importlib, os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import crf_cases as cc
wl = importlib.import_module("lc-crf-slam_amd.workloads")
sizes = [1537, 2000, 2048, 0, 1999]
base = [wl.slam_problem(n, seed=9400 + i) for i, n in enumerate(sizes)]
for pb in base:
    pb["label"] = np.array(pb["label"], np.int16); pb["label"][3::11] = -1; pb["label"][5::13] = 7
b = cc.batch_of([base[f %% len(base)] for f in range(256)], maxN=2048)
b.build()
for n_iter, relax in ((5, 1.0), (2, 0.5)):
    got = []
    for off in (None, "1", None):
        os.environ.pop("LCCRF_NO_LABEL_CODES", None)
        if off:
            os.environ["LCCRF_NO_LABEL_CODES"] = off
        for _ in range(3):
            b.inference(n_iter, True, relax=relax)
        got.append((b.probability(), b.map()))
    assert b.fused_shape() == (512, 2) and b.last_prepare()[1] == 1
    for q, m in got[1:]:
        assert cc.same_bits(q, got[0][0]) and np.array_equal(m, got[0][1]), (n_iter, relax)
b.close()
print("ok")
""" % (cc.ROOT, os.path.join(cc.ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=cc.switch_env(LCCRF_LEAN_SHAPE="2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

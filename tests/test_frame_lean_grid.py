"""The table-free lattice build of the half-CU frame kernel (csrc/frame_build.h: grid_records / grid_build, launched by
csrc/frame_lean.hip for batches of >= 256 two-kernel frames) on the deterministic cases of tests/frame_lean_cases.py: negative and
straddling key ranges, clouds far from the origin with and without phantom points, the id map, the vertex limits and the int16 guard
from both sides, kernel 1 on the bitmap path and kernel 0 on the list path, ties, rows around the 8-padded lists' units, tiny frames.

Through BatchCRF.set_inputs_host + run(), F = 256 (the smallest batch the kernel takes), maxN = 2048, the distinct cases tiled.
EVERY frame is compared with the oracle (the reference's own headers for the guard_out cases, where they are built): Q bit for
bit, the MAP labels, the downloaded label bits (zeros beyond the frame included), both lattice sizes.  The fit batches must report
ZERO frames left to the fallback -- no case may pass by falling back -- and the flag batch exactly the predicted number.
Observed routes and the modelled lattices: notes/frame_lean_tests.md.
"""
import importlib

import numpy as np
import pytest

import crf_cases as cc
import frame_lean_cases as fc

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

F, MAXN = 256, 2048
_CASES, _REFS = {}, {}


def _cases(po, wl, top):
    """{name: (problem, route)} of a batch size, classified once"""
    if top not in _CASES:
        cs = fc.cases(wl, top) + (fc.plan_cases(wl) if top == 2048 else [])
        _CASES[top] = {name: (pb, fc.expected_route(pb, po)[0]) for name, pb in cs}
    return _CASES[top]


def _raw(pb, name):
    """the problem with raw unary energies instead of labels, some beyond fast_exp's cut-off"""
    rng = np.random.default_rng(fc.hash_name(name))
    pu = {k: v for k, v in pb.items() if k != "label"}
    pu["unary"] = rng.uniform(0.05, 3.0, (pb["N"], 2)).astype(np.float32)
    pu["unary"][::50] = np.float32([0.0, 45.0])
    return pu


def _reference(po, wl, top, name, n_iter=5, relax=1.0, raw=False):
    """computed once per (case, call) and shared; read-only"""
    key = (top, name, n_iter, relax, raw)
    if key not in _REFS:
        pb = _cases(po, wl, top)[name][0]
        cls = po.RefCRF if name.startswith("guard_out") and po.have_ref() else po.OracleCRF
        r = fc.reference(_raw(pb, name) if raw else pb, po, n_iter, relax, cls=cls)
        for a in (r["Q"], r["map"]):
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _download(b):
    b.download_async(pkg.BatchCRF.DOWNLOAD_LABEL_BITS)
    return dict(Q=b.probability(), map=b.map(), bits=b.wait_download()["bits"], V=[b.lattice_sizes(k) for k in range(2)])


def _batch(po, wl, top, names, raw=False):
    pbs = [_cases(po, wl, top)[n][0] for n in names]
    return cc.batch_of([_raw(pb, n) for pb, n in zip(pbs, names)] if raw else pbs, maxN=MAXN, use_unary=raw)


def _check(po, wl, top, b, names, n_iter=5, relax=1.0, raw=False):
    distinct = sorted(set(names))
    refs = [_reference(po, wl, top, n, n_iter, relax, raw) for n in distinct]
    fc.compare_batch(_download(b), refs, [distinct.index(n) for n in names])


def _tiled(po, wl, top, route="fit"):
    pool = [n for n, (_, r) in _cases(po, wl, top).items() if r == route]
    return [pool[f % len(pool)] for f in range(F)]


@pytest.mark.parametrize("top", fc.TOPS)
def test_fit_batch_runs_every_case_in_the_kernel(po, wl, top):
    """Every points-per-lane instantiation (k_frame_lean<1..4>: the batch's largest frame has 512, 1024, 1536, 2048 points; weights
    in registers up to 2, records re-read from 3), the kinds re-generated at those sizes.  No frame may leave for the fallback."""
    names = _tiled(po, wl, top)
    assert len(set(names)) >= 31 and max(_cases(po, wl, top)[n][0]["N"] for n in names) == top
    b = _batch(po, wl, top, names)
    b.run(5, True)
    assert b.engine() == 3 and b.fused_shape() == (512, 2), (b.engine(), b.fused_shape())
    assert b.fallback_frames() == 0
    _check(po, wl, top, b, names)
    b.close()


@pytest.mark.parametrize("top", fc.TOPS)
def test_flag_batch_leaves_exactly_the_predicted_frames(po, wl, top):
    """The fit batch with two copies of every case a closed rule rejects (22 frames, under the 1 / 8 of the batch at which the engine
    stops asking for the shape): exactly those are re-run, every frame's results are the reference's, twice on the same handle."""
    flags = sorted(n for n, (_, r) in _cases(po, wl, top).items() if r == "flag")
    assert len(flags) == 11
    names = _tiled(po, wl, top)
    for i, n in enumerate(flags + flags):
        names[5 + 11 * i] = n
    assert 2 * len(flags) <= 24 and sum(n in flags for n in names) == 2 * len(flags)
    assert max(_cases(po, wl, top)[n][0]["N"] for n in names) == top
    b = _batch(po, wl, top, names)
    for again in range(2):
        b.run(5, True)
        assert b.engine() == 3 and b.fused_shape() == (512, 2), (again, b.engine(), b.fused_shape())
        assert b.fallback_frames() == 2 * len(flags), (again, b.fallback_frames())
        _check(po, wl, top, b, names)
    b.close()


def test_plan_batch_gives_the_reference_whichever_way_the_plan_decides(po, wl):
    """Frames that no closed rule rejects and whose LDS plan is at its limit, among fit cases, in a batch of their own so that they
    cannot hide in the counts above.  Results only; the count observed is in notes/frame_lean_tests.md."""
    plans = sorted(n for n, (_, r) in _cases(po, wl, 2048).items() if r == "plan")
    assert plans == sorted(fc.PLAN_KINDS)
    names = _tiled(po, wl, 2048)
    for i in range(16):
        names[3 + 15 * i] = plans[i % len(plans)]
    b = _batch(po, wl, 2048, names)
    b.run(5, True)
    print("plan batch: %d of 16 plan frames left to the fallback" % b.fallback_frames())
    assert b.engine() == 3 and b.fallback_frames() <= 16
    _check(po, wl, 2048, b, names)
    b.close()


def test_fit_batch_with_raw_unaries_and_with_damping(po, wl):
    names = _tiled(po, wl, 2048)
    b = _batch(po, wl, 2048, names, raw=True)
    b.run(5, True)
    assert b.engine() == 3 and b.fused_shape() == (512, 2) and b.fallback_frames() == 0
    _check(po, wl, 2048, b, names, raw=True)
    b.close()
    b = _batch(po, wl, 2048, names)
    b.run(3, True, relax=0.5)
    assert b.engine() == 3 and b.fused_shape() == (512, 2) and b.fallback_frames() == 0
    _check(po, wl, 2048, b, names, n_iter=3, relax=0.5)
    b.close()


def test_the_hash_build_of_the_one_frame_kernel_on_the_same_cases(po, wl):
    """The same distinct cases three frames at a time: batches too small for the half-CU kernel run k_frame's hash build
    (csrc/frame_engine.hip), which must agree on every one of them -- results only."""
    cs = _cases(po, wl, 2048)
    names = sorted(cs, key=lambda n: (cs[n][1] != "fit", n))          # fit cases first: at most one other in a batch of three
    third = (len(names) + 2) // 3
    for i in range(third):
        part = [names[(i + j * third) % len(names)] for j in range(3)]
        b = _batch(po, wl, 2048, part)
        b.run(5, True)
        assert b.engine() == 3 and b.fused_shape() != (512, 2), (part, b.engine(), b.fused_shape())
        refs = [_reference(po, wl, 2048, n) for n in part]
        fc.compare_batch(_download(b), refs, [0, 1, 2])
        b.close()

"""Every entry point as the FIRST call after every state of a handle and of a batch.

An Engine's state is made lazily: a one-launch inference may still be pending, the lattices may exist only as staged features, they
may be in locality mode's internal point order, label-derived unaries may not be written yet, the normalisation factors may be
stale.  The long call sequences of the other tests exercise the transitions out of a state only with the first call behind it; here
each (state, entry point) pair gets a handle of its own, closed afterwards -- so parked handles are reused, whatever the last call
left in flight.  Everything is compared bit for bit: with the oracle where it has the call, and with the same call as the first one
on a fresh handle (inputs set, nothing else) or a fresh batch behind build() otherwise.  Only the answers that report on the state
itself -- engine(), the splat and blur plans of a handle in locality mode, and engine() / the two plans of a batch behind run(), which
has no lattice in HBM -- are compared with the same call behind calls that have settled everything.
"""
import importlib

import numpy as np
import pytest

import crf_cases as cc
import grad_support as gs

pkg = importlib.import_module("lc-crf-slam_amd")
pytestmark = pytest.mark.gpu

N_LOCALITY = 8192                                       # Engine::kPermMinPointsDefault: the release library's threshold itself
MU = np.float32([[0.25, 1.0], [0.75, -0.5]])            # state (e): a matrix that is neither Potts nor symmetric


def _problem(wl, key):
    if key == "slam":
        return wl.slam_problem(700, seed=61)
    if key == "sparse":                                 # does not fit the one-launch kernel: settling re-runs it
        return cc.shaped_problem(wl, 1200, "sparse", seed=5)
    if key == "large":
        # (features spread wide enough for short lattice rows: then the splat plan tells locality mode's sorted build, which takes
        # blur passes along, from the plain one, which takes none -- the only probe a handle has)
        return wl.generic_problem(N_LOCALITY, [3], 2, seed=77, spread=12.0)
    raise KeyError(key)


# state -> (problem, has the oracle the model?, what puts a handle with its inputs set into the state)
def _modes(h):
    h.set_normalization(0, pkg.NORMALIZE_SYMMETRIC)
    h.set_pairwise_compatibility(1, MU)


STATES = {
    "a_fresh": ("slam", True, lambda h: None),
    "b_pending": ("slam", True, lambda h: h.inference(5, True)),
    "c_pending_unfit": ("sparse", True, lambda h: h.inference(5, True)),
    "d_locality": ("large", True, lambda h: h.inference(3, True)),
    "e_modes": ("slam", False, lambda h: (_modes(h), h.inference(3))),
}
INFERENCE = {"b_pending": 5, "c_pending_unfit": 5, "d_locality": 3, "e_modes": 3}


def _x(pb):
    return np.random.default_rng(3).normal(0, 1, (pb["N"], pb["L"])).astype(np.float32)


def _steps(c, pb):
    c.start_inference()
    c.step_inference()
    c.step_inference()
    return [c.probability()]


def _kernel(c, pb):
    k = c.kernel(0)
    return [np.int32(k["V"]), k["offset"], k["bary"], k["nbr"], k["norm"]]


def _converged(c, pb):
    r = c.inference_converged(8, with_map=True)
    assert r == c.convergence()
    return [np.int32(r["iterations"]), np.float32(r["delta"]), np.int32(r["changed"]), np.int32(r["converged"]), c.probability(), c.map()]


def _backward(c, pb):
    G = np.random.default_rng(4).normal(0, 1, (pb["N"], pb["L"])).astype(np.float32)
    return list(gs.backward(c, 3, 0.9, G, len(pb["kernels"])))


# name -> (the call, does the oracle have it?, does it leave Q and the labels of the state's inference alone?)
CALLS = {
    "steps": (_steps, True, False),
    "apply": (lambda c, pb: [c.apply(0, np.zeros((pb["N"], pb["L"]), np.float32), _x(pb))], True, True),
    "kernel": (_kernel, True, True),
    "unary": (lambda c, pb: [c.unary()], True, True),
    "step_init": (lambda c, pb: [c.step_init()], False, True),
    "splat_plan": (lambda c, pb: [np.int64(list(c.splat_plan(0).values()))], False, True),
    "blur_plan": (lambda c, pb: [np.int64(list(c.blur_plan(0).values()))], False, True),
    "converged": (_converged, False, False),
    "engine": (lambda c, pb: [np.int64(c.engine())], False, True),
    "backward": (_backward, False, False),
}

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _handle(wl, state):
    pkey, _, enter = STATES[state]
    pb = _problem(wl, pkey)
    h = cc.setup(pkg.DenseCRFHIP, pb)
    enter(h)
    return h, pb


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert cc.same_bits(g, w), (what, i)


def _fresh_reference(wl, po, state, call):
    """The call as the first one on a fresh handle with the state's inputs (and terms' modes), checked against the oracle where it can be."""
    pkey, oracle_model, _ = STATES[state]
    fn, oracle_call, _ = CALLS[call]

    def make():
        pb = _problem(wl, pkey)
        h = cc.setup(pkg.DenseCRFHIP, pb)
        if state == "e_modes":
            _modes(h)
        want = fn(h, pb)
        h.close()
        if oracle_call and (oracle_model or call in ("kernel", "unary")):       # (the lattice and the raw unaries know no matrix or mode)
            o = cc.setup(po.OracleCRF, pb)
            _same(want, fn(o, pb), ("fresh handle against the oracle", pkey, call))
            o.close()
        return want
    return _cached(("fresh", pkey, state == "e_modes", call), make)


def _inference_reference(wl, po, state):
    """(Q, labels or None) of the state's inference(): the oracle's, or for the model it does not have a handle asked right away."""
    pkey, oracle_model, enter = STATES[state]

    def make():
        pb = _problem(wl, pkey)
        if oracle_model:
            o = cc.setup(po.OracleCRF, pb)
            o.inference_native(INFERENCE[state], True)
            out = o.probability(), o.map()
            o.close()
            return out
        h, _ = _handle(wl, state)
        out = h.probability(), None
        h.close()
        return out
    return _cached(("inference", state), make)


@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("state", sorted(STATES))
def test_first_call_on_a_handle_is_history_independent(po, wl, state, call):
    fn, _, keeps_results = CALLS[call]
    if call == "engine" or (call in ("splat_plan", "blur_plan") and state == "d_locality"):
        # reports on the state: the same answer as behind calls that have settled and read everything -- and the documented one
        r, _ = _handle(wl, state)
        r.synchronize()
        r.probability()
        want = fn(r, None)
        r.close()
        if call in ("splat_plan", "blur_plan"):         # passes (in_splat) >= 1: state (d) IS in locality mode, whatever the threshold becomes
            assert int(want[0][0]) >= 1, want
            want_engine = None
        else:
            want_engine = int(want[0][0])
        assert want_engine is None or want_engine == {"a_fresh": 1, "b_pending": 3, "d_locality": 1}.get(state, want_engine), (state, want)
        assert want_engine is None or state != "c_pending_unfit" or want_engine in (1, 2), want     # (re-run on the two-kernel path: what that ran on)
    else:
        want = _fresh_reference(wl, po, state, call)
    h, pb = _handle(wl, state)
    _same(fn(h, pb), want, (state, call))
    if keeps_results and state in INFERENCE:            # ... and the state's own results are still what they were
        q, labels = _inference_reference(wl, po, state)
        assert cc.same_bits(h.probability(), q), (state, call, "Q of the state's inference")
        if labels is not None:
            assert np.array_equal(h.map(), labels), (state, call, "labels of the state's inference")
    h.close()


@pytest.mark.parametrize("state", ["b_pending", "c_pending_unfit", "d_locality"])
def test_map_first_on_a_handle_takes_the_labels_as_they_land(po, wl, state):
    """getMap() right behind inference(n, true): label by label out of pinned memory (b), through the -2 marker into the re-run (c),
    the ordinary way (d) -- the oracle's labels each time, and its Q behind them."""
    q, labels = _inference_reference(wl, po, state)
    h, _ = _handle(wl, state)
    assert np.array_equal(h.map(), labels), state
    assert cc.same_bits(h.probability(), q), state
    assert np.array_equal(h.map(), labels), state       # (nothing in flight any more: the ordinary path)
    h.close()


# ---- a batch of three frames, the same way --------------------------------------------------------------------------------------
def _batch_problems(wl, key):
    if key == "run":
        return [wl.slam_problem(n, seed=70 + i) for i, n in enumerate((700, 655, 512))]
    if key == "run_unfit":
        return [wl.slam_problem(700, seed=70), cc.shaped_problem(wl, 1200, "sparse", seed=5), wl.slam_problem(512, seed=72)]
    pbs = [wl.generic_problem(N_LOCALITY - 37 * i, [3], 2, seed=80 + i, spread=2.8) for i in range(3)]
    w = pbs[0]["kernels"][0][1]                         # (a batch has one weight per term)
    return [dict(pb, kernels=[(pb["kernels"][0][0], w)]) for pb in pbs]


def _batch(wl, key):
    pbs = _batch_problems(wl, key)
    if key != "built_locality":
        return cc.batch_of(pbs), pbs
    F, maxN = len(pbs), N_LOCALITY
    feats, unary = np.zeros((F, maxN, 3), np.float32), np.zeros((F, maxN, 2), np.float32)
    for f, pb in enumerate(pbs):
        feats[f, :pb["N"]], unary[f, :pb["N"]] = pb["kernels"][0][0], pb["unary"]
    b = pkg.BatchCRF(F, maxN, 2, [3], [float(pbs[0]["kernels"][0][1])])
    b.set_inputs_host([pb["N"] for pb in pbs], [feats], unary=unary)
    return b, pbs


def _enter_batch(b, key):
    if key == "built_locality":
        b.build()
        b.inference(3)
        assert b.locality_mode()[0]
    else:
        b.run(5, True)


def _rows(a, pbs):
    return [np.ascontiguousarray(a[f, :pb["N"]]) for f, pb in enumerate(pbs)]


def _batch_converged(b, pbs):
    b.inference_converged(8)
    r = b.convergence()
    return [r["iterations"], r["delta"], r["changed"], r["converged"]] + _rows(b.probability(), pbs) + _rows(b.map(), pbs)


def _batch_backward(b, pbs):
    G = np.random.default_rng(6).normal(0, 1, (len(pbs), b.maxN, 2)).astype(np.float32)
    gu, gw = gs.batch_backward(b, 3, 0.9, G, len(b.dims))
    return _rows(gu, pbs) + [gw]


# name -> (the call, the reference: "built" a fresh batch behind build(); "settled" the same for a batch in a built state, and for one
# behind run(), which has no lattice in HBM for these calls to report on, the state behind calls that settle and read it)
E_STATE = -5
BATCH_CALLS = {
    "norm": (lambda b, pbs: _rows(b.norm(0), pbs), "built"),
    "lattice_sizes": (lambda b, pbs: [b.lattice_sizes(0)], "built"),
    "engine": (lambda b, pbs: [np.int64(b.engine())], "settled"),
    "splat_plan": (lambda b, pbs: [np.int64(list(b.splat_plan(0).values()))], "settled"),
    "blur_plan": (lambda b, pbs: [np.int64(list(b.blur_plan(0).values()))], "settled"),
    "converged": (_batch_converged, "settled"),                   # (wants lccrf_batch_build: LCCRF_E_STATE behind a run)
    "backward": (_batch_backward, "built"),
}


def _batch_results(wl, po, key):
    """(Q rows, label rows) of the state's run, from the oracle frame by frame"""
    def make():
        q, m = [], []
        for pb in _batch_problems(wl, key):
            o = cc.setup(po.OracleCRF, pb)
            o.inference_native(3 if key == "built_locality" else 5, True)
            q.append(o.probability())
            m.append(o.map())
            o.close()
        return q, m
    return _cached(("batch results", key), make)


@pytest.mark.parametrize("call", sorted(BATCH_CALLS))
@pytest.mark.parametrize("state", ["run", "run_unfit", "built_locality"])
def test_first_call_on_a_batch_is_history_independent(po, wl, state, call):
    fn, kind = BATCH_CALLS[call]
    refused = call == "converged" and state != "built_locality"
    if kind == "built" or state == "built_locality":
        def make():
            r, pbs = _batch(wl, state)
            r.build()
            want = fn(r, pbs)
            r.close()
            if call in ("norm", "lattice_sizes"):       # the oracle has these: frame by frame
                os_ = [cc.setup(po.OracleCRF, pb) for pb in pbs]
                ks = [o.kernel(0) for o in os_]
                _same(want, [k["norm"] for k in ks] if call == "norm" else [np.int32([k["V"] for k in ks])], ("oracle", state, call))
                for o in os_:
                    o.close()
            return want
        want = _cached(("batch", state, call), make)
    elif not refused:
        r, pbs = _batch(wl, state)
        _enter_batch(r, state)
        r.synchronize()
        r.probability()
        want = fn(r, pbs)
        r.close()
    b, pbs = _batch(wl, state)
    _enter_batch(b, state)
    if refused:                                         # ... and the refusal leaves the pending run as it was (below)
        with pytest.raises(pkg.LccrfError) as err:
            fn(b, pbs)
        assert err.value.code == E_STATE, err.value
        got = want = []
    else:
        got = fn(b, pbs)
    _same(got, want, (state, call))
    if call not in ("backward",) and not (call == "converged" and len(got) > 1):   # the state's own results are still what they were
        q, m = _batch_results(wl, po, state)
        _same(_rows(b.probability(), pbs), q, (state, call, "Q of the state's run"))
        _same(_rows(b.map(), pbs), m, (state, call, "labels of the state's run"))
    b.close()

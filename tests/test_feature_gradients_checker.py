"""CPU tests of the feature-gradient checker (tests/meanfield_f64_features.py): what lccrf_inference_backward_features
(include/lccrf.h section 1d) is held against, pinned before any kernel runs -- the weights as a function of the features against
the oracle's, the forward against the oracle's Q, gradcheck, the fixed-topology derivative against a central difference with the
lattices REBUILT on both sides (float64 only), and the hand-written reverse sweep against autograd."""
import numpy as np
import pytest

import crf_cases as cc
import feature_cases as fc
import grad_support as gs
import gradient_settings as gset
import lattice_tie_cases as tc
import meanfield_f64 as mf
import meanfield_f64_features as mff

BARY_BAR = 4 * 2.6e-6          # test_bary_is_the_oracles: 4 x the largest difference measured


def _checker(po, pb):
    o = cc.setup(po.OracleCRF, pb)
    return o, mff.lattices(o, pb), o.unary().astype(np.float64)


@pytest.mark.parametrize("name", fc.CASES)
def test_bary_is_the_oracles(po, wl, golden, name):
    """The checker's b (float64, linear in the features inside the oracle's simplex) against the oracle's float32 bary, and the
    simplex itself: every corner key formed from (rem0, rank) is the key of the oracle's vertex, for every point of every case (no
    case needed its point count lowered).  The oracle forms v = (el - rem0) / (d+1) in float32 with |el| up to a few hundred, so
    the difference is a few ulp of el, not of 1: measured largest |b - bary| 2.6e-6 (slam:C3 and c2; 2.5e-6 slam:N1001, <= 1.9e-6
    on every other case); the bar is 4 x the largest."""
    pb, _ = fc.case(name, golden, po, wl)
    o, lats, _ = _checker(po, pb)
    worst = 0.0
    for lat in lats:
        assert lat.topology_agrees()
        worst = max(worst, float(np.abs(lat.linear_bary - lat.oracle_bary).max()))
        assert np.abs(lat.linear_bary.sum(1) - 1).max() < 1e-12 and lat.linear_bary.min() > -1e-12
        assert np.array_equal(lat.bary.numpy(), lat.oracle_bary)
    print("largest |b - bary| %s: %.3g" % (name, worst))
    assert worst <= BARY_BAR


@pytest.mark.parametrize("name", gset.TIES_CASES)
def test_simplex_is_the_oracles_at_exact_ties(po, name):
    """Points ON a float32 rank tie (tests/lattice_tie_cases.py): the float64 order of el - rem0 is not the build's there and would
    give the simplex across the boundary (7 + 3 points of ties:slam256 and 12 of ties:d5 did before the ranks were read off the
    oracle's corner keys: the one-sided derivative is another).  The checks of test_bary_is_the_oracles under its bar."""
    pb = tc.problem(name)
    o, lats, _ = _checker(po, pb)
    for lat, (f, _) in zip(lats, pb["kernels"]):
        s = tc.simplex_f32(f)
        assert s["rank_tie"].sum() >= 12 and (mff.ranks_of(lat.el64 - lat.rem0) != lat.rank).any()
        assert lat.topology_agrees() and np.array_equal(lat.rank, s["rank"].astype(np.int64))
        assert np.abs(lat.linear_bary - lat.oracle_bary).max() <= BARY_BAR
        # (a float32 tie is no float64 tie: in float64 the point lies outside the build's simplex by the rounding of el, no more)
        assert np.abs(lat.linear_bary.sum(1) - 1).max() < 1e-12 and lat.linear_bary.min() >= -BARY_BAR
        assert np.array_equal(lat.bary.numpy(), lat.oracle_bary)


# the cases of test_checker_forward_matches_the_oracle without the tie cases, and the tie-free generic frames
FORWARD_CASES = ["slam:N1000", "slam:relax"] + fc.CASES


@pytest.mark.parametrize("name", FORWARD_CASES)
@pytest.mark.parametrize("T,relax", [(1, 1.0), (5, 1.0), (5, 0.7)])
def test_feature_checker_forward_matches_the_oracle(po, wl, golden, name, T, relax):
    """The bars of test_checker_forward_matches_the_oracle: 1e-5, and 5e-5 for several terms of different d on one CRF (that
    test's generic:multi; here also nt:d2-5-3_L9).  Measured: generic:multi 3.0e-5, nt:d2-5-3_L9 1.2e-5, every other case
    <= 5.8e-6.  This holds because the checker carries the oracle's float32 rounding of b as a constant
    (meanfield_f64_features.FeatureLattice); with the bare linear form, whose b is up to 2.6e-6 away from the oracle's, the
    distance to the oracle's Q grows to 1.3e-5 on bilateral:c5, 1.7e-5 on large:c5 and 7.4e-5 on a tie-free d = 4 frame at
    T = 5 -- the oracle's rounding carried through five iterations."""
    import torch
    pb, _ = fc.case(name, golden, po, wl)
    o, lats, U = _checker(po, pb)
    o.inference_native(T, False, relax)
    q = mf.forward(torch.as_tensor(U), torch.as_tensor(gs.weights(pb)), lats, T, relax).numpy()
    err = np.abs(q - o.probability()).max()
    print("largest |Q - oracle| %s T=%d relax=%g: %.3g" % (name, T, relax, err))
    assert err <= (5e-5 if name in ("generic:multi", "nt:d2-5-3_L9") else 1e-5)     # (several terms of different d on one CRF)


def test_feature_checker_gradcheck(po, wl):
    import torch
    pb = wl.generic_problem(40, [2, 3], 3, seed=4)
    o, lats, U = _checker(po, pb)
    u = torch.as_tensor(U)
    w = torch.as_tensor(gs.weights(pb))
    G = torch.as_tensor(np.random.default_rng(0).standard_normal(U.shape))
    fs = [torch.as_tensor(lat.feat32.astype(np.float64)).clone().requires_grad_(True) for lat in lats]

    def run(relax):
        def f(*feats):
            for lat, x in zip(lats, feats):
                lat.bind(x)
            return mf.forward(u, w, lats, 3, relax)
        return f
    for relax in (1.0, 0.7):
        assert torch.autograd.gradcheck(run(relax), tuple(fs), eps=1e-7, atol=1e-6)


def _fd_problem(wl, name):
    if name == "slam":
        pb = wl.slam_problem(300, seed=5)
        w = gs.weights(pb) / 10                                 # (the TUM3 weights saturate most rows: their gradient is ~0)
        return pb, w
    d, N, L = {"d2": (2, 300, 2), "d3": (3, 200, 3), "d5": (5, 152, 2)}[name]       # (multiples of 4: no phantom points, quirk Q1, which the builder does not make)
    pb = wl.generic_problem(N, [d], L, seed=3, spread=1.5)
    return pb, np.array([4.0])


@pytest.mark.parametrize("name", ["d2", "d3", "d5", "slam"])
def test_fixed_topology_derivative_is_the_derivative_of_the_rebuilt_filter(po, wl, name):
    """(L(f + h delta) - L(f - h delta)) / 2h with every lattice REBUILT at f +- h delta (meanfield_f64_features.build_kern, a
    float64 builder that shares nothing with the oracle) against <dL/df, delta> of the checker at f, h = 1e-6, T = 3, relax = 0.7,
    float64 throughout.  Bar 1e-6 relative; measured d2 1.1e-9, d3 3.4e-9, d5 1.3e-10, slam (two terms) 4.2e-11.  The builder
    itself is checked first: on the case's float32 features it gives the oracle's V and, up to the numbering, its offsets."""
    pb, w = _fd_problem(wl, name)
    o = cc.setup(po.OracleCRF, pb)
    U = o.unary().astype(np.float64)
    feats = [f.astype(np.float64) for f, _ in pb["kernels"]]
    for k, f in enumerate(feats):
        kern, ok = mff.build_kern(f), o.kernel(k)
        assert kern["V"] == ok["V"]
        assert np.array_equal(kern["keys"][kern["offset"]], np.asarray(ok["keys"], np.int64)[ok["offset"]])
    rng = np.random.default_rng(11)
    G = rng.standard_normal(U.shape)
    delta = [rng.standard_normal(f.shape) for f in feats]
    T, relax, h = 3, 0.7, 1e-6
    lats = [mff.BuiltLattice(f) for f in feats]
    _, _, gf, _ = mff.feature_gradients(U, w, lats, T, relax, G, feats=feats)
    an = sum(float((g * dl).sum()) for g, dl in zip(gf, delta))
    lp = mff.rebuilt_loss(U, w, [f + h * dl for f, dl in zip(feats, delta)], T, relax, G)
    lm = mff.rebuilt_loss(U, w, [f - h * dl for f, dl in zip(feats, delta)], T, relax, G)
    fd = (lp - lm) / (2 * h)
    rel = abs(fd - an) / abs(an)
    print("central difference %s: fd %.10g analytic %.10g relative %.3g" % (name, fd, an, rel))
    assert rel <= 1e-6


@pytest.mark.parametrize("name", ["slam:N1001", "generic:multi", "nt:d6_L3", "nt:d8_L33", "nt:d2-5-3_L9", "c2"])
@pytest.mark.parametrize("T,relax", [(1, 1.0), (3, 0.7), (5, 1.0)])
def test_hand_written_sweep_equals_autograd(po, wl, golden, name, T, relax):
    """Steps 1 to 3 of section 1d as a loop (slice-side and splat-side corner dots per iteration and term, the norm part after the
    loop, then the closed form from corner weights to features) against autograd through the checker: 1e-10 relative L2 per
    term."""
    pb, _ = fc.case(name, golden, po, wl)
    o, lats, U = _checker(po, pb)
    w = gs.weights(pb) / (10 if name in ("slam:N1001", "c2") else 1)
    G = np.random.default_rng(7).standard_normal(U.shape)
    _, _, ref, _ = mff.feature_gradients(U, w, lats, T, relax, G)
    got = mff.sweep_feature_gradients(U, w, lats, T, relax, G)
    for k, (a, b) in enumerate(zip(got, ref)):
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("sweep against autograd %s term %d T=%d relax=%g: %.3g (|G| %.3g)" % (name, k, T, relax, rel, np.linalg.norm(b)))
        assert rel <= 1e-10


def test_feature_gradient_is_zero_at_t0(po, wl):
    pb = wl.generic_problem(60, [3], 3, seed=2)
    o, lats, U = _checker(po, pb)
    G = np.random.default_rng(1).standard_normal(U.shape)
    assert np.all(mff.sweep_feature_gradients(U, gs.weights(pb), lats, 0, 1.0, G)[0] == 0)
    assert np.all(mff.feature_gradients(U, gs.weights(pb), lats, 0, 1.0, G)[2][0] == 0)

"""Do the bars of the gradient tests have power?  No GPU: the checkers alone, on the settings the GPU tests are parametrised with
(tests/gradient_settings.py, tests/joint_checker.py, tests/crf_cases.py, tests/feature_cases.py -- imported, not copied).

Per setting the float64 and float32 checkers give every output's bars (grad_support.bars: the L2 bar and, for the per-point outputs,
the row bar).  Asserted, per list and case:
  cap      every bar <= grad_support.BAR_CAP (1e-2): beyond it a setting checks nothing;
  faults   the float64 checker with a fault planted in its backward (grad_support.planted: Phi for Phi^T in the filter; mu for mu^T
           in the compatibility product where the setting has matrices) lands beyond 2 x the bar -- a device within its bar can hide
           up to one bar of a fault -- in every output, for at least one setting of T >= 2, and in dL/dU for every setting of T = 5.
           Two exemptions, each checked (the fault moves the exempt outputs by <= 1e-12) and not assumed: a case whose terms are all
           d = 1 from the filter's fault (Phi = Phi^T there); a case of L = 2 from the matrix fault in all but dL/df of the terms with a matrix --
           the softmax backward's rows sum to 0, so at two labels they are a (1, -1), and (1, -1) mu - (1, -1) mu^T =
           (mu01 - mu10) (1, 1): constant along the row, kept so by the filter, annihilated by the next softmax backward; only that
           term's dL/df, whose splat side weighs the row by Q, sees it;
  local    a correct per-point array with one row scaled by 1.05 -- the row whose norm is nearest the rms row norm, and the largest
           of the last four rows -- is rejected by the row metric (the L2 norm's verdict is printed beside it: it passes).  Where the
           scaled tail row moves the row metric by no more than GRAD_TOL, the floor of every bar, no bar this project allows can see
           it (saturated rows: no gradient there to misplace): printed, not asserted.
large:c5 (8704 points) and the image crop run their T = 5 settings only, where a list has one."""
import numpy as np
import pytest

import crf_cases as cc
import feature_cases as fc
import grad_support as gs
import gradient_settings as gset
import joint_checker as jc
import normalization_checker as nc

BIG = ("large:c5", "image64x48")
POWER = 2.0                                                      # a planted fault must land beyond POWER x the bar
# Cases no search rescued (notes/gradient_bars.md): five points under the SLAM weights sit in lattice cells of their own, the filter
# couples them by 1e-7 and so is its own transpose to that order; from T = 5 on every row is saturated.  40 seeds, and the weights
# at a tenth, leave the untransposed filter within 0.8 of a bar in some output.  The case stays for what it is there for (N % 4 = 1,
# one block, phantom rows); that it has no power against this fault is asserted, so the entry cannot outlive its reason.
WITHOUT_POWER = {("meanfield", "slam:N5"), ("features", "slam:N5")}


def _settings(name, Ts, relaxes):
    return [(T, r) for T in Ts for r in relaxes]


def groups(po, wl, golden):
    """{(list, case): [(setting id, T, has matrices, builder of the setting)]}"""
    out = {}

    def add(lst, case, sid, T, mu, build):
        out.setdefault((lst, case), []).append((sid, T, mu, build))
    for n, T, r in gset.MEANFIELD_SETTINGS:
        if n not in BIG or T == 5:
            add("meanfield", n, "T%d-r%g" % (T, r), T, False, lambda n=n, T=T, r=r: gset.meanfield(po, wl, golden, n, T, r))
    for n, T, r in gset.FEATURE_SETTINGS:
        if n not in BIG or T == 5:
            add("features", n, "T%d-r%g" % (T, r), T, False, lambda n=n, T=T, r=r: gset.features(po, wl, golden, n, T, r))
    for n, T, r in gset.TIES:
        add("ties", n, "T%d-r%g" % (T, r), T, False, lambda n=n, T=T, r=r: gset.ties(po, wl, golden, n, T, r))
    for n, T, r in gset.COMPAT_SETTINGS:
        if n not in BIG or T == 5:
            add("compat", n, "T%d-r%g" % (T, r), T, True, lambda n=n, T=T, r=r: gset.compat(po, wl, golden, n, T, r))
    for n, T, r in jc.SETTINGS:
        add("joint", n, "T%d-r%g" % (T, r), T, True, lambda n=n, T=T, r=r: jc.reference_for(po, wl, golden, n, T, r))
    for n in jc.MIXED_CASES:
        for T, r in jc.MIXED_SETTINGS:
            add("joint-mixed", n, "T%d-r%g" % (T, r), T, True, lambda n=n, T=T, r=r: jc.reference_for(po, wl, golden, n, T, r, "mixed"))
    for n in jc.POTTS_CASES:
        T, r = jc.POTTS_SETTING
        add("joint-potts", n, "T%d-r%g" % (T, r), T, False, lambda n=n, T=T, r=r: jc.reference_for(po, wl, golden, n, T, r, "potts"))
    for n, m, T, r in gset.NORM_SETTINGS:
        add("normalization", n, "%s-T%d-r%g" % (nc.MODE_NAMES[m], T, r), T, True,
            lambda n=n, m=m, T=T, r=r: gset.normalization(po, wl, golden, n, m, T, r))
    for L in gset.LANE_LABELS:
        for K in gset.LANE_TERMS:
            for T, r in _settings("", gset.T_SHORT, gset.RELAX_SET):
                add("labels", "L%d-K%d" % (L, K), "T%d-r%g" % (T, r), T, False, lambda L=L, K=K, T=T, r=r: gset.lane_group(po, L, K, T, r))
    for L in gset.TERMLESS_LABELS:
        for T, r in _settings("", gset.T_SHORT, gset.RELAX_SET):
            add("labels", "L%d-K0" % L, "T%d-r%g" % (T, r), T, False, lambda L=L, T=T, r=r: gset.termless(L, T, r))

    def frames(lst, case, fr, G, settings, known_as=""):
        for f, n in enumerate(fr.N):
            for T, r in settings:
                if n:
                    add(lst, "%s-frame%d" % (case, f), "T%d-r%g" % (T, r), T, False,
                        lambda f=f, T=T, r=r: gset.batch_frame(po, fr, G, f, T, r, "%s frame %d" % (case, f), known_as))
    for L in gset.K8_BATCH_LABELS:
        fr = gset.k8_frames(L)
        frames("labels-batch", "L%d" % L, fr, fr.grad_prob(L), gset.K8_BATCH_SETTINGS)
    import batch_cases as bc
    fr = bc.slam_frames(golden, wl, Ns=gset.BATCH_FRAMES)
    frames("batch", "slam", fr, fr.grad_prob(gset.BATCH_GRAD_SEED), [(gset.BATCH_T, r) for r in gset.RELAX_SET], "batch:slam")
    return out


def group_ids():
    """the (list, case) pairs of groups(), without building anything"""
    ids = [("meanfield", n) for n in cc.CASES] + [("features", n) for n in fc.CASES] + [("ties", n) for n in dict.fromkeys(n for n, _, _ in gset.TIES)] + [("compat", n) for n in gset.COMPAT_CASES]
    ids += [("joint", n) for n in dict.fromkeys(n for n, _, _ in jc.SETTINGS)]
    ids += [("joint-mixed", n) for n in jc.MIXED_CASES] + [("joint-potts", n) for n in jc.POTTS_CASES]
    ids += [("normalization", n) for n in gset.NORM_CASES]
    ids += [("labels", "L%d-K%d" % (L, K)) for L in gset.LANE_LABELS for K in gset.LANE_TERMS]
    ids += [("labels", "L%d-K0" % L) for L in gset.TERMLESS_LABELS]
    ids += [("labels-batch", "L%d-frame%d" % (L, f)) for L in gset.K8_BATCH_LABELS for f in (0, 2, 3, 4)]
    ids += [("batch", "slam-frame%d" % f) for f, n in enumerate(gset.BATCH_FRAMES) if n]
    return ids


def local_faults(ref):
    """{name: (row index, the array with that row scaled by 1.05)} of a per-point array with a gradient in it: the row whose norm is
    nearest the rms row norm, and the largest of the last four rows"""
    norms = np.linalg.norm(ref.reshape(ref.shape[0], -1), axis=1)
    rms = np.sqrt(np.mean(norms ** 2))
    tail = max(ref.shape[0] - 4, 0)
    out = {}
    for name, i in (("rms row", int(np.argmin(np.abs(norms - rms)))), ("tail row", tail + int(np.argmax(norms[tail:])))):
        a = ref.copy()
        a[i] *= 1.05
        out[name] = (i, a)
    return out


def measure(sid, T, has_mu, s):
    """one setting's record: bars, what each planted fault moves each output by (relative L2, under the output's floor), and the
    verdicts of both metrics on the local faults"""
    refs = [s[k] for k in ("ref", "ref_1c") if k in s]
    rec = dict(id=sid, T=T, dims=s["dims"], L=s["pb"]["L"], bars={}, moved={}, local=[])
    rec["with_mu"] = [k for k, m in enumerate(s.get("mats") or []) if m is not None]
    rec["saturated"] = all(np.linalg.norm(r.ref[n]) <= r.floors[n] for r in refs for n in r.ref if n != "dL/dmu")
    for r in refs:
        rec["bars"].update(r.bars())
    faults = (["filter"] if T >= 1 and s["dims"] else []) + (["compat"] if has_mu and T >= 1 else [])
    for fault in faults:
        rec["moved"][fault] = {}
        for r in refs:
            got = r.faulty(fault)
            rec["moved"][fault].update((n, gs.rel(got[n], r.ref[n], r.floors[n])) for n in got)
    for r in refs:
        for n in sorted(r.rows):
            ref, floor = r.ref[n], r.floors[n]
            if ref.shape[0] == 0 or np.linalg.norm(ref) <= floor:
                continue                                         # no gradient here to misplace (T = 0: dL/df = 0; saturated rows)
            bar, rbar = rec["bars"][n][:2]
            for what, (i, a) in local_faults(ref).items():
                rec["local"].append(dict(out=n, what=what, row=i, N=ref.shape[0], l2=gs.rel(a, ref, floor), bar=bar,
                                         rows=gs.worst_row(a, ref, floor)[0], rbar=rbar))
    return rec


_RECORDS = {}


def records(po, wl, golden, key):
    """the records of one (list, case): every setting's gradients computed once, shared by the three tests"""
    if "groups" not in _RECORDS:
        _RECORDS["groups"] = groups(po, wl, golden)
    if key not in _RECORDS:
        _RECORDS[key] = [measure(sid, T, mu, build()) for sid, T, mu, build in _RECORDS["groups"][key]]
        jc._REFS.clear()
    return _RECORDS[key]


GROUPS = group_ids()
IDS = ["%s/%s" % k for k in GROUPS]


def test_group_ids_are_the_groups(po, wl, golden):
    assert sorted(GROUPS) == sorted(groups(po, wl, golden))


@pytest.mark.parametrize("key", GROUPS, ids=IDS)
def test_every_bar_is_under_the_cap(po, wl, golden, key):
    bad = []
    for rec in records(po, wl, golden, key):
        for n, (bar, rbar, f, fr) in rec["bars"].items():
            print("%s/%s %s %s: L2 bar %.3g%s" % (key + (rec["id"], n, bar, "" if rbar is None else ", row bar %.3g" % rbar)))
            if bar > gs.BAR_CAP or (rbar is not None and rbar > gs.BAR_CAP):
                bad.append((rec["id"], n, bar, rbar))
    assert not bad, "bars beyond %g check nothing: %s" % (gs.BAR_CAP, bad)


@pytest.mark.parametrize("key", GROUPS, ids=IDS)
def test_planted_transposition_faults_land_beyond_twice_the_bar(po, wl, golden, key):
    recs = records(po, wl, golden, key)
    for fault in ("filter", "compat"):
        have = [r for r in recs if fault in r["moved"] and not r["saturated"]]
        for r in recs:
            if fault in r["moved"] and r["saturated"]:             # every output below its floor: by the section 1c convention
                print("%s/%s %s: every gradient is below its floor (saturated rows), no fault can show" % (key + (r["id"],)))
        if not have:
            continue
        if fault == "filter" and all(d == 1 for d in have[0]["dims"]):
            # Phi = Phi^T at d = 1 (one blur direction and its mirror image): such a case says nothing about the sweep's order
            worst = max(max(r["moved"][fault].values()) for r in have)
            print("%s/%s: every term d = 1, the untransposed filter moves no output by more than %.3g" % (key + (worst,)))
            assert worst <= 1e-12
            continue
        blind = ()
        if fault == "compat" and have[0]["L"] == 2:               # only dL/df of a term that carries a matrix sees it
            blind = [n for n in have[0]["moved"][fault] if n not in ["dL/df%d" % k for k in have[0]["with_mu"]]]
            worst = max(r["moved"][fault][n] for r in have for n in blind)
            print("%s/%s: L = 2, mu for mu^T moves none of %s by more than %.3g" % (key + (" ".join(blind), worst)))
            assert worst <= 1e-12
        ratios = {r["id"]: {n: m / r["bars"][n][0] for n, m in r["moved"][fault].items() if n not in blind} for r in have}
        if not any(ratios.values()):
            continue
        for sid, q in ratios.items():
            print("%s/%s %s fault %s: moved / bar %s" % (key + (sid, fault, " ".join("%s %.3g" % x for x in q.items()))))
        late = [r["id"] for r in have if r["T"] >= 2]
        assert late, "no setting of T >= 2"
        if key in WITHOUT_POWER:
            assert not any(min(ratios[sid].values()) > POWER for sid in late), "%s/%s has power now: take it out of WITHOUT_POWER" % key
            continue
        assert any(min(ratios[sid].values()) > POWER for sid in late), \
            "fault %s: no setting of T >= 2 pushes every output beyond %g x its bar: %s" % (fault, POWER, {s: ratios[s] for s in late})
        weak = [r["id"] for r in have if r["T"] == 5 and "dL/dU" in ratios[r["id"]] and not ratios[r["id"]]["dL/dU"] > POWER]
        assert not weak, "fault %s: dL/dU within %g x its bar at T = 5 in %s" % (fault, POWER, weak)


@pytest.mark.parametrize("key", GROUPS, ids=IDS)
def test_the_row_metric_rejects_a_local_fault_the_l2_norm_passes(po, wl, golden, key):
    missed = []
    for rec in records(po, wl, golden, key):
        for x in rec["local"]:
            print("%s/%s %s %s, %s (row %d of %d) x 1.05: row metric %.3g (bar %.3g) %s; L2 %.3g (bar %.3g) %s"
                  % (key + (rec["id"], x["out"], x["what"], x["row"], x["N"], x["rows"], x["rbar"],
                            "rejects" if x["rows"] > x["rbar"] else "PASSES" if x["rows"] > gs.GRAD_TOL else "below the floor of every bar", x["l2"], x["bar"], "rejects" if x["l2"] > x["bar"] else "passes")))
            if not x["rows"] > x["rbar"] and x["rows"] > gs.GRAD_TOL:
                missed.append((rec["id"], x["out"], x["what"], x["rows"], x["rbar"]))
    assert not missed, "the row metric lets a row scaled by 1.05 through: %s" % missed

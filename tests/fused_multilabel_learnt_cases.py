"""What tests/test_fused_multilabel_learnt.py, tests/test_fused_multilabel_learnt_resources.py and tests/perf/fused_multilabel_learnt.py
share: the learnt models (label-compatibility matrices, normalisation modes) put on the frames of tests/fused_multilabel_cases.py for the
fused engine's kernel csrc/fused_multilabel_general.hip (LCCRF_MULTILABEL_LEARNT, engine 6), the model each case runs under, and the
float32 restatement (tests/normalization_checker.py) each case is compared with."""
import numpy as np

import compat_checker as ck
import crf_cases as cc
import fused_multilabel_cases as mc
import normalization_checker as nc

LANES = mc.LANES
# the shipped range, as the header of csrc/fused_multilabel_general.hip states it: label count -> largest frame (active points)
PLAN = {3: 2048, 4: 2048, 5: 1024, 6: 1024, 7: 1024, 8: 1024}
LEARNT, POTTS = 2, 1                                             # LCCRF_MULTILABEL_LEARNT, LCCRF_MULTILABEL_POTTS

# name -> (mode of the first / the second term, which of them carries a matrix); a one-term frame takes the first entries, and every
# model's first term alone is still a learnt one
MODELS = {
    # a matrix without a mode, a mode without a matrix
    "matrix0": ((nc.AFTER, nc.AFTER), (1, 0)),
    "matrix1": ((nc.AFTER, nc.AFTER), (0, 1)),                   # (two terms only)
    "matrices": ((nc.AFTER, nc.AFTER), (1, 1)),
    "before": ((nc.BEFORE, nc.AFTER), (0, 0)),
    # both on one term; a matrix on one term and a mode on the other -- each with a matrix AND a factor in front of a filter
    "symmetric+matrix": ((nc.SYMMETRIC, nc.NONE), (1, 0)),
    "matrix0/before1": ((nc.AFTER, nc.BEFORE), (1, 0)),         # (two terms only: its first term alone has no factor in front)
    "none/matrix1": ((nc.NONE, nc.SYMMETRIC), (0, 1)),           # (two terms only)
    "before+matrix": ((nc.BEFORE, nc.SYMMETRIC), (1, 1)),
}
_BOTH = {1: ("symmetric+matrix", "before+matrix"), 2: ("symmetric+matrix", "matrix0/before1", "none/matrix1", "before+matrix")}
# the margin frames of fused_multilabel_cases.CASES: the plain combinations take turns there
_MARGIN = {"L3/N5": "matrix0", "L4/N5": "before", "L3/N7": "matrix1", "L4/N7": "matrices", "L3/N2048": "matrix0/before1",
           "L4/N2048": "none/matrix1", "L3/sparse:N1100": "symmetric+matrix", "L8/N1024/smooth": "matrix0"}


def matrix(L, k, seed=77):
    """eye(L) + 0.3 N(0, 1) in float32, not symmetric, seeded by [seed, k, L]"""
    rng = np.random.default_rng([seed, k, L])
    return (np.eye(L) + 0.3 * rng.standard_normal((L, L))).astype(np.float32)


def model(name, K, L):
    """(modes, matrices) of model `name` on a frame of K terms and L labels"""
    modes, has = MODELS[name]
    return list(modes[:K]), [matrix(L, k) if has[k] else None for k in range(K)]


def _case_models():
    """case name -> model name: the margin frames as listed; on the frames that fill the lanes -- one per instantiation of the kernel --
    the models with a matrix AND a factor in front of a filter take turns, so that every instantiation sees both and every odd L a
    matrix"""
    out, turn = {}, {1: 0, 2: 0}
    for name, (args, _) in mc.CASES.items():
        if args["N"] > PLAN[args["L"]]:
            continue
        if name in _MARGIN:
            out[name] = _MARGIN[name]
            continue
        K = len(mc.TERMS[args.get("terms", "")])
        out[name] = _BOTH[K][turn[K] % len(_BOTH[K])]
        turn[K] += 1
    return out


CASE_MODEL = _case_models()
CASES = {name: mc.CASES[name] for name in CASE_MODEL}            # name -> (arguments of problem(), instantiation class), as the parent's
SCHEDULE_CASE = mc.SCHEDULE_CASE


class Prepared:
    """a case ready to run: the problem with the model's float32 weights, the model, the raw unaries and the norms of the oracle"""

    def __init__(self, name, po, wl, pb=None, model_name=None):
        self.name = name
        self.pb, self.cls = (pb, None) if pb is not None else mc.prepared(name, po, wl)
        o = cc.setup(po.OracleCRF, self.pb)
        self.U = o.unary()
        ks = [o.kernel(k) for k in range(len(self.pb["kernels"]))]
        o.close()
        if self.cls is None:
            self.cls = mc.instantiation_class(self.pb["N"], ks) if all(k["d"] == 2 for k in ks) else None
        self.nrm = [k["norm"] for k in ks]
        K, L = len(self.pb["kernels"]), self.pb["L"]
        self.model_name = model_name or CASE_MODEL[name]
        self.modes, self.mats = model(self.model_name, K, L)
        self.w = nc.weights_f32(self.pb, self.nrm, self.modes)   # (a term in mode NONE: scaled by its mean norm)
        self._trace = {}

    def handle(self, pkg, routes=LEARNT):
        """a DenseCRFHIP of the problem under the model; routes: lccrf_set_multilabel_routes' mask"""
        h = cc.setup(pkg.DenseCRFHIP, dict(self.pb, kernels=[(f, w) for (f, _), w in zip(self.pb["kernels"], self.w)]))
        self.put_model(h)
        h.set_multilabel_routes(routes)
        return h

    def put_model(self, h):
        for k, m in enumerate(self.modes):
            h.set_normalization(k, m)
        for k, m in enumerate(self.mats):
            if m is not None:
                h.set_pairwise_compatibility(k, m)

    def expected(self, T, relax=1.0, cap=5):
        """(Q, labels) of the float32 restatement after T iterations: a trace is computed once per relax and shared"""
        key = (float(relax), max(T, cap))
        if key not in self._trace:
            self._trace[key] = nc.restate_trace_f32(self.U, nc.feats(self.pb), self.w, self.mats, self.modes, key[1], relax, self.nrm)
        q = self._trace[key][T]
        return q, ck.map_of(q)


_PREPARED = {}


def prepared(name, po, wl):
    if name not in _PREPARED:
        _PREPARED[name] = Prepared(name, po, wl)
    return _PREPARED[name]


def shape_word(word):
    return mc.shape_word(word)

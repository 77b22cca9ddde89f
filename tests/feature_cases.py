"""The cases of the feature-gradient tests (include/lccrf.h sections 1d / 2d): those of test_gradients_match_the_checker without
the ones built with deliberate lattice ties (the derivative is one-sided there), plus tie-free generic frames of the same
dimensions so that every compiled d = 1 .. 8 is covered (257 points drawn with spread 1.5: at the
golden cases' spread of 4 the points of a d = 8 frame sit alone on their vertices and every feature gradient is rounding noise)."""
import crf_cases as cc

# generic:d1_L3, d3_L21, d5_L2, d6_L3 of cc.CASES are generic_problem(..., lattice_ties=True): replaced by the nt: cases
CASES = ["slam:N5", "slam:N1001", "slam:C3", "generic:multi", "bilateral:c5", "large:c5", "image64x48", "c2",
         "nt:d1_L3", "nt:d3_L21", "nt:d5_L2", "nt:d6_L3", "nt:d4_L5", "nt:d7_L2", "nt:d8_L33", "nt:d2-5-3_L9"]


def gradient_case(name, golden, po, wl):
    """(problem, image or None) of a case of the gradient lists: its twin (crf_cases.GRADIENT_TWINS) where it has one"""
    twin = cc.GRADIENT_TWINS.get(name)
    return twin(golden, po, wl) if twin else case(name, golden, po, wl)


def case(name, golden, po, wl):
    """(problem, image or None)"""
    if name.startswith("nt:"):
        dims, L = name[3:].split("_L")
        return wl.generic_problem(257, [int(d) for d in dims[1:].split("-")], int(L), seed=7, spread=1.5), None
    return cc.case(name, golden, po, wl)

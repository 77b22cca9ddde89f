// frame_engine.hip -- one frame's WHOLE CRF as ONE kernel launch (SURVEY.md section 7's design stance):
// one 1024-lane workgroup per frame builds both permutohedral lattices, normalises both kernels, runs
// startInference, every mean-field iteration and buildMap.  HBM is touched twice: the frame's inputs
// (features of every kernel + labels or unary energies, ~36 KB at N = 2000) are read once, Q and the MAP
// labels (~20 KB) are written once.  Nothing else leaves the CU: the reference's per-frame sequence
//     DenseCRF3D crf(N); crf.setUnaryEnergyFromLabel(..); crf.addPairwiseEnergy(appearanceKernel(..));
//     crf.addPairwiseEnergy(smoothKernel(..)); crf.inference(5, true);            (src/Tracking.cc:1920-1929)
// costs one launch.  L = 2 labels, 2-D kernels, K <= 2, N <= 4096 -- the SLAM configuration; anything else
// (and any frame whose lattices do not fit the LDS plan below) runs on the two-kernel / streaming path with
// identical results.
//
// Lattice construction here is NOT the streaming build's algorithm (stream_build.hip / build_small.hip keep
// the reference's vertex numbering because the parity probes compare offset_/blur_neighbors_ verbatim).  The
// mean-field result does not depend on how vertices are numbered -- a vertex's value is a sum over its OWN
// row in ascending point order, and blur neighbours are found by key -- so this kernel uses whatever
// numbering is cheapest:
//   keys in the table   a 2-D vertex key is two int16 = one 32-bit word: the LDS hash table stores the key
//                       itself (ds_cmpst claims a slot or finds the key; no representative entry, no key
//                       recomputation while probing), permutohedral_cpu.h:66-167,371-377
//   ids by slot order   dense vertex ids = exclusive scan of "slot occupied" (no first-occurrence machinery)
//   neighbours          one lane per vertex probes the same table for key +- 1, permutohedral_cpu.h:408-421
//   row order           a product's place in its vertex's row must follow ascending point index (quirk Q6).
//                       Short rows (the smoothness kernel, ~5 entries per vertex): entries are dropped into
//                       their row in arrival order and every entry counts the smaller entry ids of its row
//                       (one ds_read_b64 per 4 entries).  Long rows (the appearance kernel, ~50 entries per
//                       vertex): a bitmap per vertex over the points; rank = prefix popcount.
//   normalisation       pairwise3d.h:20-28 is one splat/blur/slice of all-ones: the loop's own phases run
//                       once with Q = 1 before startInference (ordered row sums included).
// What must match the reference exactly does: the point records (point_record<2>, quirks Q1-Q4, phantom
// points of the last block of four included), the set of vertices (V is reported and tested against the
// reference's M_), the order of every sum.  ref: permutohedral_cpu.h:241-424,634-699; densecrf_base.h:65-91.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "frame_build.h"
#include "frame_body.h"
#include "fused_lean.h"
#include "dispatch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace lccrf {

namespace {

using namespace fl;
using namespace fb;

// NT = 1024 lanes, or 512 for frames of up to 1024 points whose plan fits half the CU's LDS: two frames per CU
// (fused_loop.h: kNTSmall).  Second launch bound: 128 registers per lane in both shapes.
template <int NT, int PPT, int K, bool DUAL = false>
__global__ void __launch_bounds__(NT, 4) k_frame(CrfDev c, FrameArgs a)
{
    constexpr bool CONV = false;
    const FrameConv fc{};                 // (never read: CONV only)
#include "frame_body.inc"
}

}  // namespace

bool frame_supported(const CrfDev &c, const KernelDev *kds)
{
    const int NA = active_points(c);
    return slam_shaped(c, kds, false) && NA >= 1 && NA <= 4 * kNT;   // (it builds its own tables: any Epad)
}

size_t frame_dual_bytes(int frames) { return (size_t)frames * kDualWords * sizeof(unsigned); }

bool frame_lean_wanted(const CrfDev &c)
{
    return frame_lean_plausible(active_points(c), c.K, c.F);
}
size_t frame_lean_rec_bytes(int frames) { return (size_t)frames * kLeanRecBytes; }

int launch_frame(const CrfDev &c, const KernelDev *kds, const FrameRequest &rq, hipStream_t s)
{
    FrameArgs a = frame_args(c, kds, rq);
    // the forms in units of their own: always one 1024-lane workgroup per frame
    if (rq.run.until_converged || rq.terms.general()) {
        const FrameConv fc{rq.run.criterion, rq.run.tol, rq.out};
        if (!rq.terms.general()) launch_frame_converge(c, a, fc, s);
        else if (rq.run.until_converged) launch_frame_general_converge(c, a, fc, frame_general_terms(c, rq.terms), s);
        else launch_frame_general(c, a, frame_general_terms(c, rq.terms), s);
        return 0;
    }
    a.rec = rq.lean_rec;
    const int NA = active_points(c);
    a.dual = rq.dual;
    a.dual_epoch = rq.dual_epoch;
#if LCCRF_INSTRUMENT
    static const bool drop_helper = ab_env("LCCRF_DUAL_DROP_HELPER") != nullptr;   // fault injection: not compiled into the release library
    a.drop_helper = drop_helper ? 1 : 0;
#endif
    static StampBuffer stamps("LCCRF_FRAME_TIMING", "LCCRF_FRAME_TIMING_LANE", "frame");
    stamps.arm((rq.dual ? 2 : 1) * c.F, kNT, &a.timing, &a.timing_block, &a.timing_lane);   // (two-workgroup form: block 2f is frame f's main workgroup, 2f + 1 its helper)
    // Small frames: 512 lanes and half the CU's LDS per frame, so that two frames share a CU.  A frame whose lattices
    // do not fit that plan (or whose long rows need more chain lanes than four wavefront pairs have) flags itself
    // and is re-run like any other frame that does not fit.
    // The lattice sizes are not known before the kernel has built them: the small shape is chosen when a frame of NA points
    // with lattices of the usual SLAM proportions fits half the LDS in both phases -- an appearance kernel of ~112
    // vertices, a smoothness kernel of min(NA + 350, 1150) (734 vertices at 400 points, 985 at 700, 1071 at 1000 on
    // 640x480 images with an 18-pixel kernel) -- i.e. up to 1024 points.  Frames with larger lattices flag themselves and
    // are re-run; an engine that sees more than 1/8 of a batch flagged stops asking for this shape (allow_small).
    bool small = rq.allow_small && NA <= 2 * kNTSmall && c.F >= kSmallMinFrames;
    if (small) {
        int vest[kMaxFusedK], tables = 0;
        for (int k = 0; k < c.K; ++k) {
            vest[k] = (c.K > 1 && k == 0) ? 112 : std::min(std::min(3 * NA, NA + 350), 1150);
            tables += 2 * (vest[k] + 1) * 8 + kD1 * vest[k] * 4 + (vest[k] + 2) * 2 + 64;
        }
        FusedLayout est;
        const int build_bytes = kHdr + tables + 8 * vest[c.K - 1] + 6 * frame_hcap(NA) + 64;   // tables + vertex keys + counters + hash table
        small = layout_core(NA, c.K, vest, 1 << 20, &est, kNTSmall, kLdsHalf) && build_bytes <= (int)kLdsHalf;
    }
    static const bool no_dual = ab_env("LCCRF_NO_DUAL") != nullptr;         // A/B switch: same results either way
    // Full-size frames (1025 .. 2048 points, the two-kernel SLAM configuration): 512 lanes and half the CU's LDS per frame as well
    // (frame_lean.hip) -- flagged frames and the engine's give-up rule as for the small shape.
    static const bool no_lean = ab_env("LCCRF_NO_FRAME_LEAN") != nullptr;  // A/B switch: same results either way
    const bool lean = rq.lean_rec && !no_lean && frame_lean_plausible(NA, c.K, c.F);
    if (lean) {
        small = false;
        a.lds_total = (int)kLdsHalf;
        launch_frame_lean(c, a, NA, s);
    } else if (rq.dual && !no_dual && c.K == 2 && !small) {                           // a frame alone: two workgroups, one per lattice build
        with_dims<1, 4>((NA + kNT - 1) / kNT, [&](auto p) { launch_workgroups(k_frame<kNT, decltype(p)::value, 2, true>, 2 * c.F, kNT, a.lds_total, s, c, a); });
    } else {
        if (small) a.lds_total = (int)kLdsHalf;
        const int nt = small ? kNTSmall : kNT;
        with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
            constexpr int K = decltype(kk)::value;
            auto go = [&](auto fn) { launch_workgroups(fn, c.F, nt, a.lds_total, s, c, a); };
            if (small) with_dims<1, 2>((NA + nt - 1) / nt, [&](auto p) { go(k_frame<kNTSmall, decltype(p)::value, K>); });
            else with_dims<1, 4>((NA + nt - 1) / nt, [&](auto p) { go(k_frame<kNT, decltype(p)::value, K>); });
        });
    }
    stamps.print(s);                      // instrumented builds: synchronous read-back of one workgroup's stamps
    return lean ? 2 : small ? 1 : 0;
}

}  // namespace lccrf

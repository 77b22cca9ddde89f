// frame_converge.hip -- one frame's WHOLE CRF as one kernel launch (frame_engine.hip), with the inference run UNTIL CONVERGED, at most
// max_iter iterations: include/lccrf.h sections 1i and 2f, notes/convergence.md.
//
// Why: the tracker builds a frame's lattices once and infers on them once (src/Tracking.cc:1920-1929).  For a fixed iteration count
// that is k_frame's one launch; the convergence-driven call of sections 1h / 2e wants lattices in HBM, so a caller who swaps
// "inference(5, true)" for "until the labels settle, at most 12" pays the two-kernel build and a second launch.  Here the frame
// kernel's body (frame_body.inc: inputs, both hash-table lattice builds, normalisation, startInference, store_results) runs the shared
// loop in its convergence form (fused_loop.h: mean_field<..., CONV>, converge_decide): Q_t is bit for bit what k_frame leaves after t
// iterations, the lattices never reach HBM, and the four report words leave with the results, ahead of the done word.
//
// Scope: one 1024-lane workgroup per frame (as with LCCRF_OPT_SINGLE_WORKGROUP), 1 .. 4 points per lane, K in {1, 2}: eight
// instantiations, in a unit of their own so that frame_engine.hip's kernels compile exactly as they did.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "frame_build.h"
#include "frame_body.h"
#include "dispatch.h"

namespace lccrf {

namespace {

using namespace fl;
using namespace fb;

template <int NT, int PPT, int K, bool DUAL = false>
__global__ void __launch_bounds__(NT, 4) k_frame_converge(CrfDev c, FrameArgs a, FrameConv fc)
{
    constexpr bool CONV = true;
#include "frame_body.inc"
}

}  // namespace

namespace fb {
void launch_frame_converge(const CrfDev &c, const FrameArgs &a, const FrameConv &fc, hipStream_t s)
{
    with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
        with_dims<1, 4>((active_points(c) + kNT - 1) / kNT, [&](auto p) {
            launch_workgroups(k_frame_converge<kNT, decltype(p)::value, decltype(kk)::value>, c.F, kNT, a.lds_total, s, c, a, fc);
        });
    });
}
}  // namespace fb

}  // namespace lccrf

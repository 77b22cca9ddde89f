// fused_lean_label.h -- the label-code form of the lean plan's run from prepared records (k_fused_lean_lbl, in a unit of its own:
// fused_lean_label.hip), behind launch_inference() (fused_engine.hip).
#pragma once

#include "fused_loop.h"

namespace lccrf {

// what k_fused_lean<.., MODE 2> takes (fused_engine.hip: FusedArgs), and the codes
struct LeanLabelArgs {
    KernelDev kd[fl::kMaxFusedK];
    fl::FusedLayout lay;
    int n_iter, with_map;
    float relax, omr;                     // omr = 1 - relax (fp32, densecrf3d.h:94), formed on the host
    long long *timing;                    // instrumented builds: shader-clock stamps of one workgroup
    int timing_block, timing_lane;
    int dbg;
    unsigned char *prep;                  // the frames' prepared launch records (fused_lean.h: LeanPrepPlan), prep_stride bytes each
    int prep_stride;
    int Vcap[fl::kMaxFusedK];             // the vertex counts the LDS plan was sized for
    LabelCodes lbl;
};
// one 512-lane workgroup per frame of c, `ppt` (1 .. 4) points per lane; K and chain / short rows from c.K and a.lay.chain0
void launch_lean_label(const CrfDev &c, const LeanLabelArgs &a, int ppt, hipStream_t s);

}  // namespace lccrf

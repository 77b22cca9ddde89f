// frame_general.hip -- one frame's WHOLE CRF as one kernel launch (frame_engine.hip) for the two-label frame whose terms are not all
// Potts terms normalised AFTER the filter: per term an optional 2 x 2 label-compatibility matrix (include/lccrf.h sections 1e / 2g)
// and a normalisation mode (sections 1g / 2g).  Opt-in: LCCRF_OPT_FRAME_GENERAL.  notes/frame_general.md.
//
// Why: a learnt model -- weights, a matrix and a mode per term -- deployed in the tracker builds a frame's lattices once and infers on
// them once (src/Tracking.cc:1920-1929).  Without this unit such a handle or batch leaves the one-launch kernel for the two-kernel
// route: the build launches, the stream synchronisation that learns the lattice sizes, the factor kernels, then k_general.  Here the
// frame kernel's body (frame_body.inc: inputs, both hash-table lattice builds, normalisation, startInference, store_results) runs
// the shared loop in its GEN form (fused_loop.h: mean_field<..., GEN, CONV>), fixed count or until converged: Q_t is bit for bit what
// k_general / k_general_converge leave after t iterations, and the lattices never reach HBM.
//
// The factors.  The body's normalisation holds n = 1 / (t + 1e-20f) in a register per point and term; each term's factors are taken
// from it there with the arithmetic of Engine::ensure_factors() / k_norm_factor (stream_scaled.hip), every operation rounded on its
// own (-ffp-contract=off):
//     AFTER      no pre     post n          wn = w * n
//     BEFORE     pre n      post 1.0f       wn = w * 1.0f
//     SYMMETRIC  pre r      post r          wn = w * r,   r = sqrtf(n)
//     NONE       no pre     post 1.0f       wn = w * 1.0f
// Point slots beyond N keep wn = 0.0f.  The norm itself never depends on mode or matrix.
//
// Scope: one 1024-lane workgroup per frame, 1 or 2 points per lane (the loop keeps PPT * K pre factors in registers: k_general's
// bound), K in {1, 2}: eight instantiations, in a unit of their own so that frame_engine.hip's, frame_lean.hip's and
// frame_converge.hip's kernels compile exactly as they did.  No two-workgroup form and no half-CU form.
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

constexpr int kFrameGeneralMaxPPT = 2;    // points per lane: fused_general.hip's kGeneralMaxPPT

// The body's named places (frame_body.inc), for both kernels below.  `fg` is the kernel's FrameGeneral argument, `off` its offset in
// the argument segment (frame_body.h: kArgOffGeneral, kArgOffGeneralConv): both forms read it where it is used (args_view, the
// body's LATE), as the convergence form reads FrameConv.
#define FRAME_GENERAL_DECLS(off)                                                                                \
    static_assert(!DUAL && NT == kNT && PPT <= kFrameGeneralMaxPPT, "the general form: one 1024-lane workgroup, 1 or 2 points per lane"); \
    GeneralTerms<PPT, K> gt;                                                                                      \
    _Pragma("unroll") for (int s = 0; s < PPT; ++s)                                                              \
        _Pragma("unroll") for (int k = 0; k < K; ++k) gt.pre[s][k] = 0.0f;
// per point s and term k, with the norm n of that point: pre, post and pr.wn = w * post
#define FRAME_GENERAL_FACTORS(off, s, k, n)                                                                       \
    {                                                                                                             \
        const int mode_ = args_view<LATE>(fg, off, kargs).mode[k];                                               \
        const float n_ = (n);                                                                                     \
        float post_ = n_;                                                                                         \
        if (mode_ == LCCRF_NORMALIZE_BEFORE) {                                                                    \
            gt.pre[s][k] = n_;                                                                                    \
            post_ = 1.0f;                                                                                         \
        } else if (mode_ == LCCRF_NORMALIZE_SYMMETRIC) {                                                          \
            post_ = sqrtf(n_);                                                                                    \
            gt.pre[s][k] = post_;                                                                                 \
        } else if (mode_ == LCCRF_NORMALIZE_NONE) {                                                               \
            post_ = 1.0f;                                                                                         \
        }                                                                                                         \
        pr.wn[s][k] = al.w[k] * post_;                                                                            \
    }
// in front of the loop: GeneralTerms' uniform members, from the arguments by value.  The matrices are uniform, and as scalars they
// are eight more registers the loop holds beside its LDS offsets: with all eight there the two-term kernels spill 8 .. 16 scalar
// registers.  They are held in vector registers instead -- all of them at one point per lane, five of the eight at two (term 0's and
// term 1's first: six or eight there cost 2 spilled vector registers, four 3 spilled scalars).  notes/frame_general.md section 3.
#define FRAME_GENERAL_TERMS(off)                                                                                \
    {                                                                                                             \
        const FrameGeneral &fz_ = args_view<LATE>(fg, off, kargs);                                               \
        gt.has_mu = fz_.has_mu;                                                                                   \
        gt.has_pre = 0;                                                                                           \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                          \
            if (fz_.mode[k] == LCCRF_NORMALIZE_BEFORE || fz_.mode[k] == LCCRF_NORMALIZE_SYMMETRIC) gt.has_pre |= 1 << k; \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                      \
                gt.mu[k][e] = fz_.mu[k][e];                                                                       \
                if (PPT == 1 || k == 0 || e < 1) asm volatile("" : "+v"(gt.mu[k][e]));                            \
            }                                                                                                     \
        }                                                                                                         \
    }

// fixed iteration count a.n_iter
template <int NT, int PPT, int K, bool DUAL = false>
__global__ void __launch_bounds__(NT, 4) k_frame_general(CrfDev c, FrameArgs a, FrameGeneral fg)
{
    constexpr bool CONV = false;
    const FrameConv fc{};                 // (never read: CONV only)
#define FRAME_BODY_GEN true
#define FRAME_BODY_GT &gt
#define FRAME_BODY_DECLS FRAME_GENERAL_DECLS(kArgOffGeneral)
#define FRAME_BODY_FACTORS(s, k, n) FRAME_GENERAL_FACTORS(kArgOffGeneral, s, k, n)
#define FRAME_BODY_TERMS FRAME_GENERAL_TERMS(kArgOffGeneral)
#include "frame_body.inc"
}

// until converged, at most a.n_iter iterations
template <int NT, int PPT, int K, bool DUAL = false>
__global__ void __launch_bounds__(NT, 4) k_frame_general_converge(CrfDev c, FrameArgs a, FrameConv fc, FrameGeneral fg)
{
    constexpr bool CONV = true;
#define FRAME_BODY_GEN true
#define FRAME_BODY_GT &gt
#define FRAME_BODY_DECLS FRAME_GENERAL_DECLS(kArgOffGeneralConv)
#define FRAME_BODY_FACTORS(s, k, n) FRAME_GENERAL_FACTORS(kArgOffGeneralConv, s, k, n)
#define FRAME_BODY_TERMS FRAME_GENERAL_TERMS(kArgOffGeneralConv)
#include "frame_body.inc"
}

}  // namespace

// (two ladders, not one that picks the kernel inside: that instantiates the kernels in another order and the unit's code object changes)
namespace fb {
void launch_frame_general(const CrfDev &c, const FrameArgs &a, const FrameGeneral &fg, hipStream_t s)
{
    with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
        with_dims<1, kFrameGeneralMaxPPT>((active_points(c) + kNT - 1) / kNT, [&](auto p) {
            launch_workgroups(k_frame_general<kNT, decltype(p)::value, decltype(kk)::value>, c.F, kNT, a.lds_total, s, c, a, fg);
        });
    });
}

void launch_frame_general_converge(const CrfDev &c, const FrameArgs &a, const FrameConv &fc, const FrameGeneral &fg, hipStream_t s)
{
    with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
        with_dims<1, kFrameGeneralMaxPPT>((active_points(c) + kNT - 1) / kNT, [&](auto p) {
            launch_workgroups(k_frame_general_converge<kNT, decltype(p)::value, decltype(kk)::value>, c.F, kNT, a.lds_total, s, c, a, fc,
                              fg);
        });
    });
}
}  // namespace fb

}  // namespace lccrf

// frame_body.h -- what the kernels built on the one-launch frame body share (frame_engine.hip: k_frame, fixed iteration count;
// frame_converge.hip: k_frame_converge, until converged; frame_general.hip: both for terms with a matrix or a normalisation mode):
// the scan scratch in LDS, the hand-off area of the two-workgroup form, the convergence and the general form's arguments, the hash
// capacity.  The body itself is frame_body.inc.
#pragma once

#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "frame_build.h"

namespace lccrf {
namespace fb {

struct Hdr {                              // lives at smem + 192
    int wave_sum[16];
    int fail;
    int rowmax;
    int dual_ok, dual_V;
    unsigned kargs[2];                    // the convergence form: the argument segment's address (args_view)
};

// DUAL: a single frame (the live tracker's case: one CU busy, 255 idle) is given TWO workgroups -- workgroup 0 builds
// kernel 0's lattice and runs everything else, workgroup 1 (on another CU) builds kernel 1's lattice meanwhile and hands
// its tables (neighbour table, row starts) and per-point records (vertex | row place words, barycentric weights) over
// through this area: 29k of the frame's 157k cycles leave the critical path for ~10k of hand-off.
constexpr int kDualVcap = 8192;                           // vertices of kernel 1 the area can carry (more: the frame falls back)
constexpr int kDualHdr = 16, kDualNbr = kDualHdr, kDualRow = kDualNbr + kD1 * kDualVcap, kDualRec = kDualRow + kDualVcap / 2 + 8,
              kDualWn = kDualRec + 2 * 4 * kD1 * kNT,      // records: (vertex | row place word, barycentric weight) pairs, 8 bytes each
              kDualWords = kDualWn + 4 * kNT;              // w * norm of kernel 1, per point

__device__ __forceinline__ unsigned dual_load(const unsigned *p)       // device-coherent load (the producer ran on another CU / XCD)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long dual_load2(const unsigned *p)   // the same, 8 bytes (p 8-byte aligned)
{
    return __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// CONV: what the convergence form takes beside FrameArgs (whose n_iter is then the cap).  Its reduction needs kConvergeLds bytes
// (fused_loop.h) behind the loop's plan: a frame whose plan leaves no such room under the launch's LDS flags itself unfit, as one
// whose lattices do not fit.
struct FrameConv {
    int criterion;                        // LCCRF_STOP_* bits (1 .. 3)
    float tol;
    ConvergeOut out;                      // [F] each: iterations, delta, changed, converged
};
constexpr int kArgOffConv = (int)((kArgOffA + sizeof(FrameArgs) + alignof(FrameConv) - 1) / alignof(FrameConv) * alignof(FrameConv));
static_assert(alignof(FrameConv) == 8, "k_frame_converge's arguments (CrfDev, FrameArgs, FrameConv) as the ABI lays them out");
// GEN (frame_general.hip): what the general form takes beside FrameArgs -- and, until converged, FrameConv: the terms' label-
// compatibility matrices and normalisation modes (include/lccrf.h sections 1e / 1g / 2g), by value as GeneralArgs carries the matrices.
struct FrameGeneral {
    float mu[kMaxFusedK][4];              // term k's 2 x 2 matrix, row-major (bit k of has_mu; unread otherwise)
    int has_mu;                           // bit k: term k has a matrix
    int mode[kMaxFusedK];                 // lccrf_normalization of term k
};
constexpr int arg_behind(size_t end, size_t align) { return (int)((end + align - 1) / align * align); }
// k_frame_general's arguments are (CrfDev, FrameArgs, FrameGeneral), k_frame_general_converge's (CrfDev, FrameArgs, FrameConv, FrameGeneral)
constexpr int kArgOffGeneral = arg_behind(kArgOffA + sizeof(FrameArgs), alignof(FrameGeneral));
constexpr int kArgOffGeneralConv = arg_behind(kArgOffConv + sizeof(FrameConv), alignof(FrameGeneral));
static_assert(alignof(FrameGeneral) == 4 && sizeof(FrameArgs) % 8 == 0 && sizeof(FrameConv) % 8 == 0 &&
                  kArgOffGeneral == kArgOffA + (int)sizeof(FrameArgs) && kArgOffGeneralConv == kArgOffConv + (int)sizeof(FrameConv),
              "the general frame kernels' arguments as the ABI lays them out: FrameGeneral right behind its predecessor");
// A kernel argument as the body reads it where it is used.  LATE (the convergence form): loaded there, through the argument segment's
// address -- which itself waits in LDS (Hdr::kargs: every wavefront stores it at the kernel's entry and reads back what it stored
// itself, so no barrier is involved), not in a pair of scalar registers for the whole kernel; frame_build.h's late_args is the same
// idea with the address kept in registers.  Otherwise the argument itself.
__device__ __forceinline__ void park_args(unsigned *kargs)
{
    const unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    if ((threadIdx.x & 63) == 0) {
        kargs[0] = (unsigned)p;
        kargs[1] = (unsigned)(p >> 32);
    }
}
template <bool LATE, class T>
__device__ __forceinline__ const T &args_view(const T &direct, int offset, const unsigned *kargs)
{
    if constexpr (LATE) {
        typedef const __attribute__((address_space(4))) unsigned char *kptr;
        const unsigned long long p = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)kargs[0]) |
                                     ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)kargs[1]) << 32);
        return *(const T *)((kptr)p + offset);
    } else {
        return direct;
    }
}

inline int frame_hcap(int NA)
{
    const int live = 3 * ((NA + 3) & ~3);
    int h = 1024;
    while (h < live && h < 8192) h <<= 1;
    return h;
}

// The launch arguments every kernel on the frame body takes (host): one frame per workgroup in the whole of a CU's LDS, no hand-off
// area, no record area -- launch_frame() adds what k_frame's other shapes need.
inline FrameArgs frame_args(const CrfDev &c, const KernelDev *kds, const FrameRequest &rq)
{
    FrameArgs a{};
    for (int k = 0; k < c.K; ++k) {
        a.feat[k] = kds[k].feat;
        a.w[k] = kds[k].w;
        a.V_out[k] = kds[k].V;
    }
    a.scale[0] = kds[0].scale[0];
    a.scale[1] = kds[0].scale[1];
    a.inv_dp1 = kds[0].inv_dp1;
    a.alpha = kds[0].alpha;
    a.maxN = c.maxN;
    a.label = rq.label;
    if (rq.label)
        for (int i = 0; i < 5; ++i) a.tbl[i] = rq.tbl5[i];
    a.n_iter = rq.run.n_iter;
    a.with_map = rq.run.with_map;
    a.relax = rq.run.relax;
    a.omr = 1 - rq.run.relax;
    a.hcap = frame_hcap(active_points(c));
    a.lds_total = (int)kLdsLimit;
    a.status = rq.status;
    a.frame_status = rq.frame_status;
    a.done = c.F == 1 ? rq.done : nullptr;
    a.n_single = (c.F == 1 && rq.done && c.activeN > 0) ? c.activeN : -1;   // (object API: activeN IS the frame's count)
    a.done_epoch = rq.done_epoch;
    return a;
}
// ... and the general form's terms, by value: the matrices and the modes (no mode given: every term AFTER)
inline FrameGeneral frame_general_terms(const CrfDev &c, const TermModel &t)
{
    FrameGeneral g{};
    const int K = c.K < kMaxFusedK ? c.K : kMaxFusedK;
    for (int k = 0; k < K; ++k) g.mode[k] = t.norm_mode ? t.norm_mode[k] : LCCRF_NORMALIZE_AFTER;
    g.has_mu = copy_matrices(t, K, g.mu);
    return g;
}

// The units behind launch_frame() (frame_engine.hip), each with its kernels and its ladder over K and the points per lane: the
// arguments come filled (frame_build.h: launch_frame_lean is the fourth).  One 1024-lane workgroup per frame; the caller has checked
// the frames (frame_supported(), and for the general form at most 2 x 1024 active points -- Engine::frame_ok).
void launch_frame_converge(const CrfDev &c, const FrameArgs &a, const FrameConv &fc, hipStream_t s);
void launch_frame_general(const CrfDev &c, const FrameArgs &a, const FrameGeneral &fg, hipStream_t s);
void launch_frame_general_converge(const CrfDev &c, const FrameArgs &a, const FrameConv &fc, const FrameGeneral &fg, hipStream_t s);

}  // namespace fb
}  // namespace lccrf

// stream_common.h -- what the units of the general ("streaming") engine share.  In that engine every array lives in HBM, there is
// one kernel launch per phase, and the frames of a batch are in grid.y or cut over the XCDs (below).  It handles any N / d / L:
//   stream_build.hip       lattice construction: the hash build, the sorted build of locality mode, CSR rows, neighbour tables
//   stream_filter.hip      splat / blur / slice, the normalisation and the schedule of a mean-field step
//   stream_pointwise.hip   the kernels with a thread per point or per (point, label): unary, softmax, MAP, row copies
//   stream_scaled.hip      the scaled instantiations of the generic splat (stream_splat.h) and the factors of the normalisation modes
#pragma once
#include "engine.h"
#include "dispatch.h"   // with_dims

namespace lccrf {
namespace {

constexpr int kBlock = 256;
constexpr int kSmallFBlock = 64;          // lanes per workgroup of the iteration kernels with one or two frames in flight (iter_block)

// XCD-aware grids.  The chip's eight XCDs have private 4 MB L2s and workgroup L of a launch runs on XCD L % 8 (observed
// dispatch order; used for speed only, never for correctness).  With the frame in blockIdx.y every XCD touches every frame's
// lattice values.  Instead the launch's work -- F frames of nb blocks each, frame after frame -- is cut into EIGHT CONTIGUOUS
// parts of `per` blocks, one per XCD: workgroup L = 8 q + x handles block x per + q of that line.
//   F a multiple of 8      one XCD owns whole frames, and those frames' value arrays (4.7 MB each at C5) are what its L2 sees in
//                          the blur gathers;
//   F < 8                  an XCD handles a contiguous chunk of a frame's row-major vertex range (blur), row range (splat) or point
//                          range (slice): the neighbours a blur gather wants are mostly the centre lines of nearby blocks, i.e.
//                          lines the same L2 is fetching anyway (BASELINE config 5 as written is ONE frame: with the plain grid
//                          consecutive blocks went round-robin over the XCDs and every L2 saw the gathers of the whole array);
//   anything else          (3, 6, 12 frames ...) the same cut: every XCD gets F / 8 of a frame's worth -- frames pinned to
//                          XCDs whole, or to power-of-two groups of them, left a quarter of the chip idle at 3, 6 or 12 frames.
// `nb` = 0 selects the plain (x, frame) grid (empty launches only).
struct XcdMap { int nb, per; };
struct FrameBlock { int f, bx; };
__device__ __forceinline__ FrameBlock frame_block(XcdMap m)
{
    if (m.nb == 0) return FrameBlock{(int)blockIdx.y, (int)blockIdx.x};
    const int L = blockIdx.x, xcd = L & 7, q = L >> 3;
    const int idx = xcd * m.per + q, f = idx / m.nb;
    return FrameBlock{f, idx - f * m.nb};                 // (the last XCD's tail lies beyond frame F - 1: the kernels' own range check)
}
// lanes per workgroup of the iteration kernels: 256; with one or two frames in flight a pass is a chain of latencies and smaller
// workgroups drain sooner (scripts/ubench/phasecost.hip: 256 -> 64 lanes 6.8 -> 6.4 us per pass of one C5 frame; in the engine,
// 256 -> 64 lanes: one frame 41.0 -> 40.2 us per iteration, two 32.8 -> 32.1, four +-0)
inline int iter_block(int F)
{
    return F <= 2 ? kSmallFBlock : 256;
}
inline dim3 grid_xcd(long work, int F, XcdMap *m, int block = 256)
{
    const long n = (work + block - 1) / block;
    if (n < 1) { *m = XcdMap{0, 1}; return dim3(1u, (unsigned)F); }
    static const bool no_chunk = ab_env("LCCRF_NO_XCD_CHUNK") != nullptr;   // A/B switch (same results): plain (x, frame) grid below 8 frames
    if (no_chunk && F < 8) { *m = XcdMap{0, 1}; return dim3((unsigned)n, (unsigned)F); }
    const long per = (n * F + 7) / 8;
    *m = XcdMap{(int)n, (int)per};
    return dim3((unsigned)(8L * per));
}

inline dim3 grid_for(long work, int F)
{
    const long nb = (work + kBlock - 1) / kBlock;
    return dim3((unsigned)(nb > 0 ? nb : 1), (unsigned)F);   // empty frames still get a (no-op) block
}

}  // namespace
}  // namespace lccrf

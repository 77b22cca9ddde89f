// device_inputs.hip -- the object API's device-array inputs (include/lccrf.h section 1b): a pairwise term's features, taken from
// the caller's device array or formed from an image the way PottsPotentialCPU<M,F>::FromImage forms them (pairwise_cpu.h:33-51),
// are written into the handle's own feature buffer (KernelState::feat_own), [N][d] AoS -- the layout every lattice build reads.
//
// Only N*d values are written.  The builds never read a point at or beyond N for its value: the phantom points of quirk Q1 get
// their zeros inside the builds (stream_build.hip, build_small.hip, frame_build.h: "phantom lanes, :299"), exactly as for the
// host path, which uploads N*d values as well.  This kernel is the only reader of the caller's array, and it reads [0, N) only.
//
// Bit parity with the reference's host loop rests on two things: `(float)` of a pixel coordinate below 2^24 is exact, and the
// division is the IEEE, correctly rounded one (a plain `/`: the Makefile builds without -ffast-math, with -ffp-contract=off, and
// hipcc rounds fp32 division correctly by default).
#include "engine.h"

namespace lccrf {

namespace {

constexpr int kStageBlock = 256;

// one thread per output value (point i, dimension j); i < n by construction of the grid guard
__global__ void __launch_bounds__(kStageBlock) k_stage_features(float *__restrict__ dst, const void *__restrict__ src, long n, int d,
                                                                int mode, int width, float posdev, float featuredev)
{
    const long idx = (long)blockIdx.x * kStageBlock + threadIdx.x;
    if (idx >= n * d) return;
    if (mode == kStageCopy) {
        dst[idx] = static_cast<const float *>(src)[idx];
        return;
    }
    const long i = idx / d;
    const int j = (int)(idx - i * d);
    float v;
    if (j == 0) {
        v = (float)(int)(i % width) / posdev;                      // allFeatures[idx*F+0] = (float)wi / posdev
    } else if (j == 1) {
        v = (float)(int)(i / width) / posdev;                      // allFeatures[idx*F+1] = (float)hi / posdev
    } else {
        const long p = i * (d - 2) + (j - 2);                      // features[idx*(F-2) + (i-2)]
        v = (mode == kStageImageU8 ? (float)static_cast<const unsigned char *>(src)[p] : static_cast<const float *>(src)[p]) / featuredev;
    }
    dst[idx] = v;
}

}  // namespace

void launch_stage_features(float *dst, const void *src, int n, int d, int mode, int width, float posdev, float featuredev,
                           hipStream_t s)
{
    const long total = (long)n * d;
    if (total <= 0) return;
    const unsigned blocks = (unsigned)((total + kStageBlock - 1) / kStageBlock);
    k_stage_features<<<blocks, kStageBlock, 0, s>>>(dst, src, (long)n, d, mode, width, posdev, featuredev);
}

}  // namespace lccrf

// fused_backward_common.h -- what the one-launch backward kernels share: k_backward (fused_backward.hip: Potts terms normalised
// AFTER), k_backward_general (fused_backward_general.hip: learnt models and dL/dmu) and k_backward_features
// (fused_backward_features.hip: with feature gradients).  Device functions and the sizes of the LDS the kernels keep behind the loop's
// plan; each kernel lives in a unit of its own.
#pragma once

#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"

namespace lccrf {
namespace {

constexpr int kBackwardMaxPPT = 2;        // points per lane
constexpr int kPartialRows = 256;         // points per partial of the weight gradient: k_softmax_bwd's workgroup at L <= 4
constexpr int kWaves = fl::kNT / 64;
// behind the loop's plan: the wavefronts' sums of one iteration [K][PPT][16], and the reduction's accumulators [K][256]
constexpr int kBackwardLds = (fl::kMaxFusedK * kBackwardMaxPPT * kWaves + fl::kMaxFusedK * kPartialRows) * (int)sizeof(float);

// gamma of one row at L = 2 as softmax_bwd<1, .> forms it (meanfield_backward.hip): the row maximum, fast_exp_nonpos(x - mx), the
// label-ordered row sum, p = e / tt, G of the first largest label, the deviation in label order
__device__ __forceinline__ float2 gamma2(float x0, float x1, const float2 g, float relax)
{
    float mx = -INFINITY;
    if (mx < x0) mx = x0;
    if (mx < x1) mx = x1;
    const float e0 = fast_exp_nonpos(x0 - mx), e1 = fast_exp_nonpos(x1 - mx);
    float tt = 0.0f;
    tt += e0;
    tt += e1;
    float ga = 0.0f;
    if (x0 == mx) ga = g.x;
    else if (x1 == mx) ga = g.y;
    const float p0 = e0 / tt, p1 = e1 / tt;
    const float gp0 = p0 * (g.x - ga), gp1 = p1 * (g.y - ga);
    float dev = 0.0f;
    dev += gp0;
    dev += gp1;
    return make_float2(relax * (p0 * ((g.x - ga) - dev)), relax * (p1 * ((g.y - ga) - dev)));
}

// slice_point with the sum started at a literal 0.0f, as slice_value starts it (stream_filter.hip)
template <int PPT, int K>
__device__ __forceinline__ float2 slice_signed(const unsigned char *smem, const fl::FusedLayout &lay, const fl::PointRegs<PPT, K> &pr, int s,
                                               int k, float alpha)
{
    const float2 *val = reinterpret_cast<const float2 *>(smem + lay.val[k][fl::kD1 & 1]);
    const float2 x0 = val[pr.ix[s][k][0] & 0xffffu], x1 = val[pr.ix[s][k][0] >> 16], x2 = val[pr.ix[s][k][1] & 0xffffu];
    const float w0 = pr.bary[s][k][0] * alpha, w1 = pr.bary[s][k][1] * alpha, w2 = pr.bary[s][k][2] * alpha;
    float t0 = 0.0f, t1 = 0.0f;
    t0 += w0 * x0.x; t1 += w0 * x0.y;
    t0 += w1 * x1.x; t1 += w1 * x1.y;
    t0 += w2 * x2.x; t1 += w2 * x2.y;
    return make_float2(t0, t1);
}

// ... which also hands out the three gathered vertex values x[c] (before alpha): what k_corner_dot dots a row with (k_backward_features)
template <int PPT, int K>
__device__ __forceinline__ float2 slice_signed_corners(const unsigned char *smem, const fl::FusedLayout &lay, const fl::PointRegs<PPT, K> &pr,
                                                       int s, int k, float alpha, float2 (&x)[fl::kD1])
{
    const float2 *val = reinterpret_cast<const float2 *>(smem + lay.val[k][fl::kD1 & 1]);
    x[0] = val[pr.ix[s][k][0] & 0xffffu];
    x[1] = val[pr.ix[s][k][0] >> 16];
    x[2] = val[pr.ix[s][k][1] & 0xffffu];
    const float w0 = pr.bary[s][k][0] * alpha, w1 = pr.bary[s][k][1] * alpha, w2 = pr.bary[s][k][2] * alpha;
    float t0 = 0.0f, t1 = 0.0f;
    t0 += w0 * x[0].x; t1 += w0 * x[0].y;
    t0 += w1 * x[1].x; t1 += w1 * x[1].y;
    t0 += w2 * x[2].x; t1 += w2 * x[2].y;
    return make_float2(t0, t1);
}

}  // namespace
}  // namespace lccrf

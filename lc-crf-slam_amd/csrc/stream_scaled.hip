// stream_scaled.hip -- the streaming engine's kernels behind the normalisation modes (include/lccrf.h section 1g): the scaled
// instantiations of the generic splat (stream_splat.h, PRE = true) and the kernel that forms a term's per-point factors.
// Compiled with -ffp-contract=off, no -ffast-math: as stream_filter.hip.
#include "stream_splat.h"

namespace lccrf {
namespace {

// the per-point factor of a term that is not normalised AFTER: s[i] = sqrtf(n[i]) (SYMMETRIC; hipcc rounds sqrtf correctly unless
// told otherwise, and the Makefile does not tell it) or 1.0f (what the slice reads for a term with no factor behind the filter:
// w * 1.0f is exact).  The ones fill the whole stride, whatever the frame's point count is or becomes.
__global__ void __launch_bounds__(kBlock) k_norm_factor(CrfDev c, const float *__restrict__ norm, float *__restrict__ out, int root)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.maxN) return;
    const size_t q = (size_t)f * c.maxN + i;
    if (!root) out[q] = 1.0f;
    else if (i < c.n_points[f]) out[q] = sqrtf(norm[q]);
}

}  // namespace

void launch_norm_factor(const CrfDev &c, const float *norm, float *out, int root, hipStream_t s)
{
    k_norm_factor<<<grid_for(c.maxN, c.F), kBlock, 0, s>>>(c, norm, out, root);
}

// launch_splat (stream_filter.hip) with the input rows scaled by pre [F][kd.maxN]: the same choice of kernels, the same grids
void launch_splat_scaled(const KernelDev &kd, const float *in, int in_stride, int L, int F, int maxV, const float *pre, hipStream_t s)
{
    if (L >= 4 && splat_short_rows(kd, maxV)) k_splat4<true><<<grid_for((long)maxV * ((L + 3) / 4), F), kBlock, 0, s>>>(kd, in, in_stride, L, (L + 3) / 4, pre);
    else k_splat<true><<<grid_for((long)maxV * L, F), kBlock, 0, s>>>(kd, in, in_stride, L, pre);
    if (kd.longrow_ok) k_splat_long<true><<<splat_long_grid(F), kBlock, 0, s>>>(kd, in, in_stride, L, pre);
}

}  // namespace lccrf

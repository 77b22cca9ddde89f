// stream_pointwise.hip -- the streaming engine's kernels with a thread per point or per (point, label), and their launchers.
// Compiled with -ffp-contract=off: the reference is an SSE2 build without FMA, so every a*b+c must stay two roundings.
// No -ffast-math: fp32 division must be IEEE (V/=tt), denormals are kept (gfx950 default).
// Reference being restated (paths under the reference's Thirdparty/DenseCRF/include/):
//   expAndNormalize        densecrf3d.h:51-98            -> k_softmax
//   buildMap               densecrf3d.h:136-151          -> k_map
#include "stream_common.h"
#include "device_math.h"
#include <algorithm>

namespace lccrf {
namespace {

// unary[i][:] from a label and the three energy tables {u, n[L], p[L]}.  densecrf3d.h:116-129.
// codes (two labels, or null): the point's code -- 0 / 1 its label, 2 unknown -- beside its energies; pairs: by code the negated
// energy pair, then Q0 = softmax(-energies) with the inference kernels' own arithmetic (softmax2_fresh), kLabelPairFloats floats.
__global__ void __launch_bounds__(kBlock) k_unary_from_label_tbl(CrfDev c, const int16_t *__restrict__ label, UnaryTable tbl,
                                                                 unsigned char *__restrict__ codes, float *__restrict__ pairs)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (pairs && f == 0 && idx < 3) {         // (code `idx`; L == 2)
        const float a = idx == 2 ? tbl.v[0] : idx == 0 ? tbl.v[3] : tbl.v[2], b = idx == 2 ? tbl.v[0] : idx == 0 ? tbl.v[1] : tbl.v[4];
        const float2 q0 = softmax2_fresh(-a, -b);
        pairs[2 * idx] = -a;
        pairs[2 * idx + 1] = -b;
        pairs[6 + 2 * idx] = q0.x;
        pairs[6 + 2 * idx + 1] = q0.y;
    }
    if (idx >= c.n_points[f] * c.L) return;
    const int i = idx / c.L, m = idx - i * c.L;
    const int t = label[(size_t)f * c.maxN + (c.perm ? c.perm[(size_t)f * c.perm_stride + i] : i)];
    float u;
    if (t < 0 || t >= c.L) u = tbl.v[0];      // -1 = unknown; out-of-range labels (UB in the reference) likewise
    else u = (m == t) ? tbl.v[1 + c.L + t] : tbl.v[1 + t];
    c.unary[((size_t)f * c.maxN + i) * c.L + m] = u;
    if (codes && m == 0) codes[(size_t)f * c.maxN + i] = (t < 0 || t >= c.L) ? 2 : (unsigned char)t;
}

// out = softmax_fe(scale * in) (blended with the old out when relax != 1).
__global__ void __launch_bounds__(kBlock) k_softmax(CrfDev c, const float *__restrict__ in,
                                                    float *__restrict__ out, float scale, float relax)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.n_points[f]) return;
    const size_t q = ((size_t)f * c.maxN + i) * c.L;
    exp_and_normalize_row(in + q, out + q, c.L, scale, relax);
}

// ... for 3 to 32 labels with a LANE PER (point, label): a wavefront takes 64 / L consecutive points, whose rows are one contiguous
// block (coalesced loads and stores, no staging); the row maximum and the row sum are formed by every lane of the row from the
// others' values (__shfl) -- the sum in label order 0 .. L-1, one add at a time, as densecrf3d.h:80-84 forms it; each lane's
// exponential is computed once instead of twice (the same argument gives the same bits).  The lane-per-point kernel above reads
// rows L floats apart (64 lines per load) and runs 2 L exponentials per lane: L = 21 x 76 800 points 34 us, through LDS 26, this 24
// (L = 8: 7 us) -- 2 L lane-indexed reads per wavefront through the LDS crossbar are what is left.
constexpr int kSoftmaxMaxL = 32;
__global__ void __launch_bounds__(kBlock) k_softmax_rows(CrfDev c, const float *__restrict__ in, float *__restrict__ out, float scale, float relax)
{
    const int f = blockIdx.y, L = c.L;
    const int N = c.n_points[f];
    const int rpw = 64 / L;                               // rows per wavefront
    const int lane = threadIdx.x & 63, wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int row = lane / L, j = lane - row * L, i = wave * rpw + row;
    const bool live = row < rpw && i < N;
    const size_t q = ((size_t)f * c.maxN + (live ? i : 0)) * L + (live ? j : 0);
    const float s = live ? scale * in[q] : 0.0f;
    const int first = row * L;                            // the row's first lane
    // (the others' values eight at a time: a lane-indexed read is an LDS-crossbar round trip of ~100 cycles)
    float mx = __shfl(s, first, 64);
    for (int t0 = 1; t0 < L; t0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __shfl(s, first + min(t0 + u, L - 1), 64);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < L && mx < v[u]) mx = v[u];
    }
    const float e = fast_exp_nonpos(s - mx);              // (value - row maximum <= 0: the branch-free form, same bits)
    float tt = 0;
    for (int t0 = 0; t0 < L; t0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __shfl(e, first + min(t0 + u, L - 1), 64);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < L) tt += v[u];
    }
    if (!live) return;
    const float v = e / tt;
    if (relax == 1) out[q] = v;
    else out[q] = (1 - relax) * out[q] + relax * v;
}

// next = -unary (DenseCRF3D::stepInit, densecrf3d.h:154-158) into an arbitrary buffer
__global__ void __launch_bounds__(kBlock) k_step_init(CrfDev c, float *__restrict__ out)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= c.n_points[f] * c.L) return;
    const size_t q = (size_t)f * c.maxN * c.L + idx;
    out[q] = -c.unary[q];
}

__global__ void __launch_bounds__(kBlock) k_map(CrfDev c, const float *__restrict__ Q, int16_t *__restrict__ map)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int N = c.n_points[f];
    int lab = 0;
    if (i < N) {
        const float *p = Q + ((size_t)f * c.maxN + i) * c.L;
        lab = argmax_row(p, c.L);
        map[(size_t)f * c.maxN + i] = (int16_t)lab;
    }
    if (c.map_bits && map == c.map && c.L == 2 && (i >> 6) < c.bits_stride) {   // one bit per label: the label gather's wire format
        const unsigned long long m = __ballot(lab == 1);                           // (words beyond the frame's points: 0)
        if ((threadIdx.x & 63) == 0) c.map_bits[(size_t)f * c.bits_stride + (i >> 6)] = m;
    }
}

__global__ void __launch_bounds__(kBlock) k_validate_npoints(const int *__restrict__ in, int *__restrict__ out, int F,
                                                             int maxN, int *bad)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const int n = in[f], c = min(max(n, 0), maxN);
    out[f] = c;
    if (c != n) *bad = 1;
}

}  // namespace

void launch_unary_from_label_tbl(const CrfDev &c, const int16_t *label, const UnaryTable &tbl, hipStream_t s, unsigned char *codes,
                                 float *pairs)
{
    const bool lbl = codes && pairs && c.L == 2;
    k_unary_from_label_tbl<<<grid_for((long)c.maxN * c.L, c.F), kBlock, 0, s>>>(c, label, tbl, lbl ? codes : nullptr, lbl ? pairs : nullptr);
}

void launch_exp_and_normalize(const CrfDev &c, const float *in, float *out, float scale, float relax, hipStream_t s)
{
    if (c.L >= 3 && c.L <= kSoftmaxMaxL) {
        const int per_block = (kBlock / 64) * (64 / c.L);   // points per workgroup
        k_softmax_rows<<<dim3((unsigned)((c.maxN + per_block - 1) / per_block), (unsigned)c.F), kBlock, 0, s>>>(c, in, out, scale, relax);
    } else {
        k_softmax<<<grid_for(c.maxN, c.F), kBlock, 0, s>>>(c, in, out, scale, relax);
    }
}

void launch_start(const CrfDev &c, hipStream_t s) { launch_exp_and_normalize(c, c.unary, c.Q, -1.0f, 1.0f, s); }   // densecrf_base.h:78-80

void launch_validate_npoints(const int *in, int *out, int F, int maxN, int *bad, hipStream_t s)
{
    k_validate_npoints<<<(F + kBlock - 1) / kBlock, kBlock, 0, s>>>(in, out, F, maxN, bad);
}

void launch_map(const CrfDev &c, hipStream_t s) { launch_map_of(c, c.Q, c.map, s); }

// ---- the protected virtuals of DenseCRF on caller-chosen device buffers (launch_exp_and_normalize above is the third) ------
void launch_map_of(const CrfDev &c, const float *prob, int16_t *map, hipStream_t s)
{
    k_map<<<grid_for(c.maxN, c.F), kBlock, 0, s>>>(c, prob, map);
}

void launch_step_init(const CrfDev &c, float *out, hipStream_t s)
{
    k_step_init<<<grid_for((long)c.maxN * c.L, c.F), kBlock, 0, s>>>(c, out);
}

// dst[i][:] = src[list[i]][:] (gather) or dst[list[i]][:] = src[i][:] (scatter), rows of `units` elements of type T
template <typename T>
__global__ void __launch_bounds__(kBlock) k_copy_frames(T *__restrict__ dst, size_t dst_stride, const T *__restrict__ src,
                                                        size_t src_stride, const int *__restrict__ list, size_t units, int gather)
{
    const int i = blockIdx.y, f = list[i];
    const T *sp = src + (gather ? (size_t)f : (size_t)i) * src_stride;
    T *dp = dst + (gather ? (size_t)i : (size_t)f) * dst_stride;
    for (size_t w = (size_t)blockIdx.x * kBlock + threadIdx.x; w < units; w += (size_t)gridDim.x * kBlock) dp[w] = sp[w];
}

void launch_copy_frames(void *dst, size_t dst_stride, const void *src, size_t src_stride, const int *list, int n_list,
                        size_t bytes, int gather, hipStream_t s)
{
    if (n_list <= 0 || bytes == 0) return;
    const bool w4 = ((bytes | dst_stride | src_stride | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src) & 3) == 0;
    const size_t units = bytes / (w4 ? 4 : 2);                                 // (every per-frame array is at least int16-aligned)
    const unsigned gx = (unsigned)std::min<size_t>((units + kBlock - 1) / kBlock, 64);
    const dim3 g(gx, (unsigned)n_list);
    if (w4)
        k_copy_frames<unsigned><<<g, kBlock, 0, s>>>(static_cast<unsigned *>(dst), dst_stride / 4, static_cast<const unsigned *>(src),
                                                     src_stride / 4, list, units, gather);
    else
        k_copy_frames<unsigned short><<<g, kBlock, 0, s>>>(static_cast<unsigned short *>(dst), dst_stride / 2,
                                                           static_cast<const unsigned short *>(src), src_stride / 2, list, units, gather);
}

__global__ void __launch_bounds__(kBlock) k_permute_rows(CrfDev c, float *__restrict__ dst, const float *__restrict__ src, int width,
                                                         int gather)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= c.n_points[f] * width) return;
    const int i = idx / width, m = idx - i * width;
    const int o = c.perm[(size_t)f * c.perm_stride + i];
    const size_t a = ((size_t)f * c.maxN + i) * width + m, b = ((size_t)f * c.maxN + o) * width + m;
    if (gather) dst[a] = src[b];
    else dst[b] = src[a];
}

void launch_permute_rows(const CrfDev &c, float *dst, const float *src, int width, int gather, hipStream_t s)
{
    k_permute_rows<<<grid_for((long)c.maxN * width, c.F), kBlock, 0, s>>>(c, dst, src, width, gather);
}

}  // namespace lccrf

// stream_splat.h -- the generic (L-label) splat kernels of the streaming engine, shared by the two units that instantiate them:
// stream_filter.hip (PRE = false: the filter as the reference has it) and stream_scaled.hip (PRE = true: the input rows multiplied
// by a per-point factor where they are loaded, include/lccrf.h section 1g).
// Compiled with -ffp-contract=off: every a*b+c stays two roundings.
// Reference being restated: splat, permutohedral_cpu.h:634-699.
#pragma once
#include "stream_common.h"
#include <algorithm>

namespace lccrf {
namespace {

// val0[v+1][l] = sum over the vertex's contributions, ascending point order.  in == nullptr
// means the all-ones input of the normalisation pass (pairwise3d.h:23-24).
constexpr int kSplatUnroll = 16;
typedef float lccrf_f4u __attribute__((ext_vector_type(4), aligned(4)));     // four labels of a row, wherever L puts them
// PRE (include/lccrf.h section 1g: a term normalised BEFORE or SYMMETRICally): every input row is multiplied by its point's factor
// pre[pt] where it is loaded, xv = pre[pt] * in[pt][l] rounded once, and acc += w * xv as ever -- no scaled copy of `in` in HBM.
// pre: [F][kd.maxN], laid out as KernelDev::norm; `in` is not null then.  PRE = false is the code it was (pre is not read).
template <bool PRE>
__global__ void __launch_bounds__(kBlock) k_splat(KernelDev kd, const float *__restrict__ in,
                                                  int in_stride, int L, const float *__restrict__ pre)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * L) return;
    const int v = idx / L, l = idx - v * L;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
    if (kd.longrow_ok && t - s > kLongRowMin && kd.longcnt[f] <= kLongRowCap) return;   // k_splat_long's
    const float *x = in ? in + (size_t)f * in_stride : nullptr;
    const float *ps = PRE ? pre + (size_t)f * kd.maxN : nullptr;
    float acc = 0.0f;
    int p = s;
    // long rows (a coarse kernel over many points: the reference's image demo has rows of ~900 entries): the adds must go one by one
    // in point order, the LOADS need not -- kSplatUnroll entries' indices, weights and inputs in flight per round trip instead of one
    // (the demo's splat 944 -> ~100 us per launch)
    for (; p + kSplatUnroll <= t; p += kSplatUnroll) {
        int pt[kSplatUnroll];
        float w[kSplatUnroll], xv[kSplatUnroll];
#pragma unroll
        for (int i = 0; i < kSplatUnroll; ++i) { pt[i] = kd.csr_pt[fe + p + i]; w[i] = kd.csr_w[fe + p + i]; }
#pragma unroll
        for (int i = 0; i < kSplatUnroll; ++i) xv[i] = x ? x[(size_t)pt[i] * L + l] : 1.0f;
        if constexpr (PRE) {
            float sc[kSplatUnroll];
#pragma unroll
            for (int i = 0; i < kSplatUnroll; ++i) sc[i] = ps[pt[i]];
#pragma unroll
            for (int i = 0; i < kSplatUnroll; ++i) xv[i] = sc[i] * xv[i];
        }
#pragma unroll
        for (int i = 0; i < kSplatUnroll; ++i) acc += w[i] * xv[i];
    }
    for (; p < t; ++p) {
        float xv = x ? x[(size_t)kd.csr_pt[fe + p] * L + l] : 1.0f;
        if constexpr (PRE) xv = ps[kd.csr_pt[fe + p]] * xv;
        acc += kd.csr_w[fe + p] * xv;
    }
    kd.val0[(size_t)f * kd.vstride + kd.vbase + (long)v * L + l] = acc;
}

// ... four labels per thread from L = 4 on: a row's indices and weights are read once per four labels, the inputs as 16-byte loads
template <bool PRE>
__global__ void __launch_bounds__(kBlock) k_splat4(KernelDev kd, const float *__restrict__ in, int in_stride, int L, int C,
                                                   const float *__restrict__ pre)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * C) return;
    const int v = idx / C, l = (idx - v * C) * 4, nl = min(4, L - l);
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
    if (kd.longrow_ok && t - s > kLongRowMin && kd.longcnt[f] <= kLongRowCap) return;   // k_splat_long's
    const float *x = in + (size_t)f * in_stride + l;
    const float *ps = PRE ? pre + (size_t)f * kd.maxN : nullptr;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int U = 8;
    int p = s;
    if (nl == 4) {
        for (; p + U <= t; p += U) {
            int pt[U];
            float w[U];
            lccrf_f4u xv[U];
#pragma unroll
            for (int i = 0; i < U; ++i) { pt[i] = kd.csr_pt[fe + p + i]; w[i] = kd.csr_w[fe + p + i]; }
#pragma unroll
            for (int i = 0; i < U; ++i) xv[i] = *reinterpret_cast<const lccrf_f4u *>(x + (size_t)pt[i] * L);
            if constexpr (PRE) {
                float sc[U];
#pragma unroll
                for (int i = 0; i < U; ++i) sc[i] = ps[pt[i]];
#pragma unroll
                for (int i = 0; i < U; ++i) { xv[i].x = sc[i] * xv[i].x; xv[i].y = sc[i] * xv[i].y; xv[i].z = sc[i] * xv[i].z; xv[i].w = sc[i] * xv[i].w; }
            }
#pragma unroll
            for (int i = 0; i < U; ++i) { acc[0] += w[i] * xv[i].x; acc[1] += w[i] * xv[i].y; acc[2] += w[i] * xv[i].z; acc[3] += w[i] * xv[i].w; }
        }
        for (; p < t; ++p) {
            const float w = kd.csr_w[fe + p];
            lccrf_f4u xv = *reinterpret_cast<const lccrf_f4u *>(x + (size_t)kd.csr_pt[fe + p] * L);
            if constexpr (PRE) {
                const float sc = ps[kd.csr_pt[fe + p]];
                xv.x = sc * xv.x; xv.y = sc * xv.y; xv.z = sc * xv.z; xv.w = sc * xv.w;
            }
            acc[0] += w * xv.x; acc[1] += w * xv.y; acc[2] += w * xv.z; acc[3] += w * xv.w;
        }
    } else {
        for (; p < t; ++p) {
            const float w = kd.csr_w[fe + p];
            const float *xp = x + (size_t)kd.csr_pt[fe + p] * L;
            if constexpr (PRE) {
                const float sc = ps[kd.csr_pt[fe + p]];
                for (int u = 0; u < nl; ++u) acc[u] += w * (sc * xp[u]);
            } else {
                for (int u = 0; u < nl; ++u) acc[u] += w * xp[u];
            }
        }
    }
    float *d = kd.val0 + (size_t)f * kd.vstride + kd.vbase + (long)v * L + l;
    for (int u = 0; u < nl; ++u) d[u] = acc[u];
}

// Rows of thousands of entries (a coarse kernel over many points -- the appearance kernel of the reference's image demo puts whole
// uniformly coloured regions on one vertex): the adds of a row must still go one by one in point order (quirk Q6), but nothing says
// the LOADS must.  A workgroup per listed row (KernelDev::longrow, filled by the build): all lanes form the products
// w[p] * in[pt[p]][l] of a tile of entries in LDS, then lane l < L adds its label's column top to bottom -- the same products, the
// same order, the same bits as the in-line walk.
constexpr int kLongTile = 8192;          // products per tile (floats); two tiles in LDS
template <bool PRE>
__global__ void __launch_bounds__(kBlock) k_splat_long(KernelDev kd, const float *__restrict__ in, int in_stride, int L,
                                                       const float *__restrict__ pre)
{
    __shared__ __attribute__((aligned(16))) float prod[2][kLongTile];
    const int f = blockIdx.y;
    const int *lr = kd.longrow + (size_t)f * kLongRowCap;
    const int n = kd.longcnt[f];
    if (n > kLongRowCap) return;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const float *x = in ? in + (size_t)f * in_stride : nullptr;
    const float *ps = PRE ? pre + (size_t)f * kd.maxN : nullptr;
    // a tile holds ec entries of every label, label-major: prod[l * ecp + e] (ecp = ec + 4, a multiple of 4: the adder reads its
    // label's column four entries per 16-byte LDS load; the loaders' stores land ecp words apart -- a few ways of bank conflict)
    const int tid = threadIdx.x, ec = (kLongTile / L - 4) & ~3, ecp = ec + 4;
    constexpr int kLoaders = kBlock - 64;                 // wavefront 0 adds, the other three load: the tile being added and the tile
    for (int i = blockIdx.x; i < n; i += gridDim.x) {     // being loaded are different halves of `prod`, one barrier per tile
        const int v = lr[i];
        const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
        const int ntiles = (t - s + ec - 1) / ec;
        float acc = 0.0f;
        for (int k = -1; k < ntiles; ++k) {
            if (tid >= 64) {                              // load tile k + 1
                const int p0 = s + (k + 1) * ec;
                const int m = k + 1 < ntiles ? min(ec, t - p0) * L : 0;
                float *dst = prod[(k + 1) & 1];
                int idx = tid - 64;
                for (; idx + 7 * kLoaders < m; idx += 8 * kLoaders) {        // eight products per lane and round trip
                    int pt[8], l[8], e[8];
                    float w[8], xv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        e[u] = (idx + u * kLoaders) / L;
                        l[u] = idx + u * kLoaders - e[u] * L;
                        pt[u] = kd.csr_pt[fe + p0 + e[u]];
                        w[u] = kd.csr_w[fe + p0 + e[u]];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) xv[u] = x ? x[(size_t)pt[u] * L + l[u]] : 1.0f;
                    if constexpr (PRE) {
                        float sc[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) sc[u] = ps[pt[u]];
#pragma unroll
                        for (int u = 0; u < 8; ++u) xv[u] = sc[u] * xv[u];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) dst[l[u] * ecp + e[u]] = w[u] * xv[u];
                }
                for (; idx < m; idx += kLoaders) {
                    const int e = idx / L, l = idx - e * L;
                    float xv = x ? x[(size_t)kd.csr_pt[fe + p0 + e] * L + l] : 1.0f;
                    if constexpr (PRE) xv = ps[kd.csr_pt[fe + p0 + e]] * xv;
                    dst[l * ecp + e] = kd.csr_w[fe + p0 + e] * xv;
                }
            } else if (k >= 0 && tid < L) {               // add tile k: label tid's column, top to bottom
                const int p0 = s + k * ec;
                const int m = min(ec, t - p0);
                const float *src = prod[k & 1] + tid * ecp;
                int e = 0;
                for (; e + 8 <= m; e += 8) {
                    const float4 q0 = *reinterpret_cast<const float4 *>(src + e), q1 = *reinterpret_cast<const float4 *>(src + e + 4);
                    acc += q0.x; acc += q0.y; acc += q0.z; acc += q0.w;
                    acc += q1.x; acc += q1.y; acc += q1.z; acc += q1.w;
                }
                for (; e < m; ++e) acc += src[e];
            }
            __syncthreads();
        }
        if (tid < L) kd.val0[(size_t)f * kd.vstride + kd.vbase + (long)v * L + tid] = acc;
    }
}

// which of the two in-line kernels a term takes, and the grid of the workgroup-per-row kernel: one rule for both units
inline bool splat_short_rows(const KernelDev &kd, int maxV) { return (long)kd.maxN * kd.D1 <= 4L * std::max(maxV, 1); }
inline dim3 splat_long_grid(int F) { return dim3((unsigned)std::max(256 / std::max(F, 1), 8), (unsigned)F); }

}  // namespace
}  // namespace lccrf

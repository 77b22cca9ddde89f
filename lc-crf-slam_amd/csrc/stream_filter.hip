// stream_filter.hip -- the permutohedral filter of the streaming engine (stream_common.h): splat, blur and slice for any label
// count, the two-label specialisations of the SLAM configuration, and the host schedule that picks among them.
// Compiled with -ffp-contract=off: the reference is an SSE2 build without FMA, so every a*b+c must stay two roundings.
// No -ffast-math: fp32 division must be IEEE (1/(norm+1e-20)), denormals are kept (gfx950 default).
// Reference being restated (paths under the reference's Thirdparty/DenseCRF/include/):
//   splat / blur / slice   permutohedral_cpu.h:634-699   -> k_splat / k_blur / k_slice
//   normalisation          pairwise3d.h:20-28            -> launch_norm
//   apply                  pairwise3d.h:73-78            -> k_slice (mode APPLY)
//   stepInit               densecrf3d.h:154-158          -> k_slice (first kernel)
#include "stream_common.h"
#include "stream_splat.h"
#include "device_math.h"
#include <algorithm>

namespace lccrf {
namespace {

// ---------------------------------------------------------------------------------------
// splat / blur / slice  (value width L at run time; one thread per (vertex|point, label))
// ---------------------------------------------------------------------------------------

// the generic splat: rows in line, the long ones by a workgroup each
// pre (optional; with `in` only): the per-point factor of the input rows, [F][kd.maxN] (section 1g) -- the scaled instantiations,
// which live in stream_scaled.hip
inline void launch_splat(const KernelDev &kd, const float *in, int in_stride, int L, int F, int maxV, hipStream_t s,
                         const float *pre = nullptr)
{
    // four labels per thread where the rows are short (a fine lattice: about one entry per vertex at d = 5 or 6); a coarse kernel's
    // rows of tens to hundreds of entries want every (vertex, label) walk in flight on its own (the image demo: 344 vs 554 us)
    const bool short_rows = splat_short_rows(kd, maxV);
    if (in && pre) { launch_splat_scaled(kd, in, in_stride, L, F, maxV, pre, s); return; }
    if (L >= 4 && in && short_rows) k_splat4<false><<<grid_for((long)maxV * ((L + 3) / 4), F), kBlock, 0, s>>>(kd, in, in_stride, L, (L + 3) / 4, nullptr);
    else k_splat<false><<<grid_for((long)maxV * L, F), kBlock, 0, s>>>(kd, in, in_stride, L, nullptr);
    if (kd.longrow_ok) k_splat_long<false><<<splat_long_grid(F), kBlock, 0, s>>>(kd, in, in_stride, L, nullptr);
}

// One Jacobi blur pass along axis j.  ref: :663-679.
__global__ void __launch_bounds__(kBlock) k_blur(KernelDev kd, const float *__restrict__ src,
                                                 float *__restrict__ dst, int j, int L)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * L) return;
    const int v = idx / L, l = idx - v * L;
    const size_t fv = (size_t)f * kd.vstride;
    const int2 nb = reinterpret_cast<const int2 *>(kd.nbr)[((size_t)f * kd.D1 + j) * kd.Epad + v];
    const float *o = src + fv + kd.vbase;      // o[v*L+l], v = -1 is the all-zero "absent" vertex
    const float a = o[(long)nb.x * L + l];
    const float c = o[(long)nb.y * L + l];
    dst[fv + kd.vbase + (long)v * L + l] = o[(long)v * L + l] + 0.5f * (a + c);
}

// ... four labels per thread from L = 4 on (16-byte accesses on 4-byte alignment: a vertex's row starts wherever L puts it): the
// pass at L = 21 is bound by instructions per byte, not by bytes (55 us per 558 000 vertices against 18 at the streaming rate).
__global__ void __launch_bounds__(kBlock) k_blur4(KernelDev kd, const float *__restrict__ src, float *__restrict__ dst, int j, int L, int C)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * C) return;
    const int v = idx / C, l = (idx - v * C) * 4;         // C = ceil(L / 4) chunks per vertex
    const size_t fv = (size_t)f * kd.vstride;
    const int2 nb = reinterpret_cast<const int2 *>(kd.nbr)[((size_t)f * kd.D1 + j) * kd.Epad + v];
    const float *o = src + fv + kd.vbase;                 // o[v*L+l], v = -1 is the all-zero "absent" vertex
    float *d = dst + fv + kd.vbase + (long)v * L + l;
    const float *pa = o + (long)nb.x * L + l, *pc = o + (long)nb.y * L + l, *po = o + (long)v * L + l;
    if (l + 4 <= L) {
        const lccrf_f4u a = *reinterpret_cast<const lccrf_f4u *>(pa), c = *reinterpret_cast<const lccrf_f4u *>(pc),
                        m = *reinterpret_cast<const lccrf_f4u *>(po);
        lccrf_f4u r;
        r.x = m.x + 0.5f * (a.x + c.x);
        r.y = m.y + 0.5f * (a.y + c.y);
        r.z = m.z + 0.5f * (a.z + c.z);
        r.w = m.w + 0.5f * (a.w + c.w);
        *reinterpret_cast<lccrf_f4u *>(d) = r;
    } else {
        for (int u = 0; u < L - l; ++u) d[u] = po[u] + 0.5f * (pa[u] + pc[u]);
    }
}

// ... and ONE label (the normalisation's filter of all-ones, pairwise3d.h:22-27: seven passes per build): four vertices per thread --
// two 16-byte table loads, one 16-byte centre load, eight 4-byte gathers, one 16-byte store instead of four times (8 + 4 + 2 x 4 + 4).
typedef int lccrf_i4u __attribute__((ext_vector_type(4), aligned(4)));
__global__ void __launch_bounds__(kBlock) k_blur1x4(KernelDev kd, const float *__restrict__ src, float *__restrict__ dst, int j)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int v = 4 * (blockIdx.x * kBlock + threadIdx.x);
    if (v >= V) return;
    const size_t fv = (size_t)f * kd.vstride;
    const float *o = src + fv + kd.vbase;                 // o[-1] = the all-zero "absent" vertex
    float *d = dst + fv + kd.vbase;
    const int *nbp = kd.nbr + (((size_t)f * kd.D1 + j) * kd.Epad + v) * 2;
    if (v + 4 <= V) {
        const lccrf_i4u n0 = *reinterpret_cast<const lccrf_i4u *>(nbp), n1 = *reinterpret_cast<const lccrf_i4u *>(nbp + 4);
        const lccrf_f4u c = *reinterpret_cast<const lccrf_f4u *>(o + v);
        const float a0 = o[n0.x], b0 = o[n0.y], a1 = o[n0.z], b1 = o[n0.w], a2 = o[n1.x], b2 = o[n1.y], a3 = o[n1.z], b3 = o[n1.w];
        lccrf_f4u r;
        r.x = c.x + 0.5f * (a0 + b0);
        r.y = c.y + 0.5f * (a1 + b1);
        r.z = c.z + 0.5f * (a2 + b2);
        r.w = c.w + 0.5f * (a3 + b3);
        *reinterpret_cast<lccrf_f4u *>(d + v) = r;
    } else {
        for (int u = v; u < V; ++u) d[u] = o[u] + 0.5f * (o[nbp[2 * (u - v)]] + o[nbp[2 * (u - v) + 1]]);
    }
}

enum SliceMode { SLICE_NORM = 0, SLICE_APPLY_FIRST = 1, SLICE_APPLY = 2, SLICE_PLAIN = 3 };

// the sliced value of (point i, label l): sum over the point's corners of (bary * alpha) * value.  ref: :684-694.
__device__ __forceinline__ float slice_value(const KernelDev &kd, const float *__restrict__ vf, size_t fe, int i, int l, int L)
{
    float t = 0.0f;
    // (every corner's id and weight, then every gather, before the first use: one round trip per level instead of one per corner)
    int o[kMaxD + 1];
    float wgt[kMaxD + 1], x[kMaxD + 1];
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < kd.D1) { o[j] = kd.offset[fe + (size_t)i * kd.D1 + j]; wgt[j] = kd.bary[fe + (size_t)i * kd.D1 + j] * kd.alpha; }
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < kd.D1) x[j] = vf[(long)o[j] * L + l];
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < kd.D1) t += wgt[j] * x[j];
    return t;
}

// slice (+ what the caller does with it).  ref: :684-694, pairwise3d.h:25-27,73-78,
// densecrf3d.h:154-158.
__global__ void __launch_bounds__(kBlock) k_slice(KernelDev kd, CrfDev c, const float *__restrict__ val,
                                                  int L, int mode)
{
    const int f = blockIdx.y;
    const int N = c.n_points[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= N * L) return;
    const int i = idx / L, l = idx - i * L;
    const size_t fe = (size_t)f * kd.Epad;
    const float *vf = val + (size_t)f * kd.vstride + kd.vbase;
    const float t = slice_value(kd, vf, fe, i, l, L);
    if (mode == SLICE_NORM) {
        kd.norm[(size_t)f * kd.maxN + i] = 1.0f / (t + 1e-20f);
    } else if (mode == SLICE_PLAIN) {                      // the bare filter: out = compute(in), permutohedral_cpu.h:634-699
        c.next[((size_t)f * c.maxN + i) * L + l] = t;
    } else {
        const size_t q = ((size_t)f * c.maxN + i) * L + l;
        const float base = (mode == SLICE_APPLY_FIRST) ? -c.unary[q] : c.next[q];
        c.next[q] = base + kd.w * kd.norm[(size_t)f * kd.maxN + i] * t;
    }
}

// The slice of a term with a label-compatibility matrix mu [L][L] (include/lccrf.h section 1e), in the same launch:
//   next[i][l] = base + w * norm[i] * s,   s = 0; for l' = 0 .. L-1: s = s + mu[l][l'] * t[i][l']
// with t[i][l'] the value k_slice forms (slice_value) and every product and sum rounded on its own (-ffp-contract=off): an identity
// matrix gives k_slice's bits.  The sliced values never go to HBM: a workgroup owns kCompatGroups groups of R = 256 / L consecutive
// points, lane r * L + l of a group forms t[r][l] into LDS, and behind one barrier the same lane sums row l of mu (in LDS too)
// against the point's L values.  Row strides of mu and of the tile are odd (L | 1): ds_read_b32 serves 32 lanes per cycle from 32
// banks, lanes with the same l (or the same point) read one address (a broadcast), and the up to 32 different rows a lane group
// walks at one column l' fall on different banks.
constexpr int kCompatGroups = 4;
constexpr int kCompatTile = kBlock + kBlock / 2;           // R * (L | 1) <= 256 + R, R <= 128 (L = 2; L = 1: R = 256 rows of one)
__global__ void __launch_bounds__(kBlock) k_slice_compat(KernelDev kd, CrfDev c, const float *__restrict__ val,
                                                         const float *__restrict__ compat, int L, int mode)
{
    __shared__ float mu[LCCRF_MAX_LABELS * (LCCRF_MAX_LABELS + 1)];
    __shared__ float tile[kCompatGroups][kCompatTile];
    const int f = blockIdx.y;
    const int N = c.n_points[f];
    const int R = kBlock / L, ms = L | 1, ts = L == 1 ? 1 : (L | 1);
    const int tid = threadIdx.x;
    const int r = tid / L, l = tid - r * L;
    const int i0 = blockIdx.x * (kCompatGroups * R) + r;
    if (i0 - r >= N) return;                              // (the whole workgroup: no barrier is left behind)
    for (int idx = tid; idx < L * L; idx += kBlock) {
        const int a = idx / L;
        mu[a * ms + (idx - a * L)] = compat[idx];
    }
    const size_t fe = (size_t)f * kd.Epad;
    const float *vf = val + (size_t)f * kd.vstride + kd.vbase;
#pragma unroll
    for (int g = 0; g < kCompatGroups; ++g) {
        const int i = i0 + g * R;
        if (r < R && i < N) tile[g][r * ts + l] = slice_value(kd, vf, fe, i, l, L);
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kCompatGroups; ++g) {
        const int i = i0 + g * R;
        if (r >= R || i >= N) continue;
        const float *m = mu + l * ms, *t = tile[g] + r * ts;
        float s = 0.0f;
        for (int lp = 0; lp < L; ++lp) s = s + m[lp] * t[lp];
        const size_t q = ((size_t)f * c.maxN + i) * L + l;
        const float base = (mode == SLICE_APPLY_FIRST) ? -c.unary[q] : c.next[q];
        c.next[q] = base + kd.w * kd.norm[(size_t)f * kd.maxN + i] * s;
    }
}

inline void launch_slice_apply(const KernelDev &kd, const CrfDev &c, const float *res, int L, int mode, const float *compat, hipStream_t s)
{
    if (compat) {
        const long per = (long)kCompatGroups * (kBlock / L);
        k_slice_compat<<<dim3((unsigned)std::max((c.maxN + per - 1) / per, 1L), (unsigned)c.F), kBlock, 0, s>>>(kd, c, res, compat, L, mode);
    } else {
        k_slice<<<grid_for((long)c.maxN * L, c.F), kBlock, 0, s>>>(kd, c, res, L, mode);
    }
}

// the normalisation's slice with d + 1 known at compile time: every load of a point issued before the first use (the generic kernel
// above walks its corners one dependent gather at a time: 92 -> 35 us per 8 C5 frames).  Same operations, same order.
template <int D1>
__global__ void __launch_bounds__(kBlock) k_slice_norm(KernelDev kd, CrfDev c, const float *__restrict__ val)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.n_points[f]) return;
    const size_t fe = (size_t)f * kd.Epad;
    const float *vf = val + (size_t)f * kd.vstride + kd.vbase;
    int o[D1];
    float w[D1], x[D1];
#pragma unroll
    for (int j = 0; j < D1; ++j) { o[j] = kd.offset[fe + (size_t)i * D1 + j]; w[j] = kd.bary[fe + (size_t)i * D1 + j]; }
#pragma unroll
    for (int j = 0; j < D1; ++j) x[j] = vf[o[j]];
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < D1; ++j) t += (w[j] * kd.alpha) * x[j];
    kd.norm[(size_t)f * kd.maxN + i] = 1.0f / (t + 1e-20f);
}

// ---- two-label specialisations (the SLAM configuration, L = 2): one thread per vertex / point,
// both labels in a float2.  Same operations per label as the generic kernels above.
// (by value: `ok ? lds[i] : zero` selects between two ADDRESSES and parks the zero in scratch memory)
__device__ __forceinline__ float2 lds_or_zero(bool ok, const float2 *p)
{
    float2 r = make_float2(0.0f, 0.0f);                   // what the absent vertex's slot holds
    if (ok) r = *p;
    return r;
}

// The two-label splat of a COARSE kernel over many points (KernelDev::long_mode: a 2-D smoothness kernel on 100 000 points has 2000
// vertices and rows of 150 entries on average): eight entries' loads per round trip, the adds in order; the listed rows are left to
// k_splat_long (L = 2: the same value layout).  8 frames of C5 never come here (1.2 entries per row).
__global__ void __launch_bounds__(kBlock) k_splat2l(KernelDev kd, const float2 *__restrict__ in, int in_stride, int F, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int v = fb.bx * (int)blockDim.x + threadIdx.x;
    if (v >= kd.V[f]) return;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
    if (kd.longrow_ok && t - s > kLongRowMin && kd.longcnt[f] <= kLongRowCap) return;   // k_splat_long's
    const float2 *x = in + (size_t)f * in_stride;
    float a0 = 0.0f, a1 = 0.0f;
    int p = s;
    for (; p + 8 <= t; p += 8) {
        int pt[8];
        float w[8];
        float2 q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { pt[i] = kd.csr_pt[fe + p + i]; w[i] = kd.csr_w[fe + p + i]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = x[pt[i]];
#pragma unroll
        for (int i = 0; i < 8; ++i) { a0 += w[i] * q[i].x; a1 += w[i] * q[i].y; }
    }
    for (; p < t; ++p) {
        const float w = kd.csr_w[fe + p];
        const float2 q = x[kd.csr_pt[fe + p]];
        a0 += w * q.x;
        a1 += w * q.y;
    }
    reinterpret_cast<float2 *>(kd.val0 + (size_t)f * kd.vstride + kd.vbase)[v] = make_float2(a0, a1);
}

// ... and with rows of tens of entries on average (long_mode 2) a WAVEFRONT per vertex: its 64 lanes load 64 entries' products in one
// round trip (coalesced index / weight reads, one gather), then every lane adds them in order off the others' registers (a uniform
// lane index: v_readlane) -- two interleaved chains, one per label.  2000 vertices x 150 entries: 45 -> ~6 us.
__global__ void __launch_bounds__(kBlock) k_splat2v(KernelDev kd, const float2 *__restrict__ in, int in_stride, int F, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int lane = threadIdx.x & 63;
    const int v = fb.bx * ((int)blockDim.x / 64) + (threadIdx.x >> 6);      // (grid: one wavefront per vertex)
    if (v >= kd.V[f]) return;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
    if (kd.longrow_ok && t - s > kLongRowMin && kd.longcnt[f] <= kLongRowCap) return;   // k_splat_long's
    const float2 *x = in + (size_t)f * in_stride;
    float a0 = 0.0f, a1 = 0.0f;
    for (int base = s; base < t; base += 64) {
        const int p = base + lane, m = min(64, t - base);
        float p0 = 0.0f, p1 = 0.0f;
        if (p < t) {
            const float w = kd.csr_w[fe + p];
            const float2 q = x[kd.csr_pt[fe + p]];
            p0 = w * q.x;
            p1 = w * q.y;
        }
        for (int u = 0; u < m; ++u) {                     // (u is uniform: v_readlane, no trip through the LDS crossbar)
            a0 += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), u));
            a1 += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), u));
        }
    }
    if (lane == 0) reinterpret_cast<float2 *>(kd.val0 + (size_t)f * kd.vstride + kd.vbase)[v] = make_float2(a0, a1);
}

// BLUR0 (sorted build, KernelDev::fast0_ok): the FIRST blur pass rides along.  Axis 0 is the fastest coordinate of the row-major
// vertex code, so a vertex's axis-0 neighbours are v - 1 and v + 1 (or absent): the workgroup's row sums go to LDS -- every thread
// sums one row, the first and the last only for their neighbours' sake (blockDim - 2 results per workgroup) -- and
// t[v] = s[v] + 0.5 (s[n1] + s[n2]) is formed from there: the operations of k_blur2 on the stored sums, in the same order, hence the
// same bits, without the pass's launch, its table-to-gather round trip and its 16 bytes per vertex of reads and writes.
template <bool BLUR0>
__global__ void __launch_bounds__(kBlock) k_splat2(KernelDev kd, const float2 *__restrict__ in, int in_stride, int F, XcdMap nb)
{
    __shared__ float2 tile[BLUR0 ? kBlock : 1];
    __shared__ uint8_t next[BLUR0 ? kBlock : 1];
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int v0 = BLUR0 ? fb.bx * ((int)blockDim.x - 2) - 1 : fb.bx * (int)blockDim.x;      // the vertex of thread 0
    const int v = v0 + threadIdx.x;
    if (v0 + (BLUR0 ? 1 : 0) >= V) return;                // (the whole workgroup)
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const float2 *x = in + (size_t)f * in_stride;
    float a0 = 0.0f, a1 = 0.0f;
    uint8_t nx = 0;
    if (v >= 0 && v < V) {
        const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
        if (BLUR0) nx = kd.fastn[fe + v];
        for (int p = s; p < t; ++p) {
            const float w = kd.csr_w[fe + p];
            const float2 q = x[kd.csr_pt[fe + p]];
            a0 += w * q.x;
            a1 += w * q.y;
        }
    }
    float2 *out = reinterpret_cast<float2 *>(kd.val0 + (size_t)f * kd.vstride + kd.vbase);
    if (!BLUR0) {
        if (v < V) out[v] = make_float2(a0, a1);
        return;
    }
    tile[threadIdx.x] = make_float2(a0, a1);
    next[threadIdx.x] = nx;
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == blockDim.x - 1 || v >= V) return;
    const float2 p = lds_or_zero(next[threadIdx.x - 1], &tile[threadIdx.x - 1]), q = lds_or_zero(nx, &tile[threadIdx.x + 1]);   // n1 = v - 1, n2 = v + 1
    out[v] = make_float2(a0 + 0.5f * (p.x + q.x), a1 + 0.5f * (p.y + q.y));
}

// ... and the passes along axes 1 (and 2) too, when the sorted build found their neighbours within a few ids (KernelDev::ndist): an
// OVERLAPPED window.  A workgroup sums the rows of B consecutive vertices into LDS and runs the passes 0 .. P-1 there; a neighbour
// outside the window reads as zero, which spoils its neighbours' values pass by pass -- by at most `halo` = 1 + dist_1 (+ dist_2)
// positions from either end, so the inner B - 2 halo results are exactly what P launches of k_blur2 would have stored (the same
// operations on the same values in the same order) and only those are written.  One launch, one table read per extra pass.
template <int LANES, int U>
__global__ void __launch_bounds__(LANES) k_splat2w(KernelDev kd, const float2 *__restrict__ in, int in_stride, int F, XcdMap nb, int P, int halo)
{
    constexpr int B = LANES * U;                          // the window: U vertices per lane, at stride LANES (coalesced)
    __shared__ float2 buf[2][B];
    __shared__ uint8_t next[B];
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int v0 = fb.bx * (B - 2 * halo) - halo;         // the window's first vertex
    if (v0 + halo >= V) return;                           // (the whole workgroup)
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const float2 *x = in + (size_t)f * in_stride;
    const char2 *off1 = reinterpret_cast<const char2 *>(kd.nearoff) + (size_t)f * 2 * kd.Epad, *off2 = off1 + kd.Epad;   // axes 1, 2
    const int tid = threadIdx.x;
    float a0[U], a1[U];
    char2 o1[U], o2[U];
    uint8_t nx[U];
    int s[U], t[U];
    int pt0[U];
    float w0[U];
    float2 q0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int v = v0 + tid + u * LANES;
        const bool live = v >= 0 && v < V;
        s[u] = t[u] = 0;
        nx[u] = 0;
        o1[u] = o2[u] = make_char2(0, 0);
        if (live) {
            s[u] = kd.rowptr[f1 + v];
            t[u] = kd.rowptr[f1 + v + 1];
            nx[u] = kd.fastn[fe + v];
            o1[u] = off1[v];
            if (P > 2) o2[u] = off2[v];
        }
    }
    // the first entry of each of the lane's U rows together (rows hold 1.2 entries on average: most are done after this), then
    // whatever is left of each row in order
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool any = s[u] < t[u];
        pt0[u] = any ? kd.csr_pt[fe + s[u]] : 0;
        w0[u] = any ? kd.csr_w[fe + s[u]] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) q0[u] = x[pt0[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float b0 = 0.0f, b1 = 0.0f;
        if (s[u] < t[u]) {
            b0 += w0[u] * q0[u].x;
            b1 += w0[u] * q0[u].y;
        }
        for (int p = s[u] + 1; p < t[u]; ++p) {
            const float w = kd.csr_w[fe + p];
            const float2 q = x[kd.csr_pt[fe + p]];
            b0 += w * q.x;
            b1 += w * q.y;
        }
        a0[u] = b0;
        a1[u] = b1;
        buf[0][tid + u * LANES] = make_float2(b0, b1);
        next[tid + u * LANES] = nx[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {                         // pass 0: n1 = v - 1, n2 = v + 1
        const int i = tid + u * LANES;
        const float2 p = lds_or_zero(i > 0 && next[i > 0 ? i - 1 : 0], &buf[0][i > 0 ? i - 1 : 0]);
        const float2 q = lds_or_zero(nx[u] && i + 1 < B, &buf[0][i + 1 < B ? i + 1 : i]);
        a0[u] = a0[u] + 0.5f * (p.x + q.x);
        a1[u] = a1[u] + 0.5f * (p.y + q.y);
        buf[1][i] = make_float2(a0[u], a1[u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {                         // pass 1 (P >= 2)
        const int i = tid + u * LANES;
        const unsigned i1 = (unsigned)(i + o1[u].x), i2 = (unsigned)(i + o1[u].y);
        const float2 p = lds_or_zero(o1[u].x != 0 && i1 < (unsigned)B, &buf[1][i1 < (unsigned)B ? i1 : 0]);
        const float2 q = lds_or_zero(o1[u].y != 0 && i2 < (unsigned)B, &buf[1][i2 < (unsigned)B ? i2 : 0]);
        a0[u] = a0[u] + 0.5f * (p.x + q.x);
        a1[u] = a1[u] + 0.5f * (p.y + q.y);
    }
    if (P > 2) {                                          // pass 2 (buf[0] was last read before the barrier above)
#pragma unroll
        for (int u = 0; u < U; ++u) buf[0][tid + u * LANES] = make_float2(a0[u], a1[u]);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * LANES;
            const unsigned i1 = (unsigned)(i + o2[u].x), i2 = (unsigned)(i + o2[u].y);
            const float2 p = lds_or_zero(o2[u].x != 0 && i1 < (unsigned)B, &buf[0][i1 < (unsigned)B ? i1 : 0]);
            const float2 q = lds_or_zero(o2[u].y != 0 && i2 < (unsigned)B, &buf[0][i2 < (unsigned)B ? i2 : 0]);
            a0[u] = a0[u] + 0.5f * (p.x + q.x);
            a1[u] = a1[u] + 0.5f * (p.y + q.y);
        }
    }
    float2 *out = reinterpret_cast<float2 *>(kd.val0 + (size_t)f * kd.vstride + kd.vbase);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = tid + u * LANES, v = v0 + i;
        if (i >= halo && i < B - halo && v < V) out[v] = make_float2(a0[u], a1[u]);
    }
}

typedef int lccrf_v4i __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ int4 load_nbr_pair(const int *p)
{
    const lccrf_v4i x = NT ? __builtin_nontemporal_load(reinterpret_cast<const lccrf_v4i *>(p)) : *reinterpret_cast<const lccrf_v4i *>(p);
    return make_int4(x.x, x.y, x.z, x.w);
}
// Two vertices per thread: the neighbour pairs (int4), the centres (float4) and the results (float4) move as 16-byte
// accesses (the frame's value array is laid out so that vertex 2t is 16-byte aligned, see Engine::add_kernel).
// What bounds the pass is the CU's vector-memory path, not HBM bytes: an 8-byte gather costs ~16 + 2 cycles per distinct
// 128-byte line it touches (scripts/ubench/tacost.hip), which is why locality mode -- fewer distinct lines per gather --
// helps and why everything tried on top of it lost (notes/r3_experiments.md: 2-8 pairs per lane with all loads issued
// first, a presence-bit + id-list neighbour table, a 4096/8192-vertex LDS tile serving the in-tile neighbours).
// NT: the neighbour table is read once per pass -- with many frames in flight (a working set beyond every cache) it is
// loaded non-temporally, out of the value array's way in L2; with a few frames everything lives in L2 / the Infinity Cache
// and the plain load is the faster one (scripts/ubench/phasecost.hip: 7.2 -> 6.8 us per pass of one C5 frame).
template <bool NT>
__global__ void __launch_bounds__(kBlock) k_blur2(KernelDev kd, const float *__restrict__ src,
                                                  float *__restrict__ dst, int j, int F, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int v = 2 * (fb.bx * (int)blockDim.x + threadIdx.x);
    if (v >= V) return;
    const float2 *o = reinterpret_cast<const float2 *>(src + (size_t)f * kd.vstride + kd.vbase);   // o[-1] = absent
    float2 *d = reinterpret_cast<float2 *>(dst + (size_t)f * kd.vstride + kd.vbase);
    const int *nbp = kd.nbr + (((size_t)f * kd.D1 + j) * kd.Epad + v) * 2;
    if (v + 1 < V) {
        const int4 nb4 = load_nbr_pair<NT>(nbp);
        const float4 c = *reinterpret_cast<const float4 *>(o + v);
        const float2 x0 = o[nb4.x], y0 = o[nb4.y], x1 = o[nb4.z], y1 = o[nb4.w];
        *reinterpret_cast<float4 *>(d + v) = make_float4(c.x + 0.5f * (x0.x + y0.x), c.y + 0.5f * (x0.y + y0.y),
                                                         c.z + 0.5f * (x1.x + y1.x), c.w + 0.5f * (x1.y + y1.y));
    } else {
        const int2 n2 = *reinterpret_cast<const int2 *>(nbp);
        const float2 c = o[v], x = o[n2.x], y = o[n2.y];
        d[v] = make_float2(c.x + 0.5f * (x.x + y.x), c.y + 0.5f * (x.y + y.y));
    }
}

// The same pass off the COMPACT neighbour table of the sorted build (KernelDev::nbrc): 4 instead of 8 table bytes per vertex, the
// ids rebuilt as base-of-the-block + 16-bit offset (0xffff = absent -> -1).  Same neighbours, same operations, same bits.
// (No non-temporal form: the table exists with up to kNbrcMaxFrames frames in flight, below kBlurNtMinFrames -- engine.h.)
__global__ void __launch_bounds__(kBlock) k_blur2c(KernelDev kd, const float *__restrict__ src,
                                                   float *__restrict__ dst, int j, int F, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int v = 2 * (fb.bx * (int)blockDim.x + threadIdx.x);
    if (v >= V) return;
    const float2 *o = reinterpret_cast<const float2 *>(src + (size_t)f * kd.vstride + kd.vbase);   // o[-1] = absent
    float2 *d = reinterpret_cast<float2 *>(dst + (size_t)f * kd.vstride + kd.vbase);
    const size_t fj = (size_t)f * kd.D1 + j;
    const int2 base = reinterpret_cast<const int2 *>(kd.nbrc_base)[fj * (kd.Epad / kNbrcBlock + 1) + v / kNbrcBlock];
    const unsigned *tp = reinterpret_cast<const unsigned *>(kd.nbrc) + fj * kd.Epad + v;            // (v even: 8-byte aligned)
    if (v + 1 < V) {
        typedef unsigned lccrf_v2u __attribute__((ext_vector_type(2)));
        const lccrf_v2u t = *reinterpret_cast<const lccrf_v2u *>(tp);
        const unsigned a0 = t.x & 0xffffu, b0 = t.x >> 16, a1 = t.y & 0xffffu, b1 = t.y >> 16;
        const int n0 = a0 == 0xffffu ? -1 : base.x + (int)a0, m0 = b0 == 0xffffu ? -1 : base.y + (int)b0;
        const int n1 = a1 == 0xffffu ? -1 : base.x + (int)a1, m1 = b1 == 0xffffu ? -1 : base.y + (int)b1;
        const float4 c = *reinterpret_cast<const float4 *>(o + v);
        const float2 x0 = o[n0], y0 = o[m0], x1 = o[n1], y1 = o[m1];
        *reinterpret_cast<float4 *>(d + v) = make_float4(c.x + 0.5f * (x0.x + y0.x), c.y + 0.5f * (x0.y + y0.y),
                                                         c.z + 0.5f * (x1.x + y1.x), c.w + 0.5f * (x1.y + y1.y));
    } else {
        const unsigned t = *tp, a0 = t & 0xffffu, b0 = t >> 16;
        const int n0 = a0 == 0xffffu ? -1 : base.x + (int)a0, m0 = b0 == 0xffffu ? -1 : base.y + (int)b0;
        const float2 c = o[v], x = o[n0], y = o[m0];
        d[v] = make_float2(c.x + 0.5f * (x.x + y.x), c.y + 0.5f * (x.y + y.y));
    }
}

// TWO passes (axes j, j + 1) in one launch, no extra tables -- for one or two frames in flight, where a pass is a chain of
// latencies (launch ~2.5 us, table load, gather: ~7 us per pass of one C5 frame against ~0.5 us of streaming) and every launch
// saved counts: out[v] = t[v] + 0.5 (t[a] + t[b]) with {a, b} = the axis-(j+1) neighbours of v and
// t[x] = s[x] + 0.5 (s[n1_j(x)] + s[n2_j(x)]) recomputed for x = v, a, b.  The same operations in the same order as two
// launches of k_blur2 (permutohedral_cpu.h:663-679), hence the same bits; the absent vertex (-1) has no neighbours and
// t[-1] = 0 + 0.5 (0 + 0) = 0 exactly, which is what the separate passes leave in its slot.  9 gathers instead of 4, a
// three-level chain instead of twice two levels + a launch: 13.6 -> 10.3 us per pair of passes (scripts/ubench/phasecost.hip).
__global__ void __launch_bounds__(kBlock) k_blur2x2(KernelDev kd, const float *__restrict__ src, float *__restrict__ dst, int j, int F, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int v = fb.bx * (int)blockDim.x + threadIdx.x;
    if (v >= kd.V[f]) return;
    const float2 *o = reinterpret_cast<const float2 *>(src + (size_t)f * kd.vstride + kd.vbase);   // o[-1] = absent
    float2 *d = reinterpret_cast<float2 *>(dst + (size_t)f * kd.vstride + kd.vbase);
    const int2 *nj = reinterpret_cast<const int2 *>(kd.nbr) + ((size_t)f * kd.D1 + j) * kd.Epad;
    const int2 *nj1 = nj + kd.Epad;
    const int2 ab = nj1[v], nv = nj[v];
    const float2 sv = o[v];
    const int2 na = ab.x >= 0 ? nj[ab.x] : make_int2(-1, -1), nbb = ab.y >= 0 ? nj[ab.y] : make_int2(-1, -1);
    const float2 sa = o[ab.x], sb = o[ab.y], v1 = o[nv.x], v2 = o[nv.y];
    const float2 a1 = o[na.x], a2 = o[na.y], b1 = o[nbb.x], b2 = o[nbb.y];
    const float2 tv = make_float2(sv.x + 0.5f * (v1.x + v2.x), sv.y + 0.5f * (v1.y + v2.y));
    const float2 ta = make_float2(sa.x + 0.5f * (a1.x + a2.x), sa.y + 0.5f * (a1.y + a2.y));
    const float2 tb = make_float2(sb.x + 0.5f * (b1.x + b2.x), sb.y + 0.5f * (b1.y + b2.y));
    d[v] = make_float2(tv.x + 0.5f * (ta.x + tb.x), tv.y + 0.5f * (ta.y + tb.y));
}

// ... and with the two-hop table of the pair (KernelDev::nbr2, filled by the streaming build of single-frame engines) the launch is a
// table read and one level of gathers: same operations, same order, same bits
__global__ void __launch_bounds__(kBlock) k_blur2x2t(KernelDev kd, const float *__restrict__ src, float *__restrict__ dst, int pair, int npairs, int F,
                                                     XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int v = fb.bx * (int)blockDim.x + threadIdx.x;
    if (v >= kd.V[f]) return;
    const float2 *o = reinterpret_cast<const float2 *>(src + (size_t)f * kd.vstride + kd.vbase);   // o[-1] = absent
    float2 *d = reinterpret_cast<float2 *>(dst + (size_t)f * kd.vstride + kd.vbase);
    const int4 *tb = reinterpret_cast<const int4 *>(kd.nbr2) + (((size_t)f * npairs + pair) * kd.Epad + v) * 2;
    const int4 h0 = tb[0], h1 = tb[1];                   // {v1, v2, a, b}, {a1, a2, b1, b2}
    const float2 sv = o[v];
    const float2 v1 = o[h0.x], v2 = o[h0.y], sa = o[h0.z], sb = o[h0.w];
    const float2 a1 = o[h1.x], a2 = o[h1.y], b1 = o[h1.z], b2 = o[h1.w];
    const float2 tv = make_float2(sv.x + 0.5f * (v1.x + v2.x), sv.y + 0.5f * (v1.y + v2.y));
    const float2 ta = make_float2(sa.x + 0.5f * (a1.x + a2.x), sa.y + 0.5f * (a1.y + a2.y));
    const float2 tbv = make_float2(sb.x + 0.5f * (b1.x + b2.x), sb.y + 0.5f * (b1.y + b2.y));
    d[v] = make_float2(tv.x + 0.5f * (ta.x + tbv.x), tv.y + 0.5f * (ta.y + tbv.y));
}

// a blur pass with a launch of its own, off the compact table or the 32-bit one (engine.h: blur_alone_compact, blur_alone_nontemporal)
inline void launch_blur2(const KernelDev &kd, const float *src, float *dst, int j, int F, int maxV, bool compact, bool nt, hipStream_t s)
{
    XcdMap nb;
    const int blk = iter_block(F);
    const dim3 g = grid_xcd((maxV + 1) / 2, F, &nb, blk);
    if (compact) k_blur2c<<<g, blk, 0, s>>>(kd, src, dst, j, F, nb);
    else if (nt) k_blur2<true><<<g, blk, 0, s>>>(kd, src, dst, j, F, nb);
    else k_blur2<false><<<g, blk, 0, s>>>(kd, src, dst, j, F, nb);
}

// slice + apply for L = 2; the LAST kernel of the step also does the softmax (saves a pass over next).
// BLUR (one frame in flight, odd d + 1: the pass that is left over when passes go two per launch): `val` holds the values BEFORE
// the last blur pass and every point blurs its own d + 1 vertices on the way -- t = s[o] + 0.5 (s[n1(o)] + s[n2(o)]) along the last
// axis, the operations of k_blur2 in the same order, so the same bits -- instead of a launch of its own for that pass (a vertex
// shared by several points is blurred once per point: 1.2 x the work at C5, one launch and one chain of latencies less).
template <int D1, bool BLUR = false>
__global__ void __launch_bounds__(kBlock) k_slice2(KernelDev kd, CrfDev c, const float *__restrict__ val,
                                                   int first, int last, float relax, XcdMap nb)
{
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= c.F) return;
    const int i = fb.bx * (int)blockDim.x + threadIdx.x;
    if (i >= c.n_points[f]) return;
    const size_t fe = (size_t)f * kd.Epad;
    const float2 *vf = reinterpret_cast<const float2 *>(val + (size_t)f * kd.vstride + kd.vbase);
    float t0 = 0.0f, t1 = 0.0f;
    if (BLUR) {
        const int2 *nl = reinterpret_cast<const int2 *>(kd.nbr) + ((size_t)f * D1 + (D1 - 1)) * kd.Epad;
        int o[D1];
        int2 n[D1];
        float2 x[D1], a[D1], b[D1];
#pragma unroll
        for (int j = 0; j < D1; ++j) o[j] = kd.offset[fe + (size_t)i * D1 + j];
#pragma unroll
        for (int j = 0; j < D1; ++j) { n[j] = nl[o[j]]; x[j] = vf[o[j]]; }
#pragma unroll
        for (int j = 0; j < D1; ++j) { a[j] = vf[n[j].x]; b[j] = vf[n[j].y]; }
#pragma unroll
        for (int j = 0; j < D1; ++j) {
            const float wgt = kd.bary[fe + (size_t)i * D1 + j] * kd.alpha;
            const float bx = x[j].x + 0.5f * (a[j].x + b[j].x), by = x[j].y + 0.5f * (a[j].y + b[j].y);
            t0 += wgt * bx;
            t1 += wgt * by;
        }
    } else {
#pragma unroll
        for (int j = 0; j < D1; ++j) {
            const float wgt = kd.bary[fe + (size_t)i * D1 + j] * kd.alpha;
            const float2 x = vf[kd.offset[fe + (size_t)i * D1 + j]];
            t0 += wgt * x.x;
            t1 += wgt * x.y;
        }
    }
    const size_t q = (size_t)f * c.maxN + i;
    float2 base;
    if (first) {
        const float2 u = reinterpret_cast<const float2 *>(c.unary)[q];
        base = make_float2(-u.x, -u.y);
    } else {
        base = reinterpret_cast<const float2 *>(c.next)[q];
    }
    const float wn = kd.w * kd.norm[q];
    const float2 nx = make_float2(base.x + wn * t0, base.y + wn * t1);
    if (last) {
        float2 *Q = reinterpret_cast<float2 *>(c.Q);
        Q[q] = softmax2(1.0f * nx.x, 1.0f * nx.y, Q[q], relax);
    } else {
        reinterpret_cast<float2 *>(c.next)[q] = nx;
    }
}

// the ping-pong of the blur passes: what a pass wrote is what the next one reads
inline void swap_values(const float *&src, float *&dst) { const float *t = src; src = dst; dst = const_cast<float *>(t); }

// the d + 1 blur passes of the generic filter; returns the buffer that holds the result
const float *filter_passes(const KernelDev &kd, int F, int maxV, int L, hipStream_t s, int reverse = 0)
{
    const float *src = kd.val0;
    float *dst = kd.val1;
    for (int jj = 0; jj < kd.D1; ++jj) {
        const int j = reverse ? kd.D1 - 1 - jj : jj;     // (reverse: the transposed filter, launch_filter)
        if (L >= 4) k_blur4<<<grid_for((long)maxV * ((L + 3) / 4), F), kBlock, 0, s>>>(kd, src, dst, j, L, (L + 3) / 4);
        else if (L == 1) k_blur1x4<<<grid_for(((long)maxV + 3) / 4, F), kBlock, 0, s>>>(kd, src, dst, j);
        else k_blur<<<grid_for((long)maxV * L, F), kBlock, 0, s>>>(kd, src, dst, j, L);
        swap_values(src, dst);
    }
    return src;
}

// A two-label term of the mean-field step (launch_step_stream) in three steps.  Step 1, the splat of Q into kd.val0: returns j0, the
// number of blur passes it took along.
int splat2_term(const CrfDev &c, const KernelDev &kd, int maxV, hipStream_t s)
{
    XcdMap nb;
    const int blk = iter_block(c.F);
    // sorted build, one pass per launch: the first pass (axis 0 = the code's fastest coordinate) rides in the splat
    const int j0 = splat_passes_taken(kd);
    if (j0 >= 2) {
        const int B = kd.splat_block, core = B - 2 * kd.splat_halo;
        const float2 *q2 = reinterpret_cast<const float2 *>(c.Q);
        const SplatShape sh = splat_window_shape(B, c.F);                             // (engine.h: which instantiation and why)
        const dim3 g = grid_xcd(((long)maxV + core - 1) / core * sh.lanes, c.F, &nb, sh.lanes);
        // (one 16-byte record per vertex in place of seven loads, and 512 lanes x 2 vertices with many frames in flight: both
        // +-noise, notes/r5_experiments.md section 3)
        const int halo = kd.splat_halo;
        if (sh.lanes == 256 && sh.per_lane == 1) k_splat2w<256, 1><<<g, 256, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
        else if (sh.lanes == 512 && sh.per_lane == 1) k_splat2w<512, 1><<<g, 512, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
        else if (sh.lanes == 256 && sh.per_lane == 2) k_splat2w<256, 2><<<g, 256, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
        else if (sh.lanes == 512 && sh.per_lane == 2) k_splat2w<512, 2><<<g, 512, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
        else if (sh.lanes == 1024 && sh.per_lane == 1) k_splat2w<1024, 1><<<g, 1024, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
        else k_splat2w<256, 4><<<g, 256, 0, s>>>(kd, q2, c.maxN, c.F, nb, j0, halo);
    } else if (j0 == 1) {
        const dim3 g = grid_xcd(((long)maxV + blk - 3) / (blk - 2) * blk, c.F, &nb, blk);
        k_splat2<true><<<g, blk, 0, s>>>(kd, reinterpret_cast<const float2 *>(c.Q), c.maxN, c.F, nb);
    } else if (kd.long_mode) {                    // a coarse kernel: long rows
        if (kd.long_mode == 2) {                  // (a wavefront per vertex: grid_xcd counts workgroups of kBlock / 64 vertices)
            const dim3 g = grid_xcd((long)maxV * 64, c.F, &nb, kBlock);
            k_splat2v<<<g, kBlock, 0, s>>>(kd, reinterpret_cast<const float2 *>(c.Q), c.maxN, c.F, nb);
        } else {
            const dim3 g = grid_xcd(maxV, c.F, &nb, kBlock);
            k_splat2l<<<g, kBlock, 0, s>>>(kd, reinterpret_cast<const float2 *>(c.Q), c.maxN, c.F, nb);
        }
        if (kd.longrow_ok) k_splat_long<false><<<dim3((unsigned)std::max(256 / std::max(c.F, 1), 8), (unsigned)c.F), kBlock, 0, s>>>(kd, c.Q, c.maxN * 2, 2, nullptr);
    } else {
        const dim3 g = grid_xcd(maxV, c.F, &nb, blk);
        k_splat2<false><<<g, blk, 0, s>>>(kd, reinterpret_cast<const float2 *>(c.Q), c.maxN, c.F, nb);
    }
    return j0;
}

// Step 2, the blur passes with a launch of their own, each on the route the plan gives it (engine.h: blur_plan; the passes in the
// splat and the one in the slice have none): returns the buffer holding the result
const float *blur2_passes(const CrfDev &c, const KernelDev &kd, int maxV, const BlurPlan &plan, hipStream_t s)
{
    XcdMap nb;
    const int blk = iter_block(c.F);
    const float *src = kd.val0;
    float *dst = kd.val1;
    for (int j = 0; j < kd.D1;) {
        const int route = plan.route[j];
        if (route == kBlurInSplat || route == kBlurInSlice) {
            j += 1;
            continue;
        }
        if (route == kBlurPairTable || route == kBlurPairPlain) {                  // two passes per launch
            const dim3 gp = grid_xcd(maxV, c.F, &nb, blk);
            if (route == kBlurPairTable) k_blur2x2t<<<gp, blk, 0, s>>>(kd, src, dst, plan.table_pair[j], plan.table_pairs, c.F, nb);
            else k_blur2x2<<<gp, blk, 0, s>>>(kd, src, dst, j, c.F, nb);
            j += 2;
        } else {
            launch_blur2(kd, src, dst, j, c.F, maxV, route == kBlurAloneCompact, plan.nontemporal, s);
            j += 1;
        }
        swap_values(src, dst);
    }
    return src;
}

// Step 3, the slice of `val` into next (first: from -unary) or, for the step's last term, through the softmax into Q
void slice2_term(const CrfDev &c, const KernelDev &kd, const float *val, bool blur_in_slice, int first, int last, float relax, hipStream_t s)
{
    XcdMap nb;
    const int blk = iter_block(c.F);
    const dim3 g = grid_xcd(c.maxN, c.F, &nb, blk);
    with_dims<2, 9>(kd.D1, [&](auto d1) {
        if (blur_in_slice) k_slice2<decltype(d1)::value, true><<<g, blk, 0, s>>>(kd, c, val, first, last, relax, nb);
        else k_slice2<decltype(d1)::value><<<g, blk, 0, s>>>(kd, c, val, first, last, relax, nb);
    });
}

}  // namespace

// norm = 1 / (compute(ones) + 1e-20), value width 1.  pairwise3d.h:22-27.
void launch_norm(const KernelDev &kd, const CrfDev &c, int maxV, hipStream_t s)
{
    launch_splat(kd, nullptr, 0, 1, c.F, maxV, s);
    const float *res = filter_passes(kd, c.F, maxV, 1, s);
    const dim3 g = grid_for(c.maxN, c.F);
    if (!with_dims<2, 9>(kd.D1, [&](auto d1) { k_slice_norm<decltype(d1)::value><<<g, kBlock, 0, s>>>(kd, c, res); }))
        k_slice<<<g, kBlock, 0, s>>>(kd, c, res, 1, SLICE_NORM);
}

void launch_step_stream(const CrfDev &c, const KernelDev *kds, const int *maxV, float relax, hipStream_t s, const float *const *compat,
                        const float *const *pre)
{                                                    // densecrf_base.h:82-91
    const int L = c.L;
    // the two-label kernels hard-wire Potts terms normalised AFTER the filter: a CRF with a matrix (section 1e) or with a term in
    // another normalisation mode (section 1g: `pre` is not null) takes the general branch at L = 2 as well
    bool general = pre != nullptr;
    for (int k = 0; k < c.K && compat; ++k) general |= compat[k] != nullptr;
    if (c.K == 0) {
        // stepInit only: next = -unary, then softmax.  Done by the softmax with scale -1.
        launch_exp_and_normalize(c, c.unary, c.Q, -1.0f, relax, s);
        return;
    }
    if (L == 2 && !general) {
        for (int k = 0; k < c.K; ++k) {
            const KernelDev &kd = kds[k];
            const BlurPlan plan = blur_plan(kd, c.F, maxV[k]);                    // (engine.h: the one rule, also what the getters report)
            (void)splat2_term(c, kd, maxV[k], s);                                  // (takes plan.counts.in_splat passes along: splat_passes_taken)
            const float *res = blur2_passes(c, kd, maxV[k], plan, s);
            slice2_term(c, kd, res, plan.counts.in_slice != 0, k == 0, k == c.K - 1, relax, s);
        }
        return;
    }
    for (int k = 0; k < c.K; ++k) {
        const KernelDev &kd = kds[k];
        launch_splat(kd, c.Q, c.maxN * L, L, c.F, maxV[k], s, pre ? pre[k] : nullptr);
        launch_slice_apply(kd, c, filter_passes(kd, c.F, maxV[k], L, s), L, k == 0 ? SLICE_APPLY_FIRST : SLICE_APPLY, compat ? compat[k] : nullptr, s);
    }
    launch_exp_and_normalize(c, c.next, c.Q, 1.0f, relax, s);
}

// Measurement support (bench.py's roofline object): `reps` launches of the streaming engine's dominant kernel --
// one blur pass of kernel kd over all F frames -- bracketed by HIP events on stream s.  The lattice values it
// scribbles over are recomputed from Q by every mean-field step.
hipError_t time_blur_pass(const KernelDev &kd, int F, int maxV, int L, int reps, hipStream_t s, float *ms_per_launch)
{
    hipEvent_t e0, e1;
    hipError_t rc = hipEventCreate(&e0);
    if (rc != hipSuccess) return rc;
    if ((rc = hipEventCreate(&e1)) != hipSuccess) { (void)hipEventDestroy(e0); return rc; }
    auto pass = [&](int i) {
        const float *src = (i & 1) ? kd.val1 : kd.val0;
        float *dst = (i & 1) ? kd.val0 : kd.val1;
        if (L == 2) launch_blur2(kd, src, dst, i % kd.D1, F, maxV, blur_alone_compact(kd), blur_alone_nontemporal(F), s);
        else k_blur<<<grid_for((long)maxV * L, F), kBlock, 0, s>>>(kd, src, dst, i % kd.D1, L);
    };
    for (int i = 0; i < 3; ++i) pass(i);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < reps; ++i) pass(i);
    (void)hipEventRecord(e1, s);
    rc = hipEventSynchronize(e1);
    if (rc == hipSuccess) rc = hipEventElapsedTime(ms_per_launch, e0, e1);
    *ms_per_launch /= (float)reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

// out (+)= [w * norm *] compute(in) with value width c.L: PairwisePotential::apply (accumulate = 1, pairwise3d.h:73-78)
// or the bare PermutohedralLatticeCPU::compute (accumulate = 0, permutohedral_cpu.h:634-699); reverse = 1: its transpose (engine.h)
void launch_filter(const KernelDev &kd, const CrfDev &c, int maxV, const float *in, float *out, int accumulate, hipStream_t s,
                   int reverse, const float **blurred, const float *compat, const float *pre)
{
    const int L = c.L;
    launch_splat(kd, in, c.maxN * L, L, c.F, maxV, s, pre);
    const float *res = filter_passes(kd, c.F, maxV, L, s, reverse);
    CrfDev c2 = c;
    c2.next = out;
    launch_slice_apply(kd, c2, res, L, accumulate ? SLICE_APPLY : SLICE_PLAIN, accumulate ? compat : nullptr, s);
    if (blurred) *blurred = res;
}

// the splat and the blur passes of a width-1 filter without the slice (engine.h)
const float *launch_filter_values1(const KernelDev &kd, const CrfDev &c, int maxV, const float *in, int in_stride, hipStream_t s,
                                   int reverse)
{
    launch_splat(kd, in, in_stride, 1, c.F, maxV, s);
    return filter_passes(kd, c.F, maxV, 1, s, reverse);
}

}  // namespace lccrf

// meanfield_backward.hip -- reverse-mode gradients of DenseCRF::inference (densecrf_base.h:65-91): include/lccrf.h section 1c.
//
// The C-ABI layer (api_backward.hip: backward_call, behind every lccrf_*inference_backward* entry point) replays the forward on the step
// path, keeping Q_0 .. Q_{T-1}, and then runs the sweep below on the call's stream, for every frame at once (the frame is
// blockIdx.y; a handle is a batch of one).  What a call asks for is a BackwardRequest (engine.h); backward_layout() below lays its
// area out, for the sizing and for the run alike.  Per iteration t = T .. 1:
//   Phi_k(Q_{t-1})                          launch_filter, forward blur order (the streaming engine's splat / blur / slice)
//   x_t, P_t, gamma_t, dL/dU, n_k gamma_t   k_softmax_bwd (+ the per-workgroup partials of the K weight-gradient dot products)
//   Phi_k^T(n_k gamma_t)                    launch_filter, blur passes in REVERSE axis order (each pass is symmetric, their product
//                                           is not: the transpose of B_d .. B_0 is B_0 .. B_d)
//   G_{t-1} = (1 - r) G_t + sum_k w_k .     k_bwd_combine
// then the softmax backward of Q_0 = softmax(-U) and the fixed-order reduction of the partials (k_bwd_reduce).  No float atomics:
// every sum is formed in an order fixed by N and L alone, so the results are the same bits from run to run -- and a frame of a
// batch gets the bits a handle of its n_points[f] points gets (the weight gradient's partials included: backward_blocks(n_points[f])
// of them per iteration, reduced in the handle's order).
//
// The feature part (sections 1d and 2d: dL/d features of every term asked for) rides in the same sweep.  Inside a simplex the corner
// weights b_ic are linear in the point's features, and for any product <y, Phi(x)>
//   d<y, Phi(x)> / d b_ic = alpha (<y_i, (B S x)[v_ic]> + <x_i, (B^T S y)[v_ic]>)
// -- the blurred vertex values of the forward filter dotted with the upstream row, and those of the transposed filter dotted with the
// input row.  Both are in term k's own value buffer when they are needed (launch_filter hands the buffer out), so per (t, k) the
// sweep adds two k_corner_dot launches: x = Q_{t-1}, y = w_k n_k gamma_t.  The norm n_k = 1 / (Phi_k(1) + 1e-20) depends on the
// features too: k_softmax_bwd<G, true> also accumulates g_n[k][i] = sum_t w_k <gamma_t,i, Phi_k(Q_{t-1})_i>, and after the loop one
// width-1 filter pair per term gives the corner dots of <a_k, Phi_k(1)>, a_k = -n_k^2 g_n[k].  k_corner_to_feature then maps
// dL/db to dL/df through the simplex of the point (recomputed from the features with the build's own lattice_simplex: the ranks
// of the one-workgroup build never reach HBM).  Every g_b[i][c] has one owner and one order of additions (t = T .. 1, slice side,
// splat side; the norm part last): the same bits from run to run, and for a frame of a batch those of a handle.
//
// Both parts together (section 1f): the sweep takes section 1e's form and adds section 1d's launches to it.  Per (t, k) the slice-side
// k_corner_dot runs after k_compat_bwd has turned phi_k into mu_k^T (n_k gamma_t) and before the transposed filter overwrites it; the
// splat side runs on the transposed filter's values as before, and g_n is formed from mu_k Phi_k (k_joint_softmax<G>).
//
// Feature gradients under a normalisation mode (sections 1m and 2i; only with `modes`, i.e. a term that is not AFTER and a feature array):
// the factors a_k (behind the filter: kds[k].norm) and b_k (in front of it: pre[k]) depend on the features through the norm.  The splat
// side's row becomes b_k . Q_{t-1}; ar.gn[k] takes dL/da_k from the softmax kernel (terms with a post factor) and dL/db_k =
// w_k <Q_{t-1}, Phi_k^T(y)> from k_bwd_combine_adjoint, which runs in k_bwd_combine<true>'s place (terms with a pre factor), in that
// order; k_norm_adjoint turns the sum into dL/dn by the term's mode, with the TRUE norm.  Every other request launches what it launched.
//
// A batch's learnt model (section 2h): the compatibility part is per frame too -- k_compat_bwd cuts a frame's rows into the chunk count
// of a handle of n_points[f] points, k_compat_reduce sums that frame's chunks in order into d_grad_compat[f] -- and k_sum_frames adds
// dL/dw and dL/dmu over the frames in ascending order for the (global) model's gradient.
//
// Rows at or beyond n_points[f] (the phantom points of quirk Q1 among them) are never read: every lattice build lists real points
// only in its splat rows (k_csr_count / k_eoffsets in stream_build.hip, E = N (d+1) in build_small.hip), the slice writes rows
// i < n_points[f] only, and the kernels below stop at n_points[f].  A batch rebound with fewer points than an earlier call leaves
// stale rows in its area; nothing reads them.
#include <algorithm>
#include <type_traits>

#include "engine.h"
#include "device_math.h"
#include "stream_common.h"   // with_dims

namespace lccrf {
namespace {

constexpr int kBwdBlock = 256;
constexpr int kBwdMaxK = LCCRF_MAX_KERNELS;

struct BwdWeights { float w[kBwdMaxK]; };
struct BwdArgs {
    const int *n_points;         // [F]
    int L, K, first;             // first: the sweep's first iteration writes dL/dU, the others accumulate into it
    int rows;                    // rows per frame of gU: the first iteration writes rows [n_points[f], rows) as 0
    int nstride;                 // points between frames of norm (c.maxN)
    float relax;
    size_t fs;                   // floats between frames of unary, phi, G and gU (c.maxN * L)
    size_t slice;                // floats between the terms of phi (BackwardArea::slice)
    const float *unary;          // [F][maxN][L]
    float *phi;                  // [K][slice]: Phi_k(Q_{t-1}) in, n_k * gamma_t out
    const float *G;              // [F][maxN][L] dL/dQ_t
    float *gU;                   // [F][maxN][L] dL/dU
    float *partial;              // [K][F][gridDim.x] or null
    const float *norm[kBwdMaxK];
    float w[kBwdMaxK];
    float *gn[kBwdMaxK];         // k_softmax_bwd<G, true>: [F][gnstride] per term, or null (BackwardArea::gn)
    int gnstride;
    const float *compat[kBwdMaxK];   // k_compat_softmax<G>: the term's [L][L] matrix mu_k, or null (Potts)
    float *gam;                  // ... and [F][maxN][L]: receives gamma_t (phi is left as it came: k_compat_bwd turns it over)
    const int *counts;           // [F] or null (section 2j): the frame's own iteration count, clamped to [0, cap] by frame_count
    int t, cap;                  // ... the sweep's iteration of this launch (0: the softmax backward of Q_0) and the counts' cap
};

// section 2j: the iterations frame f is differentiated at -- the caller's count clamped to [0, cap]
__device__ __forceinline__ int frame_count(const int *__restrict__ counts, int f, int cap) { return min(max(counts[f], 0), cap); }

enum { kBwdPlain = 0, kBwdFeat = 1, kBwdCompat = 2, kBwdCompatFeat = 3 };   // what k_softmax_bwd does besides section 1c's work (bits: feature, compat)

// lanes per row: one row per lane up to 4 labels, then four labels per lane over a power-of-two group of lanes
inline int bwd_lanes(int L) { return L <= 4 ? 1 : L <= 8 ? 2 : L <= 16 ? 4 : L <= 32 ? 8 : 16; }

// ... and the one dispatch on them: fn(std::integral_constant<int, G>) with G = bwd_lanes(L) as a compile-time constant
template <typename Fn>
void with_bwd_lanes(int L, Fn fn)
{
    switch (bwd_lanes(L)) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 8: fn(std::integral_constant<int, 8>{}); break;
    default: fn(std::integral_constant<int, 16>{}); break;
    }
}

// the label-ordered sum of one value per label over the row's lanes (lane first + c holds labels 4c .. 4c+3): every lane of the row
// ends with the same sum, added one label at a time in label order 0 .. L-1, as densecrf3d.h:80-84 adds the row sum
template <int G>
__device__ __forceinline__ float row_sum_ordered(const float (&v)[4], int L, int first)
{
    float s = 0.0f;
    for (int t = 0; t < L; ++t) {
        const int u = t & 3;
        const float src = u == 0 ? v[0] : u == 1 ? v[1] : u == 2 ? v[2] : v[3];
        s += G == 1 ? src : __shfl(src, first + (t >> 2), 64);
    }
    return s;
}

// One iteration's softmax backward.  A row (point) is G lanes; lane c of the row holds labels 4c .. 4c+3.
//   x   = -U + sum_k (w_k * n_k) * Phi_k          the forward's own expression (k_slice / k_slice2: base + w * norm * t)
//   P   = softmax(x)                              fast_exp as expAndNormalize (densecrf3d.h:70-98) forms it
//   gam = r * P * (G - <G, P>)                    (in a form that keeps the bits of saturated rows, below)
//   gU  = -gam (first) or gU - gam
//   phi_k <- n_k * gam (in place: the transposed filter's input), partial[k][f][block] = sum over the block of n_k * gam * Phi_k
// K = 0: x = -U (the start, densecrf_base.h:78-80, or a CRF without terms).
// k_softmax_bwd<G, true> (kBwdFeat): also gn[k][i] += w_k * <gam_i, Phi_k,i> (labels in order) for every term with a gn -- nothing else changes.
// k_compat_softmax<G> (kBwdCompat, section 1e): a term with a matrix enters x and the weight dot as mu_k Phi_k -- per label l the forward's own sum
// s = 0; s = s + mu[l][l'] * Phi[l'], l' = 0 .. L-1 (k_slice_compat) -- gamma_t goes to a.gam and phi stays Phi_k(Q_{t-1}):
// k_compat_bwd needs both for dL/dmu and writes the transposed filter's input itself.
// k_joint_softmax<G> (kBwdCompatFeat, section 1f: k_compat_softmax<G> with the feature part, under a name of its own) does both -- gn[k][i] += w_k * <gam_i, (mu_k Phi_k)_i>, the dot formed from the row sums
// mu_k Phi_k this kernel has anyway (Phi_k itself for a Potts term), accumulated as k_softmax_bwd<G, true> does; nothing else changes.
// mu is read from global memory here, L x 4 loads per lane and term, all lanes of a wavefront within a few rows of one matrix of
// at most 16 KB (cache hits after the first touch): up to eight matrices do not fit this kernel's LDS next to each other, and
// staging them one by one would put 2 K barriers into a kernel whose rows are otherwise independent.
template <int G, int MODE>
__device__ __forceinline__ void softmax_bwd(const BwdArgs &a)
{
    constexpr bool FEAT = (MODE & kBwdFeat) != 0, COMPAT = (MODE & kBwdCompat) != 0;
    const int f = blockIdx.y;
    const int N = a.n_points[f], L = a.L, K = a.K;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, first = lane - sub;
    const int i = blockIdx.x * (kBwdBlock / G) + (int)threadIdx.x / G;
    const bool live = i < N;
    const int l0 = sub * 4;
    int begins = a.first;                                 // this launch is the frame's first step: dL/dU is written, not added to
    if (a.counts) {                                       // (section 2j; uniform over the workgroup: blockIdx.y alone decides)
        const int tf = frame_count(a.counts, f, a.cap);
        if (a.t > tf) return;                             // an idle frame: nothing written, before any barrier
        begins = a.t == tf;
    }
    if (begins && !live && i < a.rows) {                  // rows beyond the frame's points: dL/dU = 0
        const size_t z = f * a.fs + (size_t)i * L + l0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (l0 + u < L) a.gU[z + u] = 0.0f;
    }
    bool has[4];
    float x[4], g[4];
    const size_t q = f * a.fs + (size_t)(live ? i : 0) * L + l0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        has[u] = live && l0 + u < L;
        x[u] = has[u] ? -a.unary[q + u] : 0.0f;
        g[u] = has[u] ? a.G[q + u] : 0.0f;
    }
    float ph[kBwdMaxK][4];
    float nk[kBwdMaxK];
#pragma unroll
    for (int k = 0; k < kBwdMaxK; ++k) {
        nk[k] = 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) ph[k][u] = 0.0f;
        if (k < K) {
            nk[k] = live ? a.norm[k][(size_t)f * a.nstride + i] : 0.0f;
            const float wn = a.w[k] * nk[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) ph[k][u] = has[u] ? a.phi[k * a.slice + q + u] : 0.0f;
            if (COMPAT && a.compat[k]) {                    // (uniform: the shuffles see every lane of the row)
                const float *mu = a.compat[k];
                float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int t = 0; t < L; ++t) {
                    const int v = t & 3;
                    const float src = v == 0 ? ph[k][0] : v == 1 ? ph[k][1] : v == 2 ? ph[k][2] : ph[k][3];
                    const float pt = G == 1 ? src : __shfl(src, first + (t >> 2), 64);
#pragma unroll
                    for (int u = 0; u < 4; ++u) m[u] = m[u] + mu[min(l0 + u, L - 1) * L + t] * pt;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) ph[k][u] = has[u] ? m[u] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = x[u] + wn * ph[k][u];
        }
    }
    // row maximum (order-free), exponentials, the row sum in label order
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (has[u] && mx < x[u]) mx = x[u];
#pragma unroll
    for (int m = 1; m < G; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = has[u] ? fast_exp_nonpos(x[u] - mx) : 0.0f;
    const float tt = row_sum_ordered<G>(e, L, first);
    // G_l - <G, P> is formed as (G_l - G_a) - sum_m P_m (G_m - G_a), a = the row's first largest label (sum_m P_m = 1): a saturated
    // row (P_a = 1 - 1e-8) keeps its gradient's few significant bits, which G_l - <G, P> would cancel in fp32
    float ga = 0.0f;
    bool found = false;
    for (int t = 0; t < L; ++t) {
        const int u = t & 3;
        const float xs = u == 0 ? x[0] : u == 1 ? x[1] : u == 2 ? x[2] : x[3];
        const float gs = u == 0 ? g[0] : u == 1 ? g[1] : u == 2 ? g[2] : g[3];
        const float xv = G == 1 ? xs : __shfl(xs, first + (t >> 2), 64);
        const float gv = G == 1 ? gs : __shfl(gs, first + (t >> 2), 64);
        if (!found && xv == mx) { ga = gv; found = true; }
    }
    float p[4], gp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        p[u] = has[u] ? e[u] / tt : 0.0f;
        gp[u] = p[u] * (g[u] - ga);
    }
    const float dev = row_sum_ordered<G>(gp, L, first);
    float wsum[kBwdMaxK];
    float gamv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kBwdMaxK; ++k) wsum[k] = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (!has[u]) continue;
        const float gam = a.relax * (p[u] * ((g[u] - ga) - dev));
        if (FEAT) gamv[u] = gam;
        a.gU[q + u] = begins ? -gam : a.gU[q + u] - gam;
        if (COMPAT) a.gam[q + u] = gam;
#pragma unroll
        for (int k = 0; k < kBwdMaxK; ++k)
            if (k < K) {
                const float gn = nk[k] * gam;
                wsum[k] += gn * ph[k][u];
                if (!COMPAT) a.phi[k * a.slice + q + u] = gn;
            }
    }
    if (FEAT) {
#pragma unroll
        for (int k = 0; k < kBwdMaxK; ++k) {
            if (k >= K || !a.gn[k]) continue;             // (uniform)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = gamv[u] * ph[k][u];
            const float sk = row_sum_ordered<G>(v, L, first);
            if (live && sub == 0) {
                float *gp = a.gn[k] + (size_t)f * a.gnstride + i;
                *gp = *gp + a.w[k] * sk;
            }
        }
    }
    if (!a.partial) return;
    // per-workgroup partials: a fixed butterfly over the wavefront, then the four wavefronts in order
    __shared__ float red[kBwdMaxK][kBwdBlock / 64];
#pragma unroll
    for (int k = 0; k < kBwdMaxK; ++k) {
        if (k >= K) break;
        float s = wsum[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (lane == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        float s = 0.0f;
        for (int w = 0; w < kBwdBlock / 64; ++w) s += red[threadIdx.x][w];
        a.partial[((size_t)threadIdx.x * gridDim.y + f) * gridDim.x + blockIdx.x] = s;
    }
}

template <int G, bool FEAT>
__global__ void __launch_bounds__(kBwdBlock) k_softmax_bwd(BwdArgs a)
{
    softmax_bwd<G, FEAT ? kBwdFeat : kBwdPlain>(a);
}

template <int G>
__global__ void __launch_bounds__(kBwdBlock) k_compat_softmax(BwdArgs a)
{
    softmax_bwd<G, kBwdCompat>(a);
}

template <int G>
__global__ void __launch_bounds__(kBwdBlock) k_joint_softmax(BwdArgs a)
{
    softmax_bwd<G, kBwdCompatFeat>(a);
}

// G = keep * G + sum_k w_k * buf_k, element by element (keep = 1 - relax); frame blockIdx.y
// PRE (section 1g): a term whose filter input is scaled by b_k (pre.p[k], [F][nstride]; null: 1) adds w_k * (b_k[i] * buf_k) -- the
// transposed filter's result goes back through the input's factor.  PRE = false is the code it was.
struct BwdPre { const float *p[kBwdMaxK]; int nstride; };
// cn (section 2j; counts null: every frame takes the step): a frame whose count is below this launch's iteration is idle -- its G
// stays the caller's dL/dQ.
struct BwdCounts { const int *counts; int t, cap; };
template <bool PRE>
__global__ void __launch_bounds__(kBwdBlock) k_bwd_combine(const int *__restrict__ n_points, int L, int K, const float *__restrict__ buf,
                                                         size_t slice, size_t fs, BwdWeights wk, float keep, float *__restrict__ G,
                                                         BwdPre pre, BwdCounts cn)
{
    const int f = blockIdx.y;
    const long idx = (long)blockIdx.x * kBwdBlock + threadIdx.x;
    if (idx >= (long)n_points[f] * L) return;
    if (cn.counts && cn.t > frame_count(cn.counts, f, cn.cap)) return;
    const size_t o = f * fs + idx;
    float acc = keep * G[o];
    if constexpr (PRE) {
        const size_t i = (size_t)f * pre.nstride + idx / L;
#pragma unroll
        for (int k = 0; k < kBwdMaxK; ++k) {
            if (k >= K) break;
            float v = buf[k * slice + o];
            if (pre.p[k]) v = pre.p[k][i] * v;
            acc = acc + wk.w[k] * v;
        }
    } else {
        for (int k = 0; k < K; ++k) acc = acc + wk.w[k] * buf[k * slice + o];
    }
    G[o] = acc;
}

// k_bwd_combine<true> by rows, with the pre adjoint of section 1m: a row (point) is G lanes as in k_softmax_bwd, lane c of the row holds
// labels 4c .. 4c+3.  Per element the arithmetic of k_bwd_combine<true>, in its order (the same bits in G); and before buf_k = z_k is
// scaled by b_k, for every term with an accumulator (adj.gn[k]: a BEFORE or SYMMETRIC term whose feature gradient is asked for)
//   gn[k][i] += w_k * <Q_{t-1},i, z_k,i>        labels in order 0 .. L-1, one owner per point (the row's first lane)
// -- dL/d b_k[i] of x = b_k . Q_{t-1}.  It runs behind this iteration's k_softmax_bwd, so the post part is added before the pre part.
// cn (section 2l) as k_bwd_combine takes it: an idle frame's workgroups leave before the row sums' shuffles, on blockIdx.y alone -- nothing
// is added to its gn (buf is scratch for it: no softmax kernel wrote this iteration's filter input) and its G stays the caller's dL/dQ.
struct BwdPreAdjoint { float *gn[kBwdMaxK]; int gnstride; const float *q; };   // q: Q_{t-1}, [F][.][L] strided as G
template <int G>
__global__ void __launch_bounds__(kBwdBlock) k_bwd_combine_adjoint(const int *__restrict__ n_points, int L, int K, const float *__restrict__ buf,
                                                                 size_t slice, size_t fs, BwdWeights wk, float keep, float *__restrict__ Gd,
                                                                 BwdPre pre, BwdPreAdjoint adj, BwdCounts cn)
{
    const int f = blockIdx.y;
    if (cn.counts && cn.t > frame_count(cn.counts, f, cn.cap)) return;   // (uniform over the workgroup)
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, first = lane - sub;
    const int i = blockIdx.x * (kBwdBlock / G) + (int)threadIdx.x / G;
    const bool live = i < n_points[f];
    const int l0 = sub * 4;
    const size_t o = f * fs + (size_t)(live ? i : 0) * L + l0;
    bool has[4];
    float acc[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        has[u] = live && l0 + u < L;
        acc[u] = has[u] ? keep * Gd[o + u] : 0.0f;
        q[u] = has[u] ? adj.q[o + u] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kBwdMaxK; ++k) {
        if (k >= K) break;
        float z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) z[u] = has[u] ? buf[k * slice + o + u] : 0.0f;
        if (adj.gn[k]) {                                    // (uniform: the shuffles of the row sum see every lane)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = q[u] * z[u];
            const float sk = row_sum_ordered<G>(v, L, first);
            if (live && sub == 0) {
                float *gp = adj.gn[k] + (size_t)f * adj.gnstride + i;
                *gp = *gp + wk.w[k] * sk;
            }
        }
        const float b = pre.p[k] && live ? pre.p[k][(size_t)f * pre.nstride + i] : 1.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float v = pre.p[k] ? b * z[u] : z[u];
            acc[u] = acc[u] + wk.w[k] * v;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (has[u]) Gd[o + u] = acc[u];
}

// out[f][k] = sum over the iterations and the frame's workgroups of partial[t][k][f][b]: one workgroup per (term, frame), a strided
// walk over the T x backward_blocks(n_points[f]) partials of the frame in a fixed order and a fixed tree in LDS (store and sum: no
// atomics, the same bits every run, and those of a handle of n_points[f] points).  bstride: the partials' row (the sweep's grid).
// counts != null (section 2j): the frame's own t_f in T's place -- the walk and the tree of a handle at t_f.
__global__ void __launch_bounds__(kBwdBlock) k_bwd_reduce(const float *__restrict__ partial, const int *__restrict__ n_points, int K,
                                                        int T, int rows_per_block, int bstride, float *__restrict__ out,
                                                        const int *__restrict__ counts)
{
    __shared__ float s[kBwdBlock];
    const int k = blockIdx.x, f = blockIdx.y, F = gridDim.y;
    const int nblk = max((n_points[f] + rows_per_block - 1) / rows_per_block, 1);
    const long n = (long)(counts ? frame_count(counts, f, T) : T) * nblk;
    float acc = 0.0f;
    for (long idx = threadIdx.x; idx < n; idx += kBwdBlock) {
        const long t = idx / nblk, b = idx - t * nblk;
        acc += partial[((t * K + k) * F + f) * bstride + b];
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int m = kBwdBlock / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)f * K + k] = s[0];
}

template <int MODE>
void launch_softmax_bwd(const BwdArgs &a, int F, hipStream_t s)
{
    const dim3 grid((unsigned)std::max(backward_blocks(a.rows, a.L), 1), (unsigned)F);
    with_bwd_lanes(a.L, [&](auto lanes) {
        constexpr int G = decltype(lanes)::value;
        if constexpr (MODE == kBwdCompatFeat) k_joint_softmax<G><<<grid, kBwdBlock, 0, s>>>(a);
        else if constexpr (MODE == kBwdCompat) k_compat_softmax<G><<<grid, kBwdBlock, 0, s>>>(a);
        else k_softmax_bwd<G, MODE == kBwdFeat><<<grid, kBwdBlock, 0, s>>>(a);
    });
}

// ---- the compatibility part (section 1e) ---------------------------------------------------------------------------------------
// One term, behind k_compat_softmax<G>: with y_i = n_k[i] gamma_t[i] and Phi = Phi_k(Q_{t-1}) (phi, as the filter left it)
//   cpart[f][b][l][l'] (+)= w_k * sum over workgroup b's rows of y_i[l] * Phi_i[l']        the partial of dL/dmu_k (cpart != null)
//   phi[i][l']           = sum_l mu[l][l'] * y_i[l]  (labels in order; y_i[l'] for a Potts term)   the transposed filter's input
// A frame's rows are cut into compat_chunks(n_points[f]) contiguous chunks, one per workgroup -- the count a handle of that many points
// launches, so that a frame of a batch (whose grid is sized for max_points) adds its partials in the handle's order; the workgroups
// beyond the frame's count leave before the first barrier and write nothing -- walked in tiles of R = 256 / L rows: lane r * L + l
// puts y and Phi of row r into LDS, lane p (and p + 256, ...) adds the tile's rows in order to its entries (l, l') of the outer
// product, kept in registers over the whole chunk, and lane r * L + l' forms row r of mu^T y.  No atomics: an entry has one owner and
// one order of additions (rows ascending; t = T .. 1 across the sweep's launches), the same bits from run to run.
// counts != null (section 2k): a frame is idle while t > t_f -- its workgroups leave before the first barrier, on blockIdx.y alone,
// with nothing written to cpart or phi -- and its first iteration, the one that writes cpart, is t == t_f.
constexpr int kCompatTileB = kBwdBlock + kBwdBlock / 2;   // R * (L | 1) <= 256 + R floats
constexpr int kCompatPairs = (LCCRF_MAX_LABELS * LCCRF_MAX_LABELS + kBwdBlock - 1) / kBwdBlock;   // entries of mu per lane
// (compat_chunks, the chunks of a frame of n points: engine.h -- the one-launch kernel of fused_backward_general.hip cuts the same)
struct CompatArgs {
    const int *n_points;
    int L, first;                // first: the sweep's first iteration writes cpart, the others add to it
    int nstride;
    size_t fs;
    const float *gam;            // [F][maxN][L]
    const float *norm;           // [F][nstride]
    float *phi;                  // [F][maxN][L]
    const float *mu;             // [L][L] or null
    float w;
    float *cpart;                // [F][gridDim.x][L * L] or null
    const int *counts;           // [F] or null (section 2k): the frame's own iteration count, clamped to [0, cap] by frame_count
    int t, cap;                  // ... the sweep's iteration of this launch and the counts' cap
};

__global__ void __launch_bounds__(kBwdBlock) k_compat_bwd(CompatArgs a)
{
    __shared__ float mu[LCCRF_MAX_LABELS * (LCCRF_MAX_LABELS + 1)];
    __shared__ float ys[kCompatTileB], ps[kCompatTileB];
    const int f = blockIdx.y, L = a.L, N = a.n_points[f];
    const int B = compat_chunks(N);                       // (a handle: gridDim.x)
    if ((int)blockIdx.x >= B) return;                     // (the whole workgroup, before any barrier)
    int begins = a.first;                                 // this launch is the frame's first step: cpart is written, not added to
    if (a.counts) {                                       // (uniform over the workgroup: blockIdx.y alone decides)
        const int tf = frame_count(a.counts, f, a.cap);
        if (a.t > tf) return;                             // an idle frame: nothing written, before any barrier
        begins = a.t == tf;
    }
    const int R = kBwdBlock / L, st = L == 1 ? 1 : (L | 1), tid = threadIdx.x;
    const int r = tid / L, l = tid - r * L;
    const int chunk = (N + B - 1) / B;
    const int i_begin = min((int)blockIdx.x * chunk, N), i_end = min(i_begin + chunk, N);
    if (a.mu)
        for (int idx = tid; idx < L * L; idx += kBwdBlock) {
            const int x = idx / L;
            mu[x * st + (idx - x * L)] = a.mu[idx];
        }
    float acc[kCompatPairs];
#pragma unroll
    for (int j = 0; j < kCompatPairs; ++j) acc[j] = 0.0f;
    for (int base = i_begin; base < i_end; base += R) {   // (uniform bounds: every lane meets every barrier)
        const int i = base + r;
        const bool live = r < R && i < i_end;
        if (r < R) {
            const size_t q = f * a.fs + (size_t)(live ? i : 0) * L + l;
            ys[r * st + l] = live ? a.norm[(size_t)f * a.nstride + i] * a.gam[q] : 0.0f;
            ps[r * st + l] = live ? a.phi[q] : 0.0f;
        }
        __syncthreads();
        if (a.cpart) {
            const int nr = min(R, i_end - base);
#pragma unroll
            for (int j = 0; j < kCompatPairs; ++j) {
                const int p = tid + j * kBwdBlock;
                if (p < L * L) {
                    const int x = p / L, y = p - x * L;
                    float s = acc[j];
                    for (int rr = 0; rr < nr; ++rr) s += ys[rr * st + x] * ps[rr * st + y];
                    acc[j] = s;
                }
            }
        }
        if (live) {
            float o = ys[r * st + l];
            if (a.mu) {
                o = 0.0f;
                for (int x = 0; x < L; ++x) o = o + mu[x * st + l] * ys[r * st + x];
            }
            a.phi[f * a.fs + (size_t)i * L + l] = o;
        }
        __syncthreads();
    }
    if (!a.cpart) return;
    float *cp = a.cpart + ((size_t)f * gridDim.x + blockIdx.x) * L * L;
#pragma unroll
    for (int j = 0; j < kCompatPairs; ++j) {
        const int p = tid + j * kBwdBlock;
        if (p < L * L) cp[p] = begins ? a.w * acc[j] : cp[p] + a.w * acc[j];
    }
}

// out[f][k][l][l'] = sum over the frame's chunks b = 0 .. compat_chunks(n_points[f]) - 1, in that order, of cpart[k][f][b][l][l']
// (bstride: the chunks the partials have room for, the sweep's grid); one owner per (frame, term, entry).  A handle is one frame of
// bstride chunks.  A frame of 0 points gets 0.
// counts != null (section 2k): so does a frame with t_f = 0 -- no iteration wrote its cpart, and what an earlier call left there is not
// read.
__global__ void __launch_bounds__(kBwdBlock) k_compat_reduce(const float *__restrict__ cpart, const int *__restrict__ n_points, int K, int F,
                                                           int bstride, int LL, float *__restrict__ out,
                                                           const int *__restrict__ counts, int T)
{
    const long idx = (long)blockIdx.x * kBwdBlock + threadIdx.x;
    if (idx >= (long)F * K * LL) return;
    const int f = (int)(idx / ((long)K * LL));
    const int e = (int)(idx - (long)f * K * LL);
    const int k = e / LL, p = e - k * LL;
    const int N = n_points[f], B = N > 0 && (!counts || frame_count(counts, f, T) > 0) ? compat_chunks(N) : 0;
    const float *cp = cpart + ((size_t)k * F + f) * bstride * LL + p;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += cp[(size_t)b * LL];
    out[idx] = s;
}

// ---- the sums over the frames (section 2h) ---------------------------------------------------------------------------------------
// out[j] = ((x[0][j] + x[1][j]) + ..) + x[F-1][j], j < n, x [F][n]: the frames in ascending order, in fp32, one owner per entry and no
// atomics -- the order is part of section 2h's contract (0 for F = 0).  A workgroup owns kSumEntries entries and walks the frames in
// tiles of kSumFrames: all lanes load the tile (n <= kSumEntries: one contiguous run of the array; else runs of kSumEntries floats),
// lane j then adds its column of the tile, frame by frame (row stride kSumEntries + 1: the lanes of a row on 64 banks).  Frames at
// or beyond F are never read.
constexpr int kSumEntries = 64, kSumFrames = 64;
__global__ void __launch_bounds__(kBwdBlock) k_sum_frames(const float *__restrict__ x, int F, int n, float *__restrict__ out)
{
    __shared__ float tile[kSumFrames * (kSumEntries + 1)];
    const int tid = threadIdx.x, j0 = blockIdx.x * kSumEntries, ne = min(kSumEntries, n - j0);
    float acc = 0.0f;
    for (int f0 = 0; f0 < F; f0 += kSumFrames) {            // (uniform bounds: every lane meets every barrier)
        const int nf = min(kSumFrames, F - f0);
        for (int idx = tid; idx < nf * ne; idx += kBwdBlock) {
            const int fr = idx / ne, e = idx - fr * ne;
            tile[fr * (kSumEntries + 1) + e] = x[(size_t)(f0 + fr) * n + j0 + e];
        }
        __syncthreads();
        if (tid < ne) {
            int fr = 0;
            if (f0 == 0) acc = tile[tid], fr = 1;          // (the sum starts from frame 0's value, not from +0)
            for (; fr < nf; ++fr) acc = acc + tile[fr * (kSumEntries + 1) + tid];
        }
        __syncthreads();
    }
    if (tid < ne) out[j0 + tid] = acc;
}

}  // namespace

// (engine.h: the one-launch route of fused_backward_general.hip forms section 2h's sums with it too)
void launch_sum_frames(const float *x, int F, int n, float *out, hipStream_t s)
{
    if (n > 0) k_sum_frames<<<(unsigned)((n + kSumEntries - 1) / kSumEntries), kBwdBlock, 0, s>>>(x, F, n, out);
}

namespace {

// Q[f] <- hist[t_f][f] for every frame with t_f < T, element by element over the frame's maxN x L floats (every hist[t] is a copy of
// the whole of Q); a frame at the cap keeps the stepped Q.
__global__ void __launch_bounds__(kBwdBlock) k_restore_counted_q(const int *__restrict__ counts, int T, size_t fs, size_t slice,
                                                               const float *__restrict__ hist, float *__restrict__ Q)
{
    const int f = blockIdx.y;
    const int tf = frame_count(counts, f, T);
    const size_t idx = (size_t)blockIdx.x * kBwdBlock + threadIdx.x;
    if (tf >= T || idx >= fs) return;
    Q[f * fs + idx] = hist[(size_t)tf * slice + f * fs + idx];
}

// order[r] = f with r = #{g : t_g > t_f} + #{g < f : t_g == t_f}: every frame's rank among the clamped counts, longest first, ties by
// frame -- a permutation of 0 .. F-1 whatever the counts hold.  A lane per frame; the counts pass through LDS in tiles of a workgroup.
__global__ void __launch_bounds__(kBwdBlock) k_order_by_count(const int *__restrict__ counts, int F, int T, int *__restrict__ order)
{
    __shared__ int tile[kBwdBlock];
    const int f = blockIdx.x * kBwdBlock + threadIdx.x;
    const int tf = f < F ? frame_count(counts, f, T) : 0;
    int rank = 0;
    for (int g0 = 0; g0 < F; g0 += kBwdBlock) {            // (uniform bounds: every lane meets every barrier)
        const int g = g0 + (int)threadIdx.x;
        tile[threadIdx.x] = g < F ? frame_count(counts, g, T) : -1;
        __syncthreads();
        const int n = min(kBwdBlock, F - g0);
        for (int j = 0; j < n; ++j) rank += tile[j] > tf || (tile[j] == tf && g0 + j < f);
        __syncthreads();
    }
    if (f < F) order[rank] = f;
}

}  // namespace

void launch_order_by_count(const int *counts, int F, int T, int *order, hipStream_t s)
{
    if (F > 0) k_order_by_count<<<(unsigned)((F + kBwdBlock - 1) / kBwdBlock), kBwdBlock, 0, s>>>(counts, F, T, order);
}

void launch_restore_counted_q(const CrfDev &c, const BackwardArea &ar, int T, const int *counts, hipStream_t s)
{
    const size_t fs = (size_t)c.maxN * c.L;
    if (T <= 0 || !fs || !c.F) return;
    k_restore_counted_q<<<dim3((unsigned)((fs + kBwdBlock - 1) / kBwdBlock), (unsigned)c.F), kBwdBlock, 0, s>>>(counts, T, fs, ar.slice, ar.hist,
                                                                                                            c.Q);
}

namespace {

// ---- the feature part (sections 1d and 2d) ----------------------------------------------------------------------------------
// gb[i][c] += scale * <row_i, val[v_ic]> for every point i < n_points[f] and corner c: a slice without the sum over the corners.
// A row is G lanes as in k_softmax_bwd (lane c of the row holds labels 4c .. 4c+3); every id first, then every gather, then the
// dot products, each summed over the labels in order 0 .. L-1.  row == null: all ones (the norm part, L = 1).
// fac != null (section 1m): the row is fac[f][i] * row_i, every product rounded once -- the splat side's input row b_k . Q_{t-1} of a
// term with a factor in front of its filter, exactly the row the forward's splat formed.  Without it (a uniform branch) the bits it gave.
// counts != null (section 2l; the sweep's launches only, the norm part passes none): a frame is idle while t > t_f -- its workgroups
// leave on blockIdx.y alone, before the row sums' shuffles, with nothing added to gb.  For such a frame phi_k is scratch (k_softmax_bwd
// returned without writing the transposed filter's input): the slice side's row and the splat side's values would both be garbage.
struct CornerArgs {
    const int *n_points;
    int L;
    size_t fs;                   // floats between frames of row
    const float *row;            // [F][.][L]
    const float *val;            // the kernel's blurred values (launch_filter / launch_filter_values1)
    float scale;
    float *gb;                   // [F][Epad]
    const float *fac;            // [F][nstride] or null
    int nstride;
    const int *counts;           // [F] or null (section 2l): the frame's own iteration count, clamped to [0, cap] by frame_count
    int t, cap;                  // ... the sweep's iteration of this launch and the counts' cap
};

template <int G>
__global__ void __launch_bounds__(kBwdBlock) k_corner_dot(KernelDev kd, CornerArgs a)
{
    const int f = blockIdx.y;
    if (a.counts && a.t > frame_count(a.counts, f, a.cap)) return;   // an idle frame (uniform over the workgroup)
    const int N = a.n_points[f], L = a.L, D1 = kd.D1;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, first = lane - sub;
    const int i = blockIdx.x * (kBwdBlock / G) + (int)threadIdx.x / G;
    const bool live = i < N;
    const int l0 = sub * 4;
    const size_t e0 = (size_t)f * kd.Epad + (size_t)(live ? i : 0) * D1;
    const float *vf = a.val + (size_t)f * kd.vstride + kd.vbase + l0;
    bool has[4];
    float r[4];
    int o[kMaxD + 1];
    float x[kMaxD + 1][4];
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < D1) o[j] = live ? kd.offset[e0 + j] : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        has[u] = live && l0 + u < L;
        r[u] = has[u] ? (a.row ? a.row[f * a.fs + (size_t)i * L + l0 + u] : 1.0f) : 0.0f;
    }
    if (a.fac) {
        const float b = live ? a.fac[(size_t)f * a.nstride + i] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = has[u] ? b * r[u] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < D1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) x[j][u] = has[u] ? vf[(long)o[j] * L + u] : 0.0f;
        }
#pragma unroll
    for (int j = 0; j <= kMaxD; ++j)
        if (j < D1) {                                       // (uniform: the shuffles of the row sum see every lane)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = r[u] * x[j][u];
            const float sj = row_sum_ordered<G>(v, L, first);
            if (live && sub == 0) a.gb[e0 + j] = a.gb[e0 + j] + a.scale * sj;
        }
}

void launch_corner_dot(const KernelDev &kd, const CrfDev &c, int rows, int L, const float *row, size_t fs, const float *val, float scale,
                       float *gb, hipStream_t s, const float *fac = nullptr, BwdCounts cn = BwdCounts{nullptr, 0, 0})
{
    CornerArgs a{c.n_points, L, fs, row, val, scale, gb, fac, c.maxN, cn.counts, cn.t, cn.cap};
    const dim3 grid((unsigned)std::max(backward_blocks(rows, L), 1), (unsigned)c.F);
    with_bwd_lanes(L, [&](auto lanes) { k_corner_dot<decltype(lanes)::value><<<grid, kBwdBlock, 0, s>>>(kd, a); });
}

// gn[i] <- a_i = -n_i^2 g_n[i]: dL/d Phi_k(1)_i, the input of the norm part's filter pair.  norm: the term's TRUE norm n_k, [F][maxN]
// (under section 1g's modes kd.norm is the factor behind the filter, not n_k).  g_n = gn as the sweep accumulated it -- the post
// adjoint of an AFTER term, the pre adjoint of a BEFORE term -- or, root != null (SYMMETRIC, section 1m: both adjoints in the one
// accumulator, root = s = sqrtf(n)), g_n = gn * (0.5f / s[i]): ds/dn = 1 / (2 s).
__global__ void __launch_bounds__(kBwdBlock) k_norm_adjoint(KernelDev kd, const int *__restrict__ n_points, const float *__restrict__ norm,
                                                          const float *__restrict__ root, float *__restrict__ gn)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBwdBlock + threadIdx.x;
    if (i >= n_points[f]) return;
    const float n = norm[(size_t)f * kd.maxN + i];
    float *g = gn + (size_t)f * kd.maxNpad + i;
    float v = *g;
    if (root) v = v * (0.5f / root[(size_t)f * kd.maxN + i]);
    *g = -(n * n) * v;
}

// dL/df [F][maxN][D] from dL/db (gb, laid out as KernelDev::bary).  With v_j = (el_j - rem0_j) / (D+1) and p_j = D - rank_j, corner
// q receives +v of the coordinate with p = q and -v of the one with p = q - 1, cell D+1 folding into corner 0 (point_record), so
// dL/dv_j = gb[p_j] - gb[(p_j + 1) mod (D+1)]; el_0 = sum_m cf_m, el_j = sum_{m >= j} cf_m - j cf_{j-1}, cf_m = f_m scale_m, so
// dL/df_m = scale_m ((dL/del_0 + .. + dL/del_m) - (m+1) dL/del_{m+1}).  The simplex is the build's (lattice_simplex on the same
// features: the same ranks).  Rows [n_points[f], rows) are written 0.
template <int D>
__global__ void __launch_bounds__(kBwdBlock) k_corner_to_feature(KernelDev kd, const int *__restrict__ n_points, int rows,
                                                               const float *__restrict__ gb, float *__restrict__ out)
{
    constexpr int D1 = D + 1;
    const int f = blockIdx.y;
    const int i = blockIdx.x * kBwdBlock + threadIdx.x;
    if (i >= rows) return;
    float *op = out + ((size_t)f * kd.maxN + i) * D;
    if (i >= n_points[f]) {
#pragma unroll
        for (int m = 0; m < D; ++m) op[m] = 0.0f;
        return;
    }
    float feat[D], g[D1];
    const float *fp = kd.feat + ((size_t)f * kd.maxN + i) * D;
    const float *gp = gb + (size_t)f * kd.Epad + (size_t)i * D1;
#pragma unroll
    for (int m = 0; m < D; ++m) feat[m] = fp[m];
#pragma unroll
    for (int q = 0; q < D1; ++q) g[q] = gp[q];
    float el[D1], rem0[D1], rank[D1];
    lattice_simplex<D>(feat, kd.scale, kd.inv_dp1, el, rem0, rank);
    float gel[D1];
#pragma unroll
    for (int j = 0; j < D1; ++j) {
        const int p = (int)((float)D - rank[j]);
        const int pn = p == D ? 0 : p + 1;
        float gp0 = 0.0f, gp1 = 0.0f;                       // (selects, so that g stays in registers)
#pragma unroll
        for (int q = 0; q < D1; ++q) {
            gp0 = q == p ? g[q] : gp0;
            gp1 = q == pn ? g[q] : gp1;
        }
        gel[j] = (gp0 - gp1) * kd.inv_dp1;
    }
    float run = gel[0];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        if (m) run += gel[m];
        op[m] = (run - (float)(m + 1) * gel[m + 1]) * kd.scale[m];
    }
}

void launch_corner_to_feature(const KernelDev &kd, const CrfDev &c, int rows, const float *gb, float *out, hipStream_t s)
{
    const dim3 grid((unsigned)std::max((rows + kBwdBlock - 1) / kBwdBlock, 1), (unsigned)c.F);
    with_dims<1, 8>(kd.d, [&](auto d) { k_corner_to_feature<decltype(d)::value><<<grid, kBwdBlock, 0, s>>>(kd, c.n_points, rows, gb, out); });
}

}  // namespace

size_t backward_stride(int n, int L) { return (size_t)((n + 3) & ~3) * L; }

int backward_blocks(int n, int L) { return (n + kBwdBlock / bwd_lanes(L) - 1) / (kBwdBlock / bwd_lanes(L)); }

int backward_compat_blocks(int n) { return compat_chunks(n); }

size_t backward_layout(const BackwardRequest &rq, const CrfDev &c, const KernelDev *kds, size_t slice, int rows, float *base,
                       BackwardArea *ar)
{
    const size_t F = (size_t)c.F, K = (size_t)c.K, LL = (size_t)c.L * c.L;
    size_t used = 0;
    auto take = [&](size_t floats) {                      // the next part: its address in the area (null without one)
        float *p = base ? base + used : nullptr;
        used += floats;
        return p;
    };
    BackwardArea a{};
    a.slice = slice;
    a.hist = take((size_t)rq.T * slice);
    a.phi = take(K * slice);
    a.G = take(slice);
    a.partial = take((size_t)std::max(rq.T, 1) * K * F * std::max(backward_blocks(rows, c.L), 1));
    if (!rq.grad_unary) a.gU = take(slice);
    for (size_t k = 0; k < K && rq.grad_features; ++k)
        if (rq.grad_features[k]) {
            const size_t nb = F * kds[k].Epad, nn = F * kds[k].maxNpad;
            a.gb[k] = take(nb);
            a.gn[k] = take(nn);
            a.feat_floats[k] = nb + nn;
        }
    if (rq.compat_form) {
        a.gam = take(slice);
        a.cpart = take(K * F * backward_compat_blocks(rows) * LL);
    }
    if (rq.grad_model) {                                  // (section 2h: the per-frame values the sums are formed from)
        if (!rq.grad_weights) a.gW = take(F * K);
        if (!rq.grad_compat) a.gC = take(F * K * LL);
    }
    if (ar) *ar = a;
    return used * sizeof(float);
}

void launch_backward_sweep(const CrfDev &c, const KernelDev *kds, const int *maxV, int rows, const BackwardRequest &rq,
                           const BackwardArea &ar, const float *const *compat, hipStream_t s, const float *const *pre,
                           const BackwardModes *modes)
{
    const int T = rq.T;
    const float relax = rq.relax;
    float *const *grad_features = rq.grad_features;
    // (section 2h: the per-frame values behind grad_model are formed in the area where the caller left their own array out)
    float *const grad_weights = rq.grad_weights ? rq.grad_weights : ar.gW, *const grad_compat = rq.grad_compat ? rq.grad_compat : ar.gC;
    const int K = c.K, L = c.L, F = c.F;
    const size_t slice = ar.slice, fs = (size_t)c.maxN * L;
    const int nblk = std::max(backward_blocks(rows, L), 1);
    BwdArgs a{};
    a.n_points = c.n_points;
    a.L = L;
    a.rows = rows;
    a.nstride = c.maxN;
    a.fs = fs;
    a.slice = slice;
    a.unary = c.unary;
    a.phi = ar.phi;
    a.G = ar.G;
    a.gU = rq.grad_unary ? rq.grad_unary : ar.gU;
    BwdWeights wk{};
    BwdPre bp{};
    bp.nstride = c.maxN;
    for (int k = 0; k < K; ++k) {
        a.norm[k] = kds[k].norm;                            // (section 1g: the caller's copy points it at a_k)
        a.w[k] = wk.w[k] = kds[k].w;
        bp.p[k] = pre ? pre[k] : nullptr;
    }
    // the compatibility part (section 1e): some term has a matrix, or dL/dmu is asked for -- ar.gam and ar.cpart are set
    const bool cmode = rq.compat_form;
    const int cblk = backward_compat_blocks(rows);
    for (int k = 0; k < K && cmode; ++k) a.compat[k] = compat ? compat[k] : nullptr;
    a.gam = ar.gam;
    a.counts = rq.counts;                                   // (section 2j; null: every frame at T)
    a.cap = T;
    // the feature part: terms with a gradient array (T >= 1; the caller has zeroed their ar.gb / ar.gn)
    // (section 1m, modes != null: ar.gn[k] takes the post adjoint of an AFTER or SYMMETRIC term from k_softmax_bwd and the pre adjoint
    // of a BEFORE or SYMMETRIC one from k_bwd_combine_adjoint, which runs in k_bwd_combine<true>'s place while padj is set)
    bool feat = false, padj = false;
    float *gf[kBwdMaxK] = {};
    BwdPreAdjoint pa{};
    for (int k = 0; k < K && grad_features && T >= 1; ++k)
        if (grad_features[k]) {
            const int mode = modes ? modes->mode[k] : LCCRF_NORMALIZE_AFTER;
            gf[k] = grad_features[k];
            if (mode == LCCRF_NORMALIZE_AFTER || mode == LCCRF_NORMALIZE_SYMMETRIC) a.gn[k] = ar.gn[k];
            if (mode == LCCRF_NORMALIZE_BEFORE || mode == LCCRF_NORMALIZE_SYMMETRIC) pa.gn[k] = ar.gn[k], padj = true;
            a.gnstride = pa.gnstride = kds[k].maxNpad;
            feat = true;
        }
    const dim3 cgrid((unsigned)std::max<size_t>(((size_t)rows * L + kBwdBlock - 1) / kBwdBlock, 1), (unsigned)F);
    for (int t = T; t >= 1; --t) {
        const float *qprev = ar.hist + (size_t)(t - 1) * slice;
        const float *val[kBwdMaxK];                        // (B S Q_{t-1}) of every term, in the term's own value buffer
        for (int k = 0; k < K; ++k) launch_filter(kds[k], c, maxV[k], qprev, ar.phi + k * slice, 0, s, 0, &val[k], nullptr, bp.p[k]);
        a.K = K;
        a.relax = relax;
        a.first = t == T;
        a.t = t;
        a.partial = K ? ar.partial + (size_t)(t - 1) * K * F * nblk : nullptr;
        const BwdCounts cn{rq.counts, t, T};               // (sections 2j - 2l; counts null: every frame takes every launch)
        // (first uses in the order compat, plain, feature, both: the order of the kernels' instantiation, and so of the code object)
        if (cmode && !feat) launch_softmax_bwd<kBwdCompat>(a, F, s);
        else if (!feat) launch_softmax_bwd<kBwdPlain>(a, F, s);
        else if (!cmode) launch_softmax_bwd<kBwdFeat>(a, F, s);
        else launch_softmax_bwd<kBwdCompatFeat>(a, F, s);
        for (int k = 0; k < K; ++k) {
            if (cmode) {                                   // phi_k: Phi_k(Q_{t-1}) -> mu_k^T (n_k gamma_t); dL/dmu_k's partials
                CompatArgs ca{c.n_points, L, t == T, c.maxN, fs, ar.gam, kds[k].norm, ar.phi + k * slice, a.compat[k], kds[k].w,
                              grad_compat ? ar.cpart + (size_t)k * F * cblk * L * L : nullptr, rq.counts, t, T};
                k_compat_bwd<<<dim3((unsigned)cblk, (unsigned)F), kBwdBlock, 0, s>>>(ca);
            }
            // (section 1f: the slice side's upstream row is what k_compat_bwd has just left in phi_k, n_k (mu_k^T gamma_t))
            const float cs = kds[k].alpha * kds[k].w;
            if (gf[k]) launch_corner_dot(kds[k], c, rows, L, ar.phi + k * slice, fs, val[k], cs, ar.gb[k], s, nullptr, cn);   // slice side
            const float *valt;                             // (B^T S n_k gamma_t)
            launch_filter(kds[k], c, maxV[k], ar.phi + k * slice, ar.phi + k * slice, 0, s, 1, &valt);
            if (gf[k]) launch_corner_dot(kds[k], c, rows, L, qprev, fs, valt, cs, ar.gb[k], s, bp.p[k], cn);      // splat side
        }
        if (padj) {
            pa.q = qprev;
            const dim3 rgrid((unsigned)nblk, (unsigned)F);
            with_bwd_lanes(L, [&](auto lanes) {
                k_bwd_combine_adjoint<decltype(lanes)::value><<<rgrid, kBwdBlock, 0, s>>>(c.n_points, L, K, ar.phi, slice, fs, wk, 1.0f - relax,
                                                                                       ar.G, bp, pa, cn);
            });
        } else if (pre) k_bwd_combine<true><<<cgrid, kBwdBlock, 0, s>>>(c.n_points, L, K, ar.phi, slice, fs, wk, 1.0f - relax, ar.G, bp, cn);
        else k_bwd_combine<false><<<cgrid, kBwdBlock, 0, s>>>(c.n_points, L, K, ar.phi, slice, fs, wk, 1.0f - relax, ar.G, bp, cn);
    }
    // dL/dU -= P_0 (G_0 - <G_0, P_0>), P_0 = Q_0 = softmax(-U)
    a.K = 0;
    a.relax = 1.0f;
    a.first = T == 0;
    a.t = 0;                                                // (with counts: the first step of the frames with t_f = 0)
    a.partial = nullptr;
    launch_softmax_bwd<kBwdPlain>(a, F, s);
    if (grad_compat && K && T >= 1)
        k_compat_reduce<<<(unsigned)(((size_t)F * K * L * L + kBwdBlock - 1) / kBwdBlock), kBwdBlock, 0, s>>>(ar.cpart, c.n_points, K, F, cblk,
                                                                                                            L * L, grad_compat, rq.counts, T);
    // the norm part, <a_k, Phi_k(1)> with a_k = -n_k^2 g_n[k] (value width 1), and dL/db -> dL/df
    // (section 1m: g_n from the adjoints by the term's mode, n_k the true norm; a term without a norm factor has no norm part)
    // (section 2l: these launches take no counts.  A frame with t_f = 0 under a cap >= 1 runs through them on the caller's memset:
    // a_i = -(n * n) * +0 = -0 (times a finite, positive 0.5f / s under SYMMETRIC); the first corner dot forms 0.0f + (-0 * x) = +0 and
    // adds alpha * +0 to +0; the transposed filter of a field of -0 leaves +-0 in every vertex, whose corner dot is 0.0f + 1.0f * (+-0) =
    // +0 again; so every gb is +0, every gel (+0 - +0) * inv_dp1 = +0 and every dL/df (+0 - (m + 1) * +0) * scale_m = +0, scale_m > 0:
    // the bits of the handle's memset at T = 0, with no branch.)
    for (int k = 0; k < K; ++k) {
        if (!gf[k]) continue;
        const KernelDev &kd = kds[k];
        const int mode = modes ? modes->mode[k] : LCCRF_NORMALIZE_AFTER;
        if (mode == LCCRF_NORMALIZE_NONE) {
            launch_corner_to_feature(kd, c, rows, ar.gb[k], gf[k], s);
            continue;
        }
        k_norm_adjoint<<<dim3((unsigned)std::max((rows + kBwdBlock - 1) / kBwdBlock, 1), (unsigned)F), kBwdBlock, 0, s>>>(
            kd, c.n_points, modes ? modes->norm[k] : kd.norm, mode == LCCRF_NORMALIZE_SYMMETRIC ? bp.p[k] : nullptr, ar.gn[k]);
        const float *ones = launch_filter_values1(kd, c, maxV[k], nullptr, 0, s, 0);
        launch_corner_dot(kd, c, rows, 1, ar.gn[k], (size_t)kd.maxNpad, ones, kd.alpha, ar.gb[k], s);
        const float *adj = launch_filter_values1(kd, c, maxV[k], ar.gn[k], kd.maxNpad, s, 1);
        launch_corner_dot(kd, c, rows, 1, nullptr, 0, adj, kd.alpha, ar.gb[k], s);
        launch_corner_to_feature(kd, c, rows, ar.gb[k], gf[k], s);
    }
    if (grad_weights && K)
        k_bwd_reduce<<<dim3((unsigned)K, (unsigned)F), kBwdBlock, 0, s>>>(ar.partial, c.n_points, K, T, kBwdBlock / bwd_lanes(L), nblk,
                                                                       grad_weights, rq.counts);
    if (rq.grad_model) {                                  // the sums over the frames: the K weights, then the K * L * L entries
        launch_sum_frames(grad_weights, F, K, rq.grad_model, s);
        launch_sum_frames(grad_compat, F, K * L * L, rq.grad_model + K, s);
    }
}

}  // namespace lccrf

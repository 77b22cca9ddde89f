// fused_backward_features.hip -- the gradients of mean-field inference of a tracker-sized two-label frame WITH the gradients with respect
// to the kernel features (include/lccrf.h sections 1d and 2d) in ONE launch: one 1024-lane workgroup per frame, the lattices' values in
// LDS.  Opt-in (LCCRF_OPT_FUSED_BACKWARD_FEATURES, include/lccrf.h section 1l); notes/fused_backward.md section 7.  k_backward
// (fused_backward.hip) keeps the requests without a feature array and the code it has.
//
// What one launch does, per frame (blockIdx.x): everything k_backward does -- the prologue, Q_0, the replay with `hist`, the sweep, the
// softmax backward of Q_0, the reduction of dL/dw, the zero rows of dL/dU; the same bits in Q, dL/dU and dL/dw -- and for every term k
// with a feature array in the request (gF[k], uniform), with the streaming sweep's arithmetic (meanfield_backward.hip):
//     per iteration t = T .. 1 and point i of the lane
//         g_n[k][i] += w_k <gamma_t,i, Phi_k(Q_{t-1})_i>                  softmax_bwd<1, kBwdFeat>: the labels in order from 0.0f
//         g_b[k][i][c] += (alpha_k w_k) <n_k gamma_t,i, (B S Q_{t-1})[v_ic]>   k_corner_dot, slice side: the forward filter's vertex values
//                                                                         the slice gathers anyway, before the transposed filter overwrites them
//         g_b[k][i][c] += (alpha_k w_k) <Q_{t-1},i, (B^T S n_k gamma_t)[v_ic]>   k_corner_dot, splat side: the transposed filter's values
//     behind the sweep, the norm part: a_i = -n_i^2 g_n[k][i] (k_norm_adjoint), a forward filter of all ones and a transposed filter of
//         a_k of value width 1 -- label 0 of the loop's two-label filter with label 1 at 0: every row sum and blur pass treats the labels
//         independently -- each with its corner dots at scale alpha_k (row a_i; row 1), then k_corner_to_feature<2>'s arithmetic per point
//         and the zero rows of dL/df_k.
// Every g_b[k][i][c] and g_n[k][i] has one owner, the lane that owns the point, and the sweep's order of additions (t = T .. 1, slice
// side then splat side, the norm part last).  They live in the area's gb / gn (L2-resident), read and written per iteration by that
// lane as dL/dU is: 16 more registers per lane do not fit the two-term chain instantiations.  The kernel initialises them itself --
// the first iteration adds to a literal 0.0f, as the sweep adds to the host's memset -- so a rebound batch sees no stale value.
//
// Uniform arguments the sweep needs only here and there (the feature pointers, the weights, the norms' pointers) are read from the
// kernarg segment where they are used (late(), as k_backward_general does): kept from the kernel's entry they are live around the
// whole sweep and the two-term instantiations have no scalar register left for them.
//
// With per-frame counts (include/lccrf.h section 2l) T above is the frame's own t_f = min(max(counts[f], 0), T), loaded once per
// workgroup -- a uniform value, so every barrier stays uniform -- and workgroup i takes frame order[i], the frames sorted by descending
// t_f on the device (k_order_by_count, meanfield_backward.hip), as k_backward and k_backward_general do: which workgroup runs a frame
// changes no bit of it.  hist and partial keep their [T][..] layout.  A frame with t_f = 0 never initialises its g_b / g_n -- they may
// hold an earlier call's values -- so it skips the norm part and writes +0 into all `rows` rows of every dL/df_k: the bits of the
// handle's memset at T = 0.  The counts and the order are runtime arguments read once at the kernel's entry and dead behind it (t_f
// takes a.T's scalar register): no instantiation more.
//
// Scope: Potts terms normalised AFTER, K in {1, 2} 2-D terms, frames of up to 2 x 1024 active points, kernel 0 with short rows or chain
// rows: 8 instantiations.  T >= 1 (the caller streams T = 0: its memset to exactly 0 is already right); a frame's own t_f may be 0.
#include <cstddef>

#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"
#include "fused_backward_common.h"

namespace lccrf {

namespace {

using namespace fl;

struct BackwardFeatureArgs {
    KernelDev kd[kMaxFusedK];
    FusedLayout lay;
    int T, rows;                          // rows: points per frame of gU and gF (rows [n_points[f], rows) are written 0)
    int bstride;                          // partials per (iteration, term, frame): the area's row
    float relax;
    size_t slice;                         // floats between the iterations of hist
    const float *grad_prob;               // [F][maxN][2] dL/dQ_T
    float *hist;                          // [T][slice]
    float *G;                             // [F][maxN][2]
    float *gU;                            // [F][maxN][2]
    float *gW;                            // [F][K] or null
    float *partial;                       // [T][K][F][bstride]
    float *gF[kMaxFusedK];                // [F][maxN][2] dL/df_k, or null: term k does no feature work
    float *gb[kMaxFusedK];                // [F][Epad] dL/d(corner weight), laid out as KernelDev::bary (BackwardArea::gb)
    float *gn[kMaxFusedK];                // [F][maxNpad] the per-point sum behind the norm's gradient (BackwardArea::gn)
    const int *counts;                    // [F] or null (section 2l): frame f runs min(max(counts[f], 0), T) iterations, T the layout's
    const int *order;                     // [F] or null: workgroup i takes frame order[i] (a permutation: the longest counts first)
};

struct KernArgs { CrfDev c; BackwardFeatureArgs a; };   // two by-value parameters, each at its natural alignment
typedef const __attribute__((address_space(4))) BackwardFeatureArgs *LateArgs;
__device__ __forceinline__ LateArgs late()
{
    const __attribute__((address_space(4))) unsigned char *p =
        (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (LateArgs)(p + offsetof(KernArgs, a));
}

// ... and the frame's rows of the [F][maxN][2] arrays the sweep re-reads per point, formed from the late arguments where a point region
// opens: as pointers kept from the kernel's entry they are eight scalar registers around the whole sweep
struct FrameRows { const float2 *un, *gT; float2 *G, *gU; };
__device__ __forceinline__ FrameRows frame_rows(int f)
{
    const __attribute__((address_space(4))) unsigned char *p =
        (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    const __attribute__((address_space(4))) CrfDev *c = (const __attribute__((address_space(4))) CrfDev *)(p + offsetof(KernArgs, c));
    const LateArgs a = (LateArgs)(p + offsetof(KernArgs, a));
    const size_t fo = (size_t)f * c->maxN;
    return FrameRows{reinterpret_cast<const float2 *>(c->unary) + fo, reinterpret_cast<const float2 *>(a->grad_prob) + fo,
                     reinterpret_cast<float2 *>(a->G) + fo, reinterpret_cast<float2 *>(a->gU) + fo};
}

// g[c] += scale * <row, x[c]> per corner, the labels in order from a literal 0.0f (k_corner_dot at L = 2); first: g[c] was the host's +0
__device__ __forceinline__ void corner_dots2(float *g, bool first, float scale, const float2 row, const float2 (&x)[kD1])
{
#pragma unroll
    for (int c = 0; c < kD1; ++c) {
        float sj = 0.0f;
        sj += row.x * x[c].x;
        sj += row.y * x[c].y;
        const float was = first ? 0.0f : g[c];
        g[c] = was + scale * sj;
    }
}

// label 0 of the three vertex values of point slot s under term k: what a width-1 filter left (launch_filter_values1)
template <int PPT, int K>
__device__ __forceinline__ void corner_values1(const unsigned char *smem, const FusedLayout &lay, const PointRegs<PPT, K> &pr, int s, int k,
                                               float (&x)[kD1])
{
    const float2 *val = reinterpret_cast<const float2 *>(smem + lay.val[k][kD1 & 1]);
    x[0] = val[pr.ix[s][k][0] & 0xffffu].x;
    x[1] = val[pr.ix[s][k][0] >> 16].x;
    x[2] = val[pr.ix[s][k][1] & 0xffffu].x;
}

// A filter of the terms in `mask` (uniform, not 0) on the inputs xin: the loop's splat and blur, forward or TRANSPOSEd.  The terms
// outside the mask do no work.
template <int PPT, int K, int CH, bool TR>
__device__ __forceinline__ void filter_terms(int mask, unsigned char *smem, const FusedLayout &lay, const int (&V)[K], int N, int tid,
                                             const PointRegs<PPT, K> &pr, const ChainLane &cl, Instr &ins, const float2 (*xin)[K])
{
    if constexpr (K == 1) {
        splat_blur<PPT, K, CH, true, kNT, 1, true, false, TR, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
    } else {
        if (mask == 3) splat_blur<PPT, K, CH, true, kNT, 3, true, false, TR, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
        else if (mask == 1) splat_blur<PPT, K, CH, true, kNT, 1, true, false, TR, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
        else splat_blur<PPT, K, CH, true, kNT, 2, true, false, TR, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
    }
}

// dL/df of one point of a 2-D term from its dL/db g[0..2]: k_corner_to_feature<2>'s arithmetic (meanfield_backward.hip), the simplex
// recomputed with the build's lattice_simplex
__device__ __forceinline__ float2 corner_to_feature2(const float (&feat)[2], const float *scale, float inv_dp1, const float (&g)[kD1])
{
    constexpr int D = 2, D1 = 3;
    float el[D1], rem0[D1], rank[D1];
    lattice_simplex<D>(feat, scale, inv_dp1, el, rem0, rank);
    float gel[D1];
#pragma unroll
    for (int j = 0; j < D1; ++j) {
        const int p = (int)((float)D - rank[j]);
        const int pn = p == D ? 0 : p + 1;
        float gp0 = 0.0f, gp1 = 0.0f;
#pragma unroll
        for (int q = 0; q < D1; ++q) {
            gp0 = q == p ? g[q] : gp0;
            gp1 = q == pn ? g[q] : gp1;
        }
        gel[j] = (gp0 - gp1) * inv_dp1;
    }
    float out[D];
    float run = gel[0];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        if (m) run += gel[m];
        out[m] = (run - (float)(m + 1) * gel[m + 1]) * scale[m];
    }
    return make_float2(out[0], out[1]);
}

template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_backward_features(CrfDev c, BackwardFeatureArgs a)
{
    constexpr int D1 = kD1, NT = kNT, ALL = (1 << K) - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (section 2l) the frame of this workgroup and its own iteration count: uniform values, one load each per workgroup
    const int f = a.order ? a.order[blockIdx.x] : blockIdx.x;
    int tid = threadIdx.x;
    const int N = c.n_points[f];
    const int T = a.counts ? min(max(a.counts[f], 0), a.T) : a.T;
    Instr ins{nullptr, 0, 0, 0, 0};
    const size_t fo = (size_t)f * c.maxN;                 // the frame's first row of every [F][maxN][2] array
    float2 *gU = reinterpret_cast<float2 *>(a.gU) + fo;

    for (int i = max(N, 0) + tid; i < a.rows; i += NT) gU[i] = make_float2(0.f, 0.f);   // rows beyond the frame's points: dL/dU = 0
#pragma unroll
    for (int k = 0; k < K; ++k)                            // ... and dL/df_k = 0 (k_corner_to_feature); at t_f = 0 every row: nothing
        if (a.gF[k])                                       //     depends on the features, and no norm part runs for the frame
            for (int i = (T == 0 ? 0 : max(N, 0)) + tid; i < a.rows; i += NT)
                a.gF[k][((size_t)f * a.kd[k].maxN + i) * 2] = a.gF[k][((size_t)f * a.kd[k].maxN + i) * 2 + 1] = 0.0f;
    if (N <= 0) {                         // nothing to differentiate (and nothing below may index an empty frame)
        if (a.gW && tid < K) a.gW[(size_t)f * K + tid] = 0.0f;
        return;
    }

    PointRegs<PPT, K> pr;
    int V[K];
#pragma unroll
    for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    const FusedLayout &lay = a.lay;

    unsigned pk[PPT][K][D1];              // (vertex id + 1) | place in the row << 16
#include "fused_prologue.inc"
    __syncthreads();

    ChainLane cl{0u, 0u};
    if (CH != 0 && chain_k<CH>(lay, 0)) cl = chain_setup(smem, lay, V[0], tid);
    start_inference<PPT, K, NT>(pr, N, tid);
    place_products<PPT, K, CH, NT>(smem, lay, N, tid, pk, pr);

    float alpha[K];
#pragma unroll
    for (int k = 0; k < K; ++k) alpha[k] = a.kd[k].alpha;

    // ---- the replay: inference(T, 0, relax), keeping Q_0 .. Q_{T-1} -------------------------------------------------------------
    const size_t hs = a.slice / 2;        // float2 between the iterations of hist
    float2 *hist = reinterpret_cast<float2 *>(a.hist) + fo;
    for (int t = 0; t < T; ++t) {
        opaque(pr);
#pragma unroll
        for (int s = 0; s < PPT; ++s)
            if (tid + s * NT < N) hist[(size_t)t * hs + tid + s * NT] = pr.q[s];
        splat_blur<PPT, K, CH, true, NT, ALL, true>(smem, lay, V, N, tid, pr, cl, ins);
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            if (tid + s * NT < N) {
                float nx[2] = {-pr.un[s].x, -pr.un[s].y};
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 ph = slice_point(smem, lay, pr, s, k, alpha[k]);
                    nx[0] += pr.wn[s][k] * ph.x;
                    nx[1] += pr.wn[s][k] * ph.y;
                }
                pr.q[s] = softmax2(nx[0], nx[1], pr.q[s], a.relax);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < PPT; ++s)
        if (tid + s * NT < N) reinterpret_cast<float2 *>(c.Q)[fo + tid + s * NT] = pr.q[s];

    // ---- the reverse sweep ------------------------------------------------------------------------------------------------------
    float *red = reinterpret_cast<float *>(smem + lay.total);             // [K][PPT][kWaves]
    float *tree = red + kMaxFusedK * kBackwardMaxPPT * kWaves;            // [K][kPartialRows]
    // the frame's partials per iteration and term (N > 0; the clamp: the plan sized the launch for frames of at most PPT x 1024 points)
    const int nblk = min((N + kPartialRows - 1) / kPartialRows, PPT * 4);
    const float2 *hq = hist + (size_t)T * hs;
    for (int t = T; t >= 1; --t) {
        opaque(pr);
        // (the lane index and the chain lane's words are made opaque per iteration: what the phases derive from them -- the ring's four
        // clamps, the pads' address -- is formed where it is used and not kept in registers around the sweep)
        asm volatile("" : "+v"(tid), "+v"(cl.a), "+v"(cl.b));
        const bool first = t == T;                                        // dL/dQ_t is the caller's; dL/dU, g_b and g_n are written
        hq -= hs;                                                         // Q_{t-1}
        // Phi_k(Q_{t-1})
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            pr.q[s] = make_float2(0.f, 0.f);
            if (tid + s * NT < N) pr.q[s] = hq[tid + s * NT];
        }
        splat_blur<PPT, K, CH, true, NT, ALL, true>(smem, lay, V, N, tid, pr, cl, ins);
        float2 xin[PPT][K];                                               // the transposed filters' inputs n_k * gamma
        // x_t, P_t, gamma_t, dL/dU, this lane's part of the weight gradient's dot products, g_n and the slice side of g_b
        float wsum[PPT][K];
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                wsum[s][k] = 0.0f;
                xin[s][k] = make_float2(0.f, 0.f);
            }
            const int i = tid + s * NT;
            if (i < N) {
                const FrameRows fr = frame_rows(f);
                const float2 u = fr.un[i], g = (first ? fr.gT : fr.G)[i];
                float2 ph[K], cv[K][D1];                                  // Phi_k, and the forward filter's values at the point's corners
                float nk[K];                                              // n_k[i], re-read: w_k * n_k is the prologue's product (PointRegs::wn),
                float x0 = -u.x, x1 = -u.y;                               //   formed again, which frees wn across the sweep
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) nk[k] = la->kd[k].norm[(size_t)f * la->kd[k].maxN + i];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    ph[k] = slice_signed_corners(smem, lay, pr, s, k, alpha[k], cv[k]);
                    const float wn = la->kd[k].w * nk[k];
                    x0 = x0 + wn * ph[k].x;
                    x1 = x1 + wn * ph[k].y;
                }
                const float2 gam = gamma2(x0, x1, g, la->relax);
                if (first) {
                    fr.gU[i] = make_float2(-gam.x, -gam.y);
                } else {
                    const float2 was = fr.gU[i];
                    fr.gU[i] = make_float2(was.x - gam.x, was.y - gam.y);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 r = make_float2(nk[k] * gam.x, nk[k] * gam.y);   // the transposed filter's input n_k * gamma, rounded once
                    wsum[s][k] += r.x * ph[k].x;
                    wsum[s][k] += r.y * ph[k].y;
                    xin[s][k] = r;
                    if (la->gF[k]) {                                      // (uniform)
                        const float v0 = gam.x * ph[k].x, v1 = gam.y * ph[k].y;
                        float sk = 0.0f;
                        sk += v0;
                        sk += v1;
                        float *gn = la->gn[k] + (size_t)f * la->kd[k].maxNpad + i;
                        const float was = first ? 0.0f : *gn;
                        *gn = was + la->kd[k].w * sk;
                        const float cs = la->kd[k].alpha * la->kd[k].w;
                        corner_dots2(la->gb[k] + (size_t)f * la->kd[k].Epad + (size_t)i * D1, first, cs, r, cv[k]);   // slice side
                    }
                }
            }
        }
        // k_softmax_bwd's butterfly over each wavefront of 64 consecutive points (every lane takes part)
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float v = wsum[s][k];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
                if ((tid & 63) == 0) red[(k * PPT + s) * kWaves + (tid >> 6)] = v;
            }
        }
        // Phi_k^T(n_k gamma_t)  (its first barrier stands between the wavefronts' sums and their readers)
        splat_blur<PPT, K, CH, true, NT, ALL, true, false, true, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
        // ... the four wavefronts of a 256-point block in order: the partial k_softmax_bwd's workgroup stores
        if (tid < K * PPT * 4) {
            const int k = tid / (PPT * 4), b = tid - k * (PPT * 4);
            if (b < nblk) {
                const float *r = red + (k * PPT + (b >> 2)) * kWaves + (b & 3) * 4;
                float sum = 0.0f;
                for (int w = 0; w < 4; ++w) sum += r[w];
                // partial[t][k][f][b]: the floats between two terms and this frame's row of a term, formed here for sixteen lanes' one store
                const LateArgs la = late();
                const int pterm = (int)gridDim.x * la->bstride, prow = f * la->bstride;
                la->partial[(size_t)((t - 1) * K + k) * pterm + prow + b] = sum;
            }
        }
        // G_{t-1} = (1 - r) G_t + sum_k w_k Phi_k^T(n_k gamma_t), and the splat side of g_b
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
            if (i < N) {
                const FrameRows fr = frame_rows(f);
                const float2 g = (first ? fr.gT : fr.G)[i];
                const LateArgs la = late();
                const float keep = 1.0f - la->relax;
                float acc0 = keep * g.x, acc1 = keep * g.y;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float2 cv[D1];                                        // the transposed filter's values at the point's corners
                    const float2 bt = slice_signed_corners(smem, lay, pr, s, k, alpha[k], cv);
                    acc0 = acc0 + la->kd[k].w * bt.x;
                    acc1 = acc1 + la->kd[k].w * bt.y;
                    if (la->gF[k]) {                                      // (uniform)
                        const float cs = la->kd[k].alpha * la->kd[k].w;
                        corner_dots2(la->gb[k] + (size_t)f * la->kd[k].Epad + (size_t)i * D1, false, cs, hq[i], cv);
                    }
                }
                fr.G[i] = make_float2(acc0, acc1);
            }
        }
    }

    // ---- dL/dU -= P_0 (G_0 - <G_0, P_0>), P_0 = Q_0 = softmax(-U) ---------------------------------------------------------------
    {
        const bool first = T == 0;
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
            if (i < N) {
                const FrameRows fr = frame_rows(f);
                const float2 u = fr.un[i];
                const float2 gam = gamma2(-u.x, -u.y, (first ? fr.gT : fr.G)[i], 1.0f);
                if (first) {
                    fr.gU[i] = make_float2(-gam.x, -gam.y);
                } else {
                    const float2 was = fr.gU[i];
                    fr.gU[i] = make_float2(was.x - gam.x, was.y - gam.y);
                }
            }
        }
    }

    // ---- the norm part of dL/db, <a_k, Phi_k(1)> with a_k = -n_k^2 g_n[k] at value width 1, and dL/db -> dL/df ----------------------
    int fmask = 0;                        // the terms with a feature array (uniform)
#pragma unroll
    for (int k = 0; k < K; ++k) fmask |= late()->gF[k] ? 1 << k : 0;
    if (fmask && T >= 1) {               // (a frame with t_f = 0 has no norm part: its gb / gn are not this launch's)
        opaque(pr);
        asm volatile("" : "+v"(tid));
        float2 xin[PPT][K];
        // the forward filter of all ones: the splat of ones is the barycentric weight itself (bary * 1.0f)
#pragma unroll
        for (int s = 0; s < PPT; ++s)
#pragma unroll
            for (int k = 0; k < K; ++k) xin[s][k] = make_float2(1.0f, 0.f);
        filter_terms<PPT, K, CH, false>(fmask, smem, lay, V, N, tid, pr, cl, ins, xin);
        // ... its corner dots with row a_i, scale alpha_k; a_i is the transposed filter's input
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
#pragma unroll
            for (int k = 0; k < K; ++k) xin[s][k] = make_float2(0.f, 0.f);
            if (i < N) {
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!la->gF[k]) continue;                             // (uniform)
                    const float n = la->kd[k].norm[(size_t)f * la->kd[k].maxN + i];
                    const float ai = -(n * n) * la->gn[k][(size_t)f * la->kd[k].maxNpad + i];   // k_norm_adjoint
                    float x[D1];
                    corner_values1(smem, lay, pr, s, k, x);
                    float *g = la->gb[k] + (size_t)f * la->kd[k].Epad + (size_t)i * D1;
#pragma unroll
                    for (int cc = 0; cc < D1; ++cc) {
                        float sj = 0.0f;
                        sj += ai * x[cc];
                        g[cc] = g[cc] + la->kd[k].alpha * sj;
                    }
                    xin[s][k] = make_float2(ai, 0.f);
                }
            }
        }
        opaque(pr);
        asm volatile("" : "+v"(tid));
        filter_terms<PPT, K, CH, true>(fmask, smem, lay, V, N, tid, pr, cl, ins, xin);
        // ... its corner dots with a row of ones, then dL/db -> dL/df through the point's simplex
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
            if (i < N) {
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!la->gF[k]) continue;                             // (uniform)
                    float x[D1], g[D1];
                    corner_values1(smem, lay, pr, s, k, x);
                    const float *gp = la->gb[k] + (size_t)f * la->kd[k].Epad + (size_t)i * D1;
#pragma unroll
                    for (int cc = 0; cc < D1; ++cc) {
                        float sj = 0.0f;
                        sj += 1.0f * x[cc];
                        g[cc] = gp[cc] + la->kd[k].alpha * sj;
                    }
                    const size_t row = ((size_t)f * la->kd[k].maxN + i) * 2;
                    const float feat[2] = {la->kd[k].feat[row], la->kd[k].feat[row + 1]};
                    const float scale[2] = {la->kd[k].scale[0], la->kd[k].scale[1]};
                    const float2 gf = corner_to_feature2(feat, scale, la->kd[k].inv_dp1, g);
                    la->gF[k][row] = gf.x;
                    la->gF[k][row + 1] = gf.y;
                }
            }
        }
    }

    // ---- dL/dw_k: k_bwd_reduce's walk over the frame's T x nblk partials and its tree ------------------------------------------------
    if (!a.gW) return;                    // (uniform)
    __syncthreads();                      // the partials of every iteration are written
    const int k = tid / kPartialRows, j = tid - k * kPartialRows;
    if (k < K) {
        const int pterm = (int)gridDim.x * a.bstride, prow = f * a.bstride;
        const float *row = a.partial + (size_t)k * pterm + prow;             // this frame's partials of term k, iteration 1
        const int n = T * nblk;
        float acc = 0.0f;
        for (int idx = j; idx < n; idx += kPartialRows) {
            const int t = idx / nblk, b = idx - t * nblk;
            acc += row[(size_t)t * K * pterm + b];
        }
        tree[k * kPartialRows + j] = acc;
    }
    __syncthreads();
    for (int m = kPartialRows / 2; m >= 1; m >>= 1) {
        if (k < K && j < m) tree[k * kPartialRows + j] += tree[k * kPartialRows + j + m];
        __syncthreads();
    }
    if (tid < K) a.gW[(size_t)f * K + tid] = tree[tid * kPartialRows];
}

}  // namespace

// The one-launch backward of request rq WITH feature gradients on area ar (Potts terms normalised AFTER, rq.T >= 1, no compat form):
// fused_report() of the shape launched, or 0 with nothing launched -- the frames are not ones the plan takes, and the caller runs the
// streaming sweep.  ar.gb / ar.gn need no zeroing: the kernel's first iteration writes them.  With rq.counts (section 2l) every frame's
// workgroup runs its own t_f iterations, the workgroups taking the frames by descending t_f (the order in ar.phi).
int launch_fused_backward_features(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows,
                                   const BackwardRequest &rq, const BackwardArea &ar, hipStream_t s)
{
    BackwardFeatureArgs a{};
    a.T = rq.T;
    a.rows = rows;
    a.bstride = std::max(backward_blocks(rows, c.L), 1);
    a.relax = rq.relax;
    a.slice = ar.slice;
    a.grad_prob = rq.grad_prob;
    a.hist = ar.hist;
    a.G = ar.G;
    a.gU = rq.grad_unary ? rq.grad_unary : ar.gU;
    a.gW = rq.grad_weights;
    a.partial = ar.partial;
    for (int k = 0; k < c.K && k < kMaxFusedK; ++k) {
        a.gF[k] = rq.grad_features ? rq.grad_features[k] : nullptr;
        a.gb[k] = ar.gb[k];
        a.gn[k] = ar.gn[k];
    }
    a.counts = rq.counts;
    return plan_variant<kBackwardMaxPPT>(c, kds, maxV, maxRow, kBackwardLds, a, [&](auto p, auto kk, auto ch) {
        // (section 2l) the longest frames first, as k_backward takes them (fused_backward.hip): the order lives in the area's `phi`, which
        // this kernel does not touch (K * slice floats: room for F ints)
        if (rq.counts && (size_t)c.K * ar.slice >= (size_t)c.F) {
            launch_order_by_count(rq.counts, c.F, rq.T, reinterpret_cast<int *>(ar.phi), s);
            a.order = reinterpret_cast<const int *>(ar.phi);
        }
        launch_workgroups(k_backward_features<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT,
                          a.lay.total + kBackwardLds, s, c, a);
    });
}

}  // namespace lccrf

// fused_backward.hip -- the gradients of mean-field inference (include/lccrf.h section 1c; a batch: section 2c) of a tracker-sized
// two-label frame in ONE launch: one 1024-lane workgroup per frame, the lattices' values in LDS, as the fused engine infers.
// Opt-in (LCCRF_OPT_FUSED_BACKWARD, include/lccrf.h section 1j); notes/fused_backward.md.
//
// Why: the streaming sweep (meanfield_backward.hip) is a launch per phase -- about 150 launches of a few microseconds each for two
// 2-D terms and T = 5 -- which a frame of 2000 keypoints cannot fill: the call is bound by launch gaps.
//
// What one launch does, per frame (blockIdx.x):
//     the fused engine's self-contained prologue (fused_prologue.inc) from the lattices in HBM, Q_0 = softmax(-U)
//     the replay: T x (splat, blur, slice, softmax) with fused_loop.h's phases, Q_0 .. Q_{T-1} kept in the area's `hist`, Q_T left in Q
//     for t = T .. 1:   Phi_k(Q_{t-1})                        splat_blur, forward axis order
//                       x_t, P_t, gamma_t, dL/dU, the partials of dL/dw_k        softmax_bwd<1, kBwdPlain>'s arithmetic at L = 2
//                       Phi_k^T(n_k gamma_t)                  splat_blur<.., GEN, TRANSPOSE>: the input n_k * gamma, rounded once
//                       G_{t-1} = (1 - r) G_t + sum_k w_k .   k_bwd_combine<false>'s arithmetic
//     the softmax backward of Q_0, and k_bwd_reduce's walk and tree over the frame's T x ceil(N / 256) partials
// With per-frame counts (section 2j) T above is the frame's own t_f, loaded once per workgroup: a frame that stopped early leaves its CU
// early, and the Q it leaves is Q_{t_f}.  Workgroup i then takes frame order[i], the frames sorted by descending t_f on the device
// (k_order_by_count, meanfield_backward.hip): which workgroup runs a frame changes no bit of it.
//
// Bit for bit the streaming sweep's results: every product and every sum is the one the streaming kernels form, in their order
// (-ffp-contract=off).  A row sum starts at +0 and adds the products in ascending point order (k_splat<false>); the slices start
// their sums at a literal 0.0f (slice_value: the inputs are signed here, and 0 + (-0) is +0); lane t owns points t and t + 1024, so
// a wavefront holds 64 consecutive points aligned to 64 -- the wavefronts k_softmax_bwd's butterfly runs over -- and four consecutive
// wavefronts of a point slot are one of its 256-point workgroups.  The cross-lane steps run with every lane, outside the per-point
// regions; lanes without a point contribute +0.
//
// On chip across the sweep: the vertex ids, product slots, barycentric weights and w * n_k of a lane's points (PointRegs).  Re-read
// per iteration by the lane that owns the point (L2-resident: 128 KB per frame): Q_{t-1}, the unaries, n_k, G and dL/dU.  Memory: section 1c's area, of which `phi` is not touched.
//
// Scope: Potts terms normalised AFTER, K in {1, 2} 2-D terms, frames of up to 2 x 1024 active points, kernel 0 with short rows or
// chain rows: 8 instantiations.  Not covered: matrices and normalisation modes, feature gradients, the sums over the frames
// (grad_model), larger frames, the half-CU shapes.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"
#include "fused_backward_common.h"

namespace lccrf {

namespace {

using namespace fl;

struct BackwardArgs {
    KernelDev kd[kMaxFusedK];
    FusedLayout lay;
    int T, rows;                          // rows: points per frame of gU (rows [n_points[f], rows) are written 0)
    int bstride;                          // partials per (iteration, term, frame): the area's row
    float relax;
    size_t slice;                         // floats between the iterations of hist
    const float *grad_prob;               // [F][maxN][2] dL/dQ_T
    float *hist;                          // [T][slice]
    float *G;                             // [F][maxN][2]
    float *gU;                            // [F][maxN][2]
    float *gW;                            // [F][K] or null
    float *partial;                       // [T][K][F][bstride]
    const int *counts;                    // [F] or null (section 2j): frame f runs min(max(counts[f], 0), T) iterations, T the layout's
    const int *order;                     // [F] or null: workgroup i takes frame order[i] (a permutation: the longest counts first)
};

// (gamma2 and slice_signed, the sweep's row arithmetic: fused_backward_common.h, shared with k_backward_general)

#define FUSED_PROLOGUE_TERMS \
    gt.has_pre = (1 << K) - 1; \
    gt.has_mu = 0;
template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_backward(CrfDev c, BackwardArgs a)
{
    constexpr int D1 = kD1, NT = kNT, ALL = (1 << K) - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = a.order ? a.order[blockIdx.x] : blockIdx.x;
    int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};
    const size_t fo = (size_t)f * c.maxN;                 // the frame's first row of every [F][maxN][2] array
    float2 *gU = reinterpret_cast<float2 *>(a.gU) + fo;

    for (int i = max(N, 0) + tid; i < a.rows; i += NT) gU[i] = make_float2(0.f, 0.f);   // rows beyond the frame's points: dL/dU = 0
    if (N <= 0) {                         // nothing to differentiate (and nothing below may index an empty frame)
        if (a.gW && tid < K) a.gW[(size_t)f * K + tid] = 0.0f;
        return;
    }

    // the frame's own iteration count (section 2j): one uniform load per workgroup, so every barrier below stays uniform; hist and
    // partial keep their [a.T][...] layout
    const int T = a.counts ? min(max(a.counts[f], 0), a.T) : a.T;

    PointRegs<PPT, K> pr;
    GeneralTerms<PPT, K> gt;
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
    const float2 *un = reinterpret_cast<const float2 *>(c.unary) + fo;
    const float2 *gT = reinterpret_cast<const float2 *>(a.grad_prob) + fo;
    float2 *G = reinterpret_cast<float2 *>(a.G) + fo;
    float *red = reinterpret_cast<float *>(smem + lay.total);             // [K][PPT][kWaves]
    float *tree = red + kMaxFusedK * kBackwardMaxPPT * kWaves;            // [K][kPartialRows]
    // the frame's partials per iteration and term (N > 0; the clamp: the plan sized the launch for frames of at most PPT x 1024 points)
    const int nblk = min((N + kPartialRows - 1) / kPartialRows, PPT * 4);
    // partial[t][k][f][b]: the floats between two terms, and where this frame's row of a term begins -- kept in vector registers on
    // purpose: as uniform values they are live around the whole sweep for sixteen lanes' one store per iteration, and the two-term
    // chain kernel has no scalar register left for them
    int pterm = (int)gridDim.x * a.bstride, prow = f * a.bstride;
    asm volatile("" : "+v"(pterm), "+v"(prow));
    const float2 *hq = hist + (size_t)T * hs;
    for (int t = T; t >= 1; --t) {
        opaque(pr);
        asm volatile("" : "+v"(tid));
        const bool first = t == T;                                        // dL/dQ_t is the caller's, dL/dU is written
        hq -= hs;                                                         // Q_{t-1}
        // Phi_k(Q_{t-1})
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            pr.q[s] = make_float2(0.f, 0.f);
            if (tid + s * NT < N) pr.q[s] = hq[tid + s * NT];
        }
        splat_blur<PPT, K, CH, true, NT, ALL, true>(smem, lay, V, N, tid, pr, cl, ins);
        // x_t, P_t, gamma_t, dL/dU and this lane's part of the weight gradient's dot products
        float wsum[PPT][K];
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
#pragma unroll
            for (int k = 0; k < K; ++k) wsum[s][k] = 0.0f;
            pr.q[s] = make_float2(0.f, 0.f);
#pragma unroll
            for (int k = 0; k < K; ++k) gt.pre[s][k] = 0.0f;
            const int i = tid + s * NT;
            if (i < N) {
                const float2 u = un[i], g = (first ? gT : G)[i];
                float2 ph[K];
                float x0 = -u.x, x1 = -u.y;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    ph[k] = slice_signed(smem, lay, pr, s, k, alpha[k]);
                    x0 = x0 + pr.wn[s][k] * ph[k].x;
                    x1 = x1 + pr.wn[s][k] * ph[k].y;
                }
                const float2 gam = gamma2(x0, x1, g, a.relax);
                if (first) {
                    gU[i] = make_float2(-gam.x, -gam.y);
                } else {
                    const float2 was = gU[i];
                    gU[i] = make_float2(was.x - gam.x, was.y - gam.y);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    gt.pre[s][k] = a.kd[k].norm[(size_t)f * a.kd[k].maxN + i];   // n_k: the transposed filter's input is n_k * gamma
                    wsum[s][k] += (gt.pre[s][k] * gam.x) * ph[k].x;
                    wsum[s][k] += (gt.pre[s][k] * gam.y) * ph[k].y;
                }
                pr.q[s] = gam;                                            // the transposed filter's input: n_k * gamma (filter_input)
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
        splat_blur<PPT, K, CH, true, NT, ALL, true, true, true>(smem, lay, V, N, tid, pr, cl, ins, &gt);
        // ... the four wavefronts of a 256-point block in order: the partial k_softmax_bwd's workgroup stores
        if (tid < K * PPT * 4) {
            const int k = tid / (PPT * 4), b = tid - k * (PPT * 4);
            if (b < nblk) {
                const float *r = red + (k * PPT + (b >> 2)) * kWaves + (b & 3) * 4;
                float sum = 0.0f;
                for (int w = 0; w < 4; ++w) sum += r[w];
                a.partial[(size_t)((t - 1) * K + k) * pterm + prow + b] = sum;
            }
        }
        // G_{t-1} = (1 - r) G_t + sum_k w_k Phi_k^T(n_k gamma_t)
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
            if (i < N) {
                const float2 g = (first ? gT : G)[i];
                const float keep = 1.0f - a.relax;
                float acc0 = keep * g.x, acc1 = keep * g.y;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 bt = slice_signed(smem, lay, pr, s, k, alpha[k]);
                    acc0 = acc0 + a.kd[k].w * bt.x;
                    acc1 = acc1 + a.kd[k].w * bt.y;
                }
                G[i] = make_float2(acc0, acc1);
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
                const float2 u = un[i];
                const float2 gam = gamma2(-u.x, -u.y, (first ? gT : G)[i], 1.0f);
                if (first) {
                    gU[i] = make_float2(-gam.x, -gam.y);
                } else {
                    const float2 was = gU[i];
                    gU[i] = make_float2(was.x - gam.x, was.y - gam.y);
                }
            }
        }
    }

    // ---- dL/dw_k: k_bwd_reduce's walk over the frame's T x nblk partials and its tree ------------------------------------------------
    if (!a.gW) return;                    // (uniform)
    __syncthreads();                      // the partials of every iteration are written
    const int k = tid / kPartialRows, j = tid - k * kPartialRows;
    if (k < K) {
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

// The one-launch backward of request rq (dL/dU and / or dL/dw only) on area ar: fused_report() of the shape launched, or 0 with nothing
// launched -- the frames are not ones the plan takes, and the caller runs the streaming sweep.
int launch_fused_backward(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows, const BackwardRequest &rq,
                          const BackwardArea &ar, hipStream_t s)
{
    BackwardArgs a{};
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
    a.counts = rq.counts;
    return plan_variant<kBackwardMaxPPT>(c, kds, maxV, maxRow, kBackwardLds, a, [&](auto p, auto kk, auto ch) {
        // (section 2j) workgroups start in index order as CUs fall free: with the longest frames first the last CU to finish holds a short
        // one.  The order lives in the area's `phi`, which this kernel does not touch (K * slice floats: room for F ints).
        if (rq.counts && (size_t)c.K * ar.slice >= (size_t)c.F) {
            launch_order_by_count(rq.counts, c.F, rq.T, reinterpret_cast<int *>(ar.phi), s);
            a.order = reinterpret_cast<const int *>(ar.phi);
        }
        launch_workgroups(k_backward<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT, a.lay.total + kBackwardLds, s, c,
                          a);
    });
}

}  // namespace lccrf

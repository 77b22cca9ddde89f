// fused_backward_general.hip -- the gradients of mean-field inference under a LEARNT two-label model (include/lccrf.h sections 1e, 1g
// and 2h: terms with a label-compatibility matrix or a normalisation mode, and dL/dmu also of Potts terms) of a tracker-sized frame in
// ONE launch: one 1024-lane workgroup per frame, the lattices' values in LDS.  Opt-in (LCCRF_OPT_FUSED_BACKWARD_LEARNT, include/lccrf.h
// section 1k); notes/fused_backward.md section 6.  k_backward (fused_backward.hip) keeps the Potts / AFTER requests and the code it has.
//
// What one launch does, per frame (blockIdx.x):
//     the fused engine's self-contained prologue (fused_prologue.inc), Q_0 = softmax(-U)
//     the replay: T x (splat of b_k . Q, blur, slice, mu_k, softmax) as mean_field<.., GEN> forms Q_t -- Q_0 .. Q_{T-1} to `hist`, Q_T to Q
//     for t = T .. 1:   Phi_k(b_k . Q_{t-1})                  splat_blur, forward axis order, the input through the term's pre factor
//                       ph_k = mu_k Phi_k (Phi_k itself for a Potts term), x_t, gamma_t, dL/dU, the partials of dL/dw_k
//                                                              softmax_bwd<1, kBwdCompat / kBwdPlain>'s arithmetic at L = 2
//                       y_k = a_k gamma_t, and y_k (x) Phi_k staged for dL/dmu_k                          k_compat_bwd's products
//                       the chunks' ordered sums of the staged products, cp = (first ? . : cp +) w_k acc  k_compat_bwd's chains
//                       Phi_k^T(mu_k^T y_k)  (y_k for a Potts term)   splat_blur<.., TRANSPOSE, XIN>: an input per term
//                       G_{t-1} = (1 - r) G_t + sum_k w_k (b_k .) Phi_k^T(..)                              k_bwd_combine<PRE>'s arithmetic
//     the softmax backward of Q_0, k_bwd_reduce's walk and tree, and dL/dmu_k = the chunks' cp added in ascending order (k_compat_reduce)
// With per-frame counts (section 2k) T above is the frame's own t_f, loaded once per workgroup -- a frame that stopped early leaves its CU
// early, the Q it leaves is Q_{t_f}, and at t_f = 0 the chains' cp stay the zeros they start as -- and workgroup i takes frame
// order[i], the frames sorted by descending t_f on the device (k_order_by_count, meanfield_backward.hip), as k_backward does: which
// workgroup runs a frame changes no bit of it.  The counts and the order are runtime arguments, read once at the kernel's entry and dead
// behind it (t_f takes a.T's scalar register): no instantiation more, the register figures of the kernel without them.
//
// Bit for bit the streaming sweep's results (-ffp-contract=off): every product and every sum is the one the streaming kernels form, in
// their order.  a_k is what step_kdevs()[k].norm points at (n, sqrtf(n) or ones), b_k is pre_arg()[k] or absent; both are re-read per
// iteration from L2 by the lane that owns the point, like Q_{t-1}, U, G and dL/dU.
//
// dL/dmu.  A frame of N points has B = compat_chunks(N) <= 8 chunks of ceil(N / B) consecutive rows, and per iteration, term, chunk and
// entry (l, l') one chain acc = 0.0f; acc += y_i[l] * Phi_i[l'] over the chunk's rows in ascending order.  The products are formed by
// the lanes that own the points (contraction is off: a product is the same bits wherever it is formed) and staged as one float4 per
// point in the term's own product buffer -- free between the forward filter's row sums and the transposed filter's products, and never
// smaller than 16 bytes per point -- so the route needs no LDS beyond k_backward's.  Wavefront 0 owns the K * B * 4 <= 64 chains, lane
// (k * 8 + b) * 4 + e, eight loads ahead of the adds, a lane past the end of its chunk reading the zero block (x + (+0) is exact: a sum
// that started at +0 never holds -0); cp lives in that lane's word of LDS across the sweep.  This needs every term to own its product
// buffer (FusedLayout::prod_all): frames whose lattices leave the plan one shared buffer stream.
//
// Every barrier is met by every lane: the N <= 0 exit is the whole workgroup's and comes first, the cross-lane steps and the chain
// phase run outside the per-point predicates, and what decides a barrier (a.gC, a.gW) is uniform.
//
// Scope: K in {1, 2} 2-D terms, frames of up to 2 x 1024 active points, kernel 0 with short rows or chain rows: 8 instantiations.
// Not covered: feature gradients (at a fixed count or at per-frame counts), larger frames, the half-CU shapes.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"
#include "fused_backward_common.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kMuChunks = 8;              // compat_chunks(2048): the chunks of the largest frame the plan takes

struct BackwardGeneralArgs {
    KernelDev kd[kMaxFusedK];             // Engine::step_kdevs(): `norm` is a_k, the factor behind the filter
    const float *pre[kMaxFusedK];         // Engine::pre_arg()[k]: [F][maxN] b_k, the factor in front of term k's filter, or null
    float mu[kMaxFusedK][4];              // term k's matrix, row-major, by value: uniform in the kernel
    int has_mu;                           // bit k: term k has a matrix
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
    float *gC;                            // [F][K][2][2] or null
    float *partial;                       // [T][K][F][bstride]
    const int *counts;                    // [F] or null (section 2k): frame f runs min(max(counts[f], 0), T) iterations, T the layout's
    const int *order;                     // [F] or null: workgroup i takes frame order[i] (a permutation: the longest counts first)
};

// The kernel's arguments as the kernarg segment holds them, read where they are used: the 8 matrix words, the factors' pointers and the
// other uniform values of the learnt model, kept in scalar registers from the kernel's entry on, are live around the whole sweep, and
// the two-term kernels have no scalar register left for them (k_backward<2, 2, 1> is short of them as it is).  late() hands out the
// arguments behind an opaque scalar pointer, so that each use is a scalar load of its own next to the use.
struct KernArgs { CrfDev c; BackwardGeneralArgs a; };   // two by-value parameters, each at its natural alignment
typedef const __attribute__((address_space(4))) BackwardGeneralArgs *LateArgs;
__device__ __forceinline__ LateArgs late()
{
    const __attribute__((address_space(4))) unsigned char *p =
        (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (LateArgs)(p + offsetof(KernArgs, a));
}

// the input of term k's filter at point i of frame f: q, or b_k[i] * q rounded once (filter_input; k_splat<true>)
__device__ __forceinline__ float2 term_input(LateArgs a, int f, int i, int k, const float2 q)
{
    if (a->pre[k]) {                      // (uniform)
        const float b = a->pre[k][(size_t)f * a->kd[k].maxN + i];
        return make_float2(b * q.x, b * q.y);
    }
    return q;
}

// mu_k t behind a slice (k_slice_compat; softmax_bwd<1, kBwdCompat>): s_l = 0; s_l = s_l + mu[l][0] * t[0]; s_l = s_l + mu[l][1] * t[1]
typedef const __attribute__((address_space(4))) float *MuWords;
__device__ __forceinline__ float2 mu_times(MuWords m, const float2 t)
{
    float s0 = 0.0f, s1 = 0.0f;
    s0 = s0 + m[0] * t.x;
    s0 = s0 + m[1] * t.y;
    s1 = s1 + m[2] * t.x;
    s1 = s1 + m[3] * t.y;
    return make_float2(s0, s1);
}

// mu_k^T y (k_compat_bwd): o_l' = 0; o_l' = o_l' + mu[0][l'] * y[0]; o_l' = o_l' + mu[1][l'] * y[1]
__device__ __forceinline__ float2 mu_transposed_times(MuWords m, const float2 y)
{
    float o0 = 0.0f, o1 = 0.0f;
    o0 = o0 + m[0] * y.x;
    o0 = o0 + m[2] * y.y;
    o1 = o1 + m[1] * y.x;
    o1 = o1 + m[3] * y.y;
    return make_float2(o0, o1);
}

template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_backward_general(CrfDev c, BackwardGeneralArgs a)
{
    constexpr int D1 = kD1, NT = kNT, ALL = (1 << K) - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (section 2k) the frame of this workgroup and, below, its own iteration count: uniform values
    const int f = a.order ? a.order[blockIdx.x] : blockIdx.x;
    int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};
    const size_t fo = (size_t)f * c.maxN;                 // the frame's first row of every [F][maxN][2] array
    float2 *gU = reinterpret_cast<float2 *>(a.gU) + fo;

    for (int i = max(N, 0) + tid; i < a.rows; i += NT) gU[i] = make_float2(0.f, 0.f);   // rows beyond the frame's points: dL/dU = 0
    if (N <= 0) {                         // nothing to differentiate (and nothing below may index an empty frame)
        if (a.gW && tid < K) a.gW[(size_t)f * K + tid] = 0.0f;
        if (a.gC && tid < K * 4) a.gC[(size_t)f * K * 4 + tid] = 0.0f;
        return;
    }

    // the frame's own iteration count: one uniform load per workgroup, so every barrier below stays uniform; hist and partial keep
    // their [a.T][...] layout
    const int T = a.counts ? min(max(a.counts[f], 0), a.T) : a.T;

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

    // ---- the replay: inference(T, 0, relax) under the model, keeping Q_0 .. Q_{T-1} --------------------------------------------------
    const size_t hs = a.slice / 2;        // float2 between the iterations of hist
    float2 *hist = reinterpret_cast<float2 *>(a.hist) + fo;
    for (int t = 0; t < T; ++t) {
        opaque(pr);
        asm volatile("" : "+v"(tid));
        float2 xin[PPT][K];
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
#pragma unroll
            for (int k = 0; k < K; ++k) xin[s][k] = pr.q[s];
            if (i < N) {
                hist[(size_t)t * hs + i] = pr.q[s];
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) xin[s][k] = term_input(la, f, i, k, pr.q[s]);
            }
        }
        splat_blur<PPT, K, CH, true, NT, ALL, true, false, false, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            if (tid + s * NT < N) {
                float nx[2] = {-pr.un[s].x, -pr.un[s].y};
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float2 ph = slice_point(smem, lay, pr, s, k, alpha[k]);
                    if ((la->has_mu >> k) & 1) ph = mu_times(la->mu[k], ph);
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
    float *tree = red + kMaxFusedK * kBackwardMaxPPT * kWaves;            // [K][kPartialRows]; during the sweep its head holds the chains' cp [K][8][4]
    // the frame's partials per iteration and term (N > 0; the clamp: the plan sized the launch for frames of at most PPT x 1024 points)
    const int nblk = min((N + kPartialRows - 1) / kPartialRows, PPT * 4);
    // wavefront 0: this lane's chain, accumulated over the sweep in the lane's own word of `tree` (unused until the reduction)
    if (tid < kMaxFusedK * kMuChunks * 4) tree[tid] = 0.0f;
    // partial[t][k][f][b]: the floats between two terms, and where this frame's row of a term begins -- in vector registers on purpose
    // (fused_backward.hip: as uniform values they are live around the whole sweep for sixteen lanes' one store per iteration)
    int pterm = (int)gridDim.x * a.bstride, prow = f * a.bstride;
    asm volatile("" : "+v"(pterm), "+v"(prow));
    const float2 *hq = hist + (size_t)T * hs;
    for (int t = T; t >= 1; --t) {
        opaque(pr);
        asm volatile("" : "+v"(tid));
        const bool first = t == T;                                        // dL/dQ_t is the caller's, dL/dU is written
        hq -= hs;                                                         // Q_{t-1}
        float2 xin[PPT][K];
        // Phi_k(b_k . Q_{t-1})
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
#pragma unroll
            for (int k = 0; k < K; ++k) xin[s][k] = make_float2(0.f, 0.f);
            if (i < N) {
                const float2 q = hq[i];
                const LateArgs la = late();
#pragma unroll
                for (int k = 0; k < K; ++k) xin[s][k] = term_input(la, f, i, k, q);
            }
        }
        splat_blur<PPT, K, CH, true, NT, ALL, true, false, false, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
        // x_t, gamma_t, dL/dU, this lane's part of the weight gradient's dot products, the staged products of dL/dmu and the inputs of
        // the transposed filters
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
                const float2 u = un[i], g = (first ? gT : G)[i];
                const LateArgs la = late();
                float2 ph[K], mph[K];                                     // Phi_k, and mu_k Phi_k (Phi_k itself for a Potts term)
                float ak[K];                                              // a_k[i], re-read: w_k * a_k is the prologue's product (PointRegs::wn)
                float x0 = -u.x, x1 = -u.y;
#pragma unroll
                for (int k = 0; k < K; ++k) ak[k] = la->kd[k].norm[(size_t)f * la->kd[k].maxN + i];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    ph[k] = slice_signed(smem, lay, pr, s, k, alpha[k]);
                    mph[k] = ph[k];
                    if ((la->has_mu >> k) & 1) mph[k] = mu_times(la->mu[k], ph[k]);
                    const float wn = la->kd[k].w * ak[k];
                    x0 = x0 + wn * mph[k].x;
                    x1 = x1 + wn * mph[k].y;
                }
                const float2 gam = gamma2(x0, x1, g, la->relax);
                if (first) {
                    gU[i] = make_float2(-gam.x, -gam.y);
                } else {
                    const float2 was = gU[i];
                    gU[i] = make_float2(was.x - gam.x, was.y - gam.y);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 y = make_float2(ak[k] * gam.x, ak[k] * gam.y);   // y_k = a_k * gamma, rounded once
                    wsum[s][k] += y.x * mph[k].x;
                    wsum[s][k] += y.y * mph[k].y;
                    // y_k (x) Phi_k, entries (0,0) (0,1) (1,0) (1,1): one float4 per point in the term's product buffer (its rows are summed,
                    // the transposed filter's products come behind the chain phase); the guard keeps a frame the plan did not size in bounds
                    if (la->gC && i < (la->lay.Ecap[k] >> 1))
                        reinterpret_cast<float4 *>(smem + la->lay.prod[k])[i] = make_float4(y.x * ph[k].x, y.x * ph[k].y, y.y * ph[k].x, y.y * ph[k].y);
                    xin[s][k] = ((la->has_mu >> k) & 1) ? mu_transposed_times(la->mu[k], y) : y;
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
        __syncthreads();                  // the wavefronts' sums and the staged products are written
        // ... the four wavefronts of a 256-point block in order: the partial k_softmax_bwd's workgroup stores
        if (tid < K * PPT * 4) {
            const int k = tid / (PPT * 4), b = tid - k * (PPT * 4);
            if (b < nblk) {
                const float *r = red + (k * PPT + (b >> 2)) * kWaves + (b & 3) * 4;
                float sum = 0.0f;
                for (int w = 0; w < 4; ++w) sum += r[w];
                late()->partial[(size_t)((t - 1) * K + k) * pterm + prow + b] = sum;
            }
        }
        // the chains of dL/dmu: lane (k * 8 + b) * 4 + e of wavefront 0 adds entry e of chunk b's rows of term k in ascending order
        if (late()->gC) {                 // (uniform)
            if (tid < kMaxFusedK * kMuChunks * 4) {
                const LateArgs la = late();
                // the chunks of dL/dmu (k_compat_bwd's: compat_chunks(N) of ceil(N / B) rows), clamped like nblk; formed here, not kept
                const int nchunk = min(compat_chunks(N), kMuChunks), chunk = (N + nchunk - 1) / nchunk;
                const int k = tid >> 5, b = (tid >> 2) & (kMuChunks - 1), e = tid & 3;
                if (k < K && b < nchunk) {
                    const float *st = reinterpret_cast<const float *>(smem + (k == 0 ? la->lay.prod[0] : la->lay.prod[K - 1])) + e;
                    const float *zero = reinterpret_cast<const float *>(smem + la->lay.zero);
                    const int cap = min(N, (k == 0 ? la->lay.Ecap[0] : la->lay.Ecap[K - 1]) >> 1);
                    const int i0 = min(b * chunk, cap), i1 = min(i0 + chunk, cap);
                    float acc = 0.0f;
                    for (int p = i0; p < i1; p += 8) {
                        float x[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) x[u] = *((p + u < i1) ? st + 4 * (p + u) : zero);
#pragma unroll
                        for (int u = 0; u < 8; ++u) acc += x[u];          // strictly in row order
                    }
                    const float wk = k == 0 ? la->kd[0].w : la->kd[K - 1].w;
                    tree[tid] = first ? wk * acc : tree[tid] + wk * acc;
                }
            }
            __syncthreads();              // the staged products are read: the product buffers are the transposed filter's again
        }
        // Phi_k^T(mu_k^T y_k)
        splat_blur<PPT, K, CH, true, NT, ALL, true, false, true, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
        // G_{t-1} = (1 - r) G_t + sum_k w_k (b_k .) Phi_k^T(..)
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int i = tid + s * NT;
            if (i < N) {
                const float2 g = (first ? gT : G)[i];
                const LateArgs la = late();
                const float keep = 1.0f - la->relax;
                float acc0 = keep * g.x, acc1 = keep * g.y;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 bt = term_input(la, f, i, k, slice_signed(smem, lay, pr, s, k, alpha[k]));
                    acc0 = acc0 + la->kd[k].w * bt.x;
                    acc1 = acc1 + la->kd[k].w * bt.y;
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

    // ---- dL/dmu_k: the chunks' partials in ascending order (k_compat_reduce) -----------------------------------------------------------
    if (late()->gC) {                     // (uniform)
        __syncthreads();
        if (tid < K * 4) {
            const int k = tid >> 2, e = tid & 3, nchunk = min(compat_chunks(N), kMuChunks);
            float out = 0.0f;
            for (int b = 0; b < nchunk; ++b) out += tree[(k * kMuChunks + b) * 4 + e];
            late()->gC[((size_t)f * K + k) * 4 + e] = out;
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

// The one-launch backward of request rq (no feature gradients) on area ar under the model `terms`: fused_report() of the shape launched,
// or 0 with nothing launched -- the frames are not ones the plan takes, or (dL/dmu asked for) its terms share one product buffer -- and
// the caller runs the streaming sweep.
int launch_fused_backward_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows,
                                  const BackwardRequest &rq, const BackwardArea &ar, const TermModel &terms, hipStream_t s)
{
    BackwardGeneralArgs a{};
    a.T = rq.T;
    a.rows = rows;
    a.bstride = std::max(backward_blocks(rows, c.L), 1);
    a.relax = rq.relax;
    a.slice = ar.slice;
    a.grad_prob = rq.grad_prob;
    a.hist = ar.hist;
    a.G = ar.G;
    a.gU = rq.grad_unary ? rq.grad_unary : ar.gU;
    a.gW = rq.grad_weights ? rq.grad_weights : ar.gW;
    a.gC = rq.grad_compat ? rq.grad_compat : ar.gC;
    a.partial = ar.partial;
    a.counts = rq.counts;
    bool launched = false;
    const int report = plan_variant<kBackwardMaxPPT>(c, kds, maxV, maxRow, kBackwardLds, a, [&](auto p, auto kk, auto ch) {
        if (a.gC && !a.lay.prod_all) return;              // (the staged products of dL/dmu live in the terms' own product buffers)
        for (int k = 0; k < c.K; ++k) a.pre[k] = terms.pre ? terms.pre[k] : nullptr;
        a.has_mu = copy_matrices(terms, c.K, a.mu);
        // (section 2k) the longest frames first, as k_backward takes them (fused_backward.hip): the order lives in the area's `phi`, which
        // this kernel does not touch (K * slice floats: room for F ints)
        if (rq.counts && (size_t)c.K * ar.slice >= (size_t)c.F) {
            launch_order_by_count(rq.counts, c.F, rq.T, reinterpret_cast<int *>(ar.phi), s);
            a.order = reinterpret_cast<const int *>(ar.phi);
        }
        launch_workgroups(k_backward_general<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT,
                          a.lay.total + kBackwardLds, s, c, a);
        launched = true;
    });
    return launched ? report : 0;
}

}  // namespace lccrf

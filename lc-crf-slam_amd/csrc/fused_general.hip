// fused_general.hip -- the fused engine's inference (fused_engine.hip: one launch, one 1024-lane workgroup per frame, the mean-field
// state on chip) for the two-label handle or batch whose terms are not all Potts terms normalised AFTER the filter: per term an optional 2 x 2
// label-compatibility matrix (include/lccrf.h section 1e), a per-point factor in front of the filter and one behind it (section 1g).
//
// Why: such a handle (and such a batch, include/lccrf.h section 2g) used to leave the one-workgroup engines for the streaming engine's general L-label step -- one splat, d + 1
// blur passes and one slice per term plus a softmax, 11 launches per iteration for the tracker's two 2-D terms, 57 for
// inference(5, true) -- where a launch-per-phase design is bound by launch gaps.  notes/fused_general.md.
//
// The loop is fused_loop.h's, in its GEN form: ordered row sums, chain rows, blur, softmax2, relax blending, store_results and the
// label bits are the fused engine's code.  The arithmetic is what the streaming kernels do (k_splat<true>, k_slice_compat), every
// product and every sum rounded on its own (-ffp-contract=off):
//     x    = pre[i] * Q[i][l], rounded once, then bary * x          (Q itself without a pre)
//     s_l  = 0; s_l = s_l + mu[l][0] * t[0]; s_l = s_l + mu[l][1] * t[1]   behind the slice t of a term with a matrix
//     next_l += wn * s_l,  wn = w * post[i]                           (post: n, sqrtf(n), or 1.0f for BEFORE / NONE)
//
// Scope: frames of up to 2 x 1024 active points -- a handle's one, or every frame of a batch, indexed by blockIdx.x -- K in {1, 2} 2-D
// terms, kernel 0 with short rows or chain rows, the self-contained prologue only (fused_prologue.inc: the one text k_fused includes too;
// prepared launch records belong to the batches' Potts path and are neither read nor written here): 8 instantiations, kept in a unit of
// their own so that a change to this kernel leaves the fused engine's kernels the code they are.  Run until converged:
// fused_general_converge.hip.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kGeneralMaxPPT = 2;         // points per lane: the loop keeps PPT * K pre factors in registers beside w * post

struct GeneralArgs {
    KernelDev kd[kMaxFusedK];             // Engine::step_kdevs(): `norm` is the factor behind the filter
    const float *pre[kMaxFusedK];         // Engine::pre_arg()[k]: [F][maxN] factor in front of term k's filter, or null
    float mu[kMaxFusedK][4];              // term k's matrix, row-major, by value: uniform in the kernel
    int has_mu;                           // bit k: term k has a matrix
    FusedLayout lay;
    int n_iter, with_map;
    float relax;
};

// k_fused<1024, PPT, K, CH, 0> (fused_engine.hip) with the terms of GeneralTerms: the same self-contained prologue
// (fused_prologue.inc) plus GeneralTerms' uniform members behind the table loads and the pre factors beside the norms.
#define FUSED_PROLOGUE_TERMS                                            \
    gt.has_pre = 0;                                                     \
    gt.has_mu = a.has_mu;                                               \
    _Pragma("unroll") for (int k = 0; k < K; ++k) {                     \
        if (a.pre[k]) gt.has_pre |= 1 << k;                             \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) gt.mu[k][e] = a.mu[k][e]; \
    }
#define FUSED_PROLOGUE_POINT gt.pre[s][k] = a.pre[k] ? a.pre[k][(size_t)f * kd.maxN + ic] : 1.0f;
template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_general(CrfDev c, GeneralArgs a)
{
    constexpr int D1 = kD1, NT = kNT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};

    PointRegs<PPT, K> pr;
    GeneralTerms<PPT, K> gt;
    int V[K];
#pragma unroll
    for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    const FusedLayout &lay = a.lay;

    if (N <= 0) {                         // nothing to infer (and nothing below may index an empty frame)
        if (a.with_map) clear_label_bits<NT>(c, f, 0, tid);
        return;
    }

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
    mean_field<PPT, K, CH, NT, true, true>(smem, lay, V, N, tid, pr, cl, alpha, a.n_iter, a.relax, ins, -1, &gt);

    store_results<PPT, K, NT>(c, f, N, tid, pr, a.with_map);
}

}  // namespace

// kds: Engine::step_kdevs() -- `norm` is each term's factor behind the filter.  Frames beyond 2048 active points: 0.
int launch_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s)
{
    GeneralArgs a{};
    a.n_iter = rq.run.n_iter;
    a.with_map = rq.run.with_map;
    a.relax = rq.run.relax;
    return plan_variant<kGeneralMaxPPT>(c, kds, maxV, maxRow, 0, a, [&](auto p, auto kk, auto ch) {
        fill_general_terms(a, c, rq.terms);
        launch_workgroups(k_general<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT, a.lay.total, s, c, a);
    });
}

}  // namespace lccrf

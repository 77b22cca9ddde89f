// fused_multilabel_general.hip -- k_multilabel (fused_multilabel.hip: frames of THREE TO EIGHT labels in one launch, one 1024-lane
// workgroup per frame) for the frame whose terms are not all Potts terms normalised AFTER the filter: per term an optional L x L
// label-compatibility matrix (include/lccrf.h sections 1e and 2g), a per-point factor in front of the filter and one behind it
// (section 1g).  Opt-in: LCCRF_MULTILABEL_LEARNT (lccrf_set_multilabel_routes); the engine report is 6.  notes/fused_multilabel.md
// section 6.
//
// Why: a matrix is what the project learns, and at three to eight labels it carries most of the model; such a frame ran on the
// streaming engine, 11 launches per iteration for the tracker's two 2-D terms, 57 for inference(5, true).
//
// The arithmetic is the streaming engine's general L-label step (k_splat<true>, k_slice_compat in stream_filter.hip; restated for
// L = 2 in the header of fused_general.hip), every product and every sum rounded on its own (-ffp-contract=off):
//     x    = pre_k[i] * Q[i][l], rounded once, then bary * x                (Q itself for a term without a pre: AFTER, NONE)
//     s_l  = 0; s_l = s_l + mu_k[l][l'] * t_k[l'], l' = 0 .. L-1 ascending  behind the slice t_k of a term with a matrix
//     next_l = -U_l; next_l += wn_k * s_l (or wn_k * t_k[l]), k ascending;  wn_k = w_k * post_k[i]   (post: Engine::step_kdevs()'s norm)
// then exp_and_normalize_reg<L> with the relax blend and argmax_row, as in k_multilabel.  The sum s_l starts at literal 0:
// 0 + (-0) is +0 (see mean_field in fused_loop.h).
//
// The filter runs two labels per pass (splat_blur's XIN form, as in k_multilabel), so the l'-sum of a term with a matrix is a
// RUNNING sum: pass p adds columns 2p and 2p + 1 of mu_k to sk[k][0 .. L) -- ascending l', the order above.  A term without a
// matrix keeps its sliced values in the same registers.  The accumulation into next waits for the last pass, so that the terms
// add in the order they were added whichever of them has a matrix.  Two layouts:
//     pair-major   every pass filters all K terms (ceil(L / 2) passes of splat_blur per iteration): K * L partial sums per point
//     term-major   term by term, ceil(L / 2) passes of the one-term mask each (K times the barriers): L partial sums per point
// multi_general_term_major() names the layout of every instantiation; the figures behind it are in the note.
//
// The matrices are uniform: the kernel reads them where it uses them from the engine's device array (Engine::LearntModel::
// compat_ptr, TermModel::mats_dev) through the constant address space -- nothing writes them while a launch runs -- so they
// arrive in scalar registers, a column pair per row at a time, and cost no vector register and no LDS.
//
// Shipped range (tests/test_fused_multilabel_learnt_resources.py holds the same table and checks every instantiation: at most 128
// registers per lane, no scratch, no spill):
//     L = 3, 4        frames of up to 2048 active points (one or two points per lane)
//     L = 5 .. 8      frames of up to 1024 active points (one point per lane)
// K in {1, 2} 2-D terms, kernel 0 with short rows or chain rows, a fixed iteration count, the self-contained prologue
// (fused_prologue.inc).  The convergence form, the fresh-frame kernels and the gradients: follow-ups.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kMultiMinL = 3, kMultiMaxL = 8;
// points per lane by label count: the shipped range above
constexpr int multi_general_max_ppt(int L) { return L <= 4 ? 2 : 1; }
// the layout by instantiation: pair-major wherever it compiles clean (fewer barriers); two points per lane of two terms on chain rows
// need 80 (L = 4) and 48 (L = 3) bytes of scratch that way and none term-major.  Built term-major, every two-term frame of one point
// per lane measured 7 to 14 us slower per inference(5, true): notes/fused_multilabel.md section 6.
constexpr bool multi_general_term_major(int PPT, int K, int CH) { return K == 2 && PPT == 2 && CH == 1; }

struct MultiGeneralArgs {
    KernelDev kd[kMaxFusedK];             // Engine::step_kdevs(): `norm` is the factor behind the filter
    const float *pre[kMaxFusedK];         // Engine::pre_arg()[k]: [F][maxN] factor in front of term k's filter, or null
    const float *mu[kMaxFusedK];          // term k's [L][L] matrix in HBM, row-major, or null
    FusedLayout lay;
    int n_iter, with_map;
    float relax;
};

// a matrix entry through the constant address space: a scalar load (the array is written by the host before the launch only)
typedef const __attribute__((address_space(4))) float *ConstFloats;

// (fused_multilabel.hip: the prologue's own float2 unary load is in bounds and unread; the L energies come with the first term)
#define FUSED_PROLOGUE_POINT                                                                            \
    if (k == 0) {                                                                                       \
        _Pragma("unroll") for (int l = 0; l < L; ++l) un[s][l] = c.unary[((size_t)f * c.maxN + ic) * L + l]; \
    }                                                                                                   \
    pre[s][k] = a.pre[k] ? a.pre[k][(size_t)f * kd.maxN + ic] : 1.0f;
template <int L, int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_multilabel_general(CrfDev c, MultiGeneralArgs a)
{
    constexpr int D1 = kD1, NT = kNT, NP = (L + 1) / 2;
    constexpr bool TM = multi_general_term_major(PPT, K, CH);
    constexpr int KS = TM ? 1 : K;        // terms whose partial sums are alive at a time
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};

    PointRegs<PPT, K> pr;
    float un[PPT][L], q[PPT][L], pre[PPT][K];
    int V[K];
#pragma unroll
    for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    const FusedLayout &lay = a.lay;

    if (N <= 0) return;                   // nothing to infer (and nothing below may index an empty frame)

    unsigned pk[PPT][K][D1];              // (vertex id + 1) | place in the row << 16
#include "fused_prologue.inc"
    __syncthreads();

    ChainLane cl{0u, 0u};
    if (CH != 0 && chain_k<CH>(lay, 0)) cl = chain_setup(smem, lay, V[0], tid);
    place_products<PPT, K, CH, NT>(smem, lay, N, tid, pk, pr);

    // startInference: Q = softmax(-unary), densecrf_base.h:78-80
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
#pragma unroll
        for (int l = 0; l < L; ++l) q[s][l] = 0.0f;
        if (tid + s * NT < N) exp_and_normalize_reg<L>(un[s], q[s], -1.0f, 1.0f);
    }

    float alpha[K];
#pragma unroll
    for (int k = 0; k < K; ++k) alpha[k] = a.kd[k].alpha;
    const float relax = a.relax;
    // the second channel of an odd L's last pair: +0.0f in an opaque register, its slice summed like a label's (fused_multilabel.hip)
    float pad = 0.0f;
    asm volatile("" : "+v"(pad));
    for (int it = 0; it < a.n_iter; ++it) {
        float nx[PPT][L], sk[PPT][KS][L], skpad = 0.0f;
        asm volatile("" : "+v"(tid));   // (mean_field's FENCE: what the phases derive from the lane index is formed where it is used)
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
#pragma unroll
            for (int l = 0; l < L; ++l) nx[s][l] = -un[s][l];               // stepInit, densecrf3d.h:154-158
        }
        // term k's filter input of label pair p at point slot s: x = pre * Q, rounded once (k_splat<true>), or Q itself
        auto input = [&](int s, int k, int p) {
            const bool scaled = a.pre[k] != nullptr;
            const float x0 = scaled ? pre[s][k] * q[s][2 * p] : q[s][2 * p];
            const float x1 = 2 * p + 1 < L ? (scaled ? pre[s][k] * q[s][2 * p + 1] : q[s][2 * p + 1]) : pad;
            return make_float2(x0, x1);
        };
        // behind pass p's slice of term k (partial sums in sk[.][j]): columns 2p and 2p + 1 of the running sum, or the values themselves
        auto gather = [&](int s, int k, int j, int p) {
            const float2 t = slice_point(smem, lay, pr, s, k, alpha[k]);
            if (a.mu[k]) {
                ConstFloats m = (ConstFloats)a.mu[k];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    sk[s][j][l] = sk[s][j][l] + m[l * L + 2 * p] * t.x;      // k_slice_compat: ascending l', each rounded
                    if (2 * p + 1 < L) sk[s][j][l] = sk[s][j][l] + m[l * L + 2 * p + 1] * t.y;
                }
                if (2 * p + 1 >= L) skpad += pr.wn[s][k] * t.y;
            } else {
                sk[s][j][2 * p] = t.x;
                if (2 * p + 1 < L) sk[s][j][2 * p + 1] = t.y;
                else skpad += pr.wn[s][k] * t.y;
            }
        };
        auto clear = [&](int s, int j) {
#pragma unroll
            for (int l = 0; l < L; ++l) sk[s][j][l] = 0.0f;                  // (literally 0: 0 + (-0) is +0)
        };
        auto apply = [&](int s, int k, int j) {
#pragma unroll
            for (int l = 0; l < L; ++l) nx[s][l] += pr.wn[s][k] * sk[s][j][l];   // pairwise3d.h:77
        };
        if constexpr (!TM) {
#pragma unroll
            for (int s = 0; s < PPT; ++s)
#pragma unroll
                for (int k = 0; k < K; ++k) clear(s, k);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                opaque(pr);               // (fused_loop.h: the loop invariants stay in the registers they came in)
                float2 xin[PPT][K];
#pragma unroll
                for (int s = 0; s < PPT; ++s)
#pragma unroll
                    for (int k = 0; k < K; ++k) xin[s][k] = input(s, k, p);
                splat_blur<PPT, K, CH, true, NT, (1 << K) - 1, false, false, false, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
                // (no barrier behind the slices: fused_multilabel.hip)
#pragma unroll
                for (int s = 0; s < PPT; ++s) {
                    if (tid + s * NT < N) {
#pragma unroll
                        for (int k = 0; k < K; ++k) gather(s, k, k, p);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PPT; ++s)
#pragma unroll
                for (int k = 0; k < K; ++k) apply(s, k, k);
        } else {
            auto term = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
#pragma unroll
                for (int s = 0; s < PPT; ++s) clear(s, 0);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    opaque(pr);
                    float2 xin[PPT][K];
#pragma unroll
                    for (int s = 0; s < PPT; ++s) xin[s][k] = input(s, k, p);
                    splat_blur<PPT, K, CH, true, NT, 1 << k, false, false, false, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
#pragma unroll
                    for (int s = 0; s < PPT; ++s)
                        if (tid + s * NT < N) gather(s, k, 0, p);
                }
#pragma unroll
                for (int s = 0; s < PPT; ++s) apply(s, k, 0);
            };
            term(std::integral_constant<int, 0>{});
            if constexpr (K > 1) term(std::integral_constant<int, 1>{});
        }
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            if (L & 1 && s == 0) asm volatile("" : : "v"(skpad));
            if (tid + s * NT < N) exp_and_normalize_reg<L>(nx[s], q[s], 1.0f, relax);   // densecrf3d.h:70-98
        }
    }

    // Q and the MAP labels (densecrf3d.h:136-151: the first maximum wins) of this lane's points
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        const int i = tid + s * NT;
        if (i < N) {
            float *out = c.Q + ((size_t)f * c.maxN + i) * L;
#pragma unroll
            for (int l = 0; l < L; ++l) out[l] = q[s][l];
            if (a.with_map) c.map[(size_t)f * c.maxN + i] = (int16_t)argmax_row(q[s], L);
        }
    }
}

// the frames the kernel is written for: 3 .. 8 labels, one or two 2-D kernels whose tables fit the u16 records, of at most the
// plan's active points, on lattices that fit the two-label LDS plan (sized by the largest frame and lattices)
bool multilabel_general_plan(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, FusedLayout *lay)
{
    if (c.L < kMultiMinL || c.L > kMultiMaxL || c.K < 1 || c.K > kMaxFusedK) return false;
    for (int k = 0; k < c.K; ++k)
        if (kds[k].d != 2 || kds[k].Epad >= 65535) return false;
    if (active_points(c) > multi_general_max_ppt(c.L) * kNT) return false;
    return layout_core(active_points(c), c.K, maxV, maxRow ? maxRow[0] : 0, lay);
}

}  // namespace

bool multilabel_general_supported(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow)
{
    FusedLayout lay;
    return multilabel_general_plan(c, kds, maxV, maxRow, &lay);
}

// kds: Engine::step_kdevs() -- `norm` is each term's factor behind the filter.  A fixed count (the caller has seen to the schedule).
// Frames outside the plan: 0.
int launch_multilabel_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq,
                              hipStream_t s)
{
    MultiGeneralArgs a{};
    if (rq.run.until_converged || !rq.terms.general() || !multilabel_general_plan(c, kds, maxV, maxRow, &a.lay)) return 0;
    if (rq.terms.mats && !rq.terms.mats_dev) return 0;
    for (int k = 0; k < c.K; ++k) {
        a.kd[k] = kds[k];
        a.pre[k] = rq.terms.pre ? rq.terms.pre[k] : nullptr;
        a.mu[k] = rq.terms.mats_dev ? rq.terms.mats_dev[k] : nullptr;
    }
    a.n_iter = rq.run.n_iter;
    a.with_map = rq.run.with_map;
    a.relax = rq.run.relax;
    const int ppt = std::max((active_points(c) + kNT - 1) / kNT, 1);
    with_dims<kMultiMinL, kMultiMaxL>(c.L, [&](auto ll) {
        with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
            with_dims<0, 1>(a.lay.chain0 ? 1 : 0, [&](auto ch) {
                with_dims<1, multi_general_max_ppt(decltype(ll)::value)>(ppt, [&](auto p) {
                    launch_workgroups(k_multilabel_general<decltype(ll)::value, decltype(p)::value, decltype(kk)::value, decltype(ch)::value>,
                                      c.F, kNT, a.lay.total, s, c, a);
                });
            });
        });
    });
    return fused_report(kNT, ppt, a.lay.chain0);
}

}  // namespace lccrf

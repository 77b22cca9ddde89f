// fused_multilabel.hip -- the fused engine's inference (fused_engine.hip: one launch, one 1024-lane workgroup per frame, the lattice
// side of the mean-field state on chip) for frames of THREE TO EIGHT labels.  Opt-in: LCCRF_OPT_FUSED_MULTILABEL; the engine
// report is 5.  notes/fused_multilabel.md.
//
// Why: every other one-workgroup kernel is a two-label kernel (slam_shaped), so a tracker-sized frame with a handful of classes ran
// on the streaming engine -- one launch per phase, 11 per iteration for the tracker's two 2-D terms, 57 for inference(5, true)
// (fused_general.hip), where a launch-per-phase design is bound by launch gaps.
//
// How: the permutohedral filter is linear and treats every label channel on its own (permutohedral_cpu.h:653-694): one vertex's value
// for one channel is the same left-to-right sum over the same (point, corner) order whatever the other channels hold.  An L-label
// filter is therefore ceil(L / 2) passes of the two-label filter fused_loop.h already has -- splat_blur in its XIN form, whose input
// at a point is the pair (q[2p], q[2p+1]), the last pair of an odd L padded with +0.0f (its products and sums are +0 and are never
// read back) -- and slice_point reads each pass's result.  The lattice tables and the LDS plan are the two-label plan unchanged
// (layout_core; each term its own product buffer or all of them one: splat_blur's WITH_P form serves both); only the point side is
// L wide, and it lives in registers: un[PPT][L], q[PPT][L] and the accumulator nx[PPT][L] beside PointRegs' ix / bary / wn.
//
// One iteration: nx = -un (stepInit, densecrf3d.h:154-158); for the label pairs in ascending order one splat_blur over ALL K terms,
// then per point and term, in the order the terms were added, nx[2p] += wn * t.x, nx[2p+1] += wn * t.y (pairwise3d.h:77) -- every
// pass handles all terms, so a label's sum runs over the terms in that order; then exp_and_normalize_reg<L> with the relax blend
// (densecrf3d.h:70-98).  Every product and every sum is rounded on its own (-ffp-contract=off).
//
// Shipped range (tests/test_fused_multilabel_resources.py holds the same table and checks every instantiation: at most 128
// registers per lane, no scratch, no spill):
//     L = 3, 4        frames of up to 2048 active points (one or two points per lane)
//     L = 5 .. 8      frames of up to 1024 active points (one point per lane: with two, the kernels of two terms on chain rows
//                     -- un, q and nx are 6 L registers beside the 32 of chain_rows' ring -- do not compile without scratch)
// K in {1, 2} 2-D Potts terms normalised AFTER the filter, kernel 0 with short rows or chain rows, a fixed iteration count, the
// self-contained prologue (fused_prologue.inc).  Matrices and normalisation modes at L > 2 would need K * L partial sums per point
// carried across the label pairs: the follow-up.  Label bits exist for two labels only: map_bits is not touched.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kMultiMinL = 3, kMultiMaxL = 8;
// points per lane by label count: the shipped range above
constexpr int multi_max_ppt(int L) { return L <= 4 ? 2 : 1; }

struct MultiArgs {
    KernelDev kd[kMaxFusedK];
    FusedLayout lay;
    int n_iter, with_map;
    float relax;
};

// The prologue's own unary load is a float2 at two-label stride: in bounds (the array holds L >= 3 floats per point) and meaningless
// here -- pr.un and pr.q are never read.  The L energies of a point come in with the first term's records.
#define FUSED_PROLOGUE_POINT                                                                            \
    if (k == 0) {                                                                                       \
        _Pragma("unroll") for (int l = 0; l < L; ++l) un[s][l] = c.unary[((size_t)f * c.maxN + ic) * L + l]; \
    }
template <int L, int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_multilabel(CrfDev c, MultiArgs a)
{
    constexpr int D1 = kD1, NT = kNT, NP = (L + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};

    PointRegs<PPT, K> pr;
    float un[PPT][L], q[PPT][L];
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
    // The second channel of an odd L's last pair: +0.0f, in a register the compiler knows nothing about, and its slice is summed
    // like a label's (nxpad) and handed to an empty asm: the last pass is then the code of every other pass.  With the literal and
    // the slice's second channel dropped, the short-row kernels of odd L at one point per lane came out of hipcc with the copy of a
    // barycentric weight into the register pair of a packed multiply left out ("; kill: def $vgprA killed $vgprB" in the assembly)
    // and computed garbage; tests/test_fused_multilabel_resources.py looks for that remark, tests/test_fused_multilabel.py runs
    // every instantiation on the GPU.
    float pad = 0.0f;
    asm volatile("" : "+v"(pad));
    for (int it = 0; it < a.n_iter; ++it) {
        float nx[PPT][L], nxpad[PPT];      // (nxpad: see pad)
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            nxpad[s] = 0.0f;
#pragma unroll
            for (int l = 0; l < L; ++l) nx[s][l] = -un[s][l];               // stepInit, densecrf3d.h:154-158
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            opaque(pr);                   // (fused_loop.h: the loop invariants stay in the registers they came in)
            float2 xin[PPT][K];
#pragma unroll
            for (int s = 0; s < PPT; ++s)
#pragma unroll
                for (int k = 0; k < K; ++k) xin[s][k] = make_float2(q[s][2 * p], 2 * p + 1 < L ? q[s][2 * p + 1] : pad);
            splat_blur<PPT, K, CH, true, NT, (1 << K) - 1, false, false, false, true>(smem, lay, V, N, tid, pr, cl, ins, nullptr, xin);
            // No barrier behind the slices: the next pass's products go to the product buffers and its row sums to val[k][0], whose
            // readers are two barriers back; val[k][1], which the slices read, is first written behind two more.
#pragma unroll
            for (int s = 0; s < PPT; ++s) {
                if (tid + s * NT < N) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float2 t = slice_point(smem, lay, pr, s, k, alpha[k]);
                        nx[s][2 * p] += pr.wn[s][k] * t.x;                  // pairwise3d.h:77
                        if (2 * p + 1 < L) nx[s][2 * p + 1] += pr.wn[s][k] * t.y;
                        else nxpad[s] += pr.wn[s][k] * t.y;
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            if (L & 1) asm volatile("" : : "v"(nxpad[s]));
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

// the frames the kernel is written for: 3 .. 8 labels, one or two 2-D kernels whose tables fit the u16 records
bool multilabel_shaped(const CrfDev &c, const KernelDev *kds)
{
    if (c.L < kMultiMinL || c.L > kMultiMaxL || c.K < 1 || c.K > kMaxFusedK) return false;
    for (int k = 0; k < c.K; ++k)
        if (kds[k].d != 2 || kds[k].Epad >= 65535) return false;
    return true;
}

// ... of at most the plan's active points, on lattices that fit the two-label LDS plan (sized by the largest frame and lattices)
bool multilabel_plan(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, FusedLayout *lay)
{
    if (!multilabel_shaped(c, kds) || active_points(c) > multi_max_ppt(c.L) * kNT) return false;
    return layout_core(active_points(c), c.K, maxV, maxRow ? maxRow[0] : 0, lay);
}

}  // namespace

bool multilabel_supported(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow)
{
    FusedLayout lay;
    return multilabel_plan(c, kds, maxV, maxRow, &lay);
}

// A fixed count of Potts iterations (the caller has seen to the terms and the schedule).  Frames outside the plan: 0.
int launch_multilabel(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s)
{
    MultiArgs a{};
    if (rq.run.until_converged || rq.terms.general() || !multilabel_plan(c, kds, maxV, maxRow, &a.lay)) return 0;
    for (int k = 0; k < c.K; ++k) a.kd[k] = kds[k];
    a.n_iter = rq.run.n_iter;
    a.with_map = rq.run.with_map;
    a.relax = rq.run.relax;
    const int ppt = std::max((active_points(c) + kNT - 1) / kNT, 1);
    with_dims<kMultiMinL, kMultiMaxL>(c.L, [&](auto ll) {
        with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
            with_dims<0, 1>(a.lay.chain0 ? 1 : 0, [&](auto ch) {
                with_dims<1, multi_max_ppt(decltype(ll)::value)>(ppt, [&](auto p) {
                    launch_workgroups(k_multilabel<decltype(ll)::value, decltype(p)::value, decltype(kk)::value, decltype(ch)::value>,
                                      c.F, kNT, a.lay.total, s, c, a);
                });
            });
        });
    });
    return fused_report(kNT, ppt, a.lay.chain0);
}

}  // namespace lccrf

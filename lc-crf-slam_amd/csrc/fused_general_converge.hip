// fused_general_converge.hip -- the fused engine's kernel for terms with a label-compatibility matrix or a normalisation mode
// (fused_general.hip: include/lccrf.h sections 1e and 1g) run UNTIL CONVERGED, at most max_iter iterations (sections 1h and 2e), for
// every frame of a batch in ONE launch: notes/batch_general.md.
//
// Why: a learnt model -- weights, a 2 x 2 matrix and a normalisation mode per term -- is evaluated over a capture as a batch, and
// "until the labels settle" on such a batch used to be the streaming step with the bookkeeping of converge_track.hip behind it: 11
// launches and one host read per iteration, every frame stepped until the last one has finished.  Here a frame is one workgroup
// that stops on its own and leaves its CU to the next frame.
//
// The loop is fused_loop.h's, in its GEN and CONV forms at once: k_general's arithmetic (x = pre * Q rounded once, section 1e's sum
// behind the slice, w * post), k_converge's reduction (converge_decide: two registers per lane, one barrier per iteration, 16 bytes
// of LDS behind the plan), so Q_t is bit for bit what k_general leaves after t iterations and the report is k_converge's.
//
// Scope: k_general's -- frames of up to 2 x 1024 active points, K in {1, 2} 2-D terms, kernel 0 with short rows or chain rows, the
// self-contained prologue only (fused_prologue.inc): 8 instantiations, in a unit of their own so that a change to this kernel leaves
// k_general and k_converge the code they are.
//
// Registers.  <2, 2, 1> (the C2 shape) is the tight one: with k_general's text around the CONV loop it spills 11 vector and 4 scalar
// registers, 48 bytes of scratch per lane.  Two things bring all eight to none (notes/batch_general.md section 2; the means are
// k_frame_converge's, notes/convergence.md section 2): the arguments are read where they are used, through a copy of the argument
// segment's address the compiler cannot see through, instead of being held from the entry on; and the loop fences the lane index once
// per iteration in this form (fused_loop.h: mean_field, under `if constexpr (GEN && CONV)`), so that what the phases derive from it --
// the blur passes' and the chain rows' addresses -- is formed where it is used and not kept in registers around the whole loop.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kGeneralConvergeMaxPPT = 2; // points per lane: k_general's bound

struct GeneralConvergeArgs {
    KernelDev kd[kMaxFusedK];             // Engine::step_kdevs(): `norm` is the factor behind the filter
    const float *pre[kMaxFusedK];         // Engine::pre_arg()[k]: [F][maxN] factor in front of term k's filter, or null
    float mu[kMaxFusedK][4];              // term k's matrix, row-major, by value: uniform in the kernel
    int has_mu;                           // bit k: term k has a matrix
    FusedLayout lay;
    int max_iter, with_map, criterion;
    float relax, tol;
    ConvergeOut out;
};

// The arguments as the phase that is about to run sees them: the same segment, behind an address the compiler cannot follow, so
// that what a late phase needs is loaded there (scalar loads, a few per phase) and not kept in registers from the entry on.
// (frame_build.h's late_args; the kernel's arguments are CrfDev, then GeneralConvergeArgs, by value, naturally aligned, in order)
constexpr int kArgOff = (int)((sizeof(CrfDev) + alignof(GeneralConvergeArgs) - 1) / alignof(GeneralConvergeArgs) * alignof(GeneralConvergeArgs));
static_assert(alignof(CrfDev) == 8 && alignof(GeneralConvergeArgs) == 8, "the kernel's arguments as the ABI lays them out");
__device__ __forceinline__ const GeneralConvergeArgs &late(const GeneralConvergeArgs &)
{
    typedef const __attribute__((address_space(4))) unsigned char *kptr;
    kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const GeneralConvergeArgs *)(p + kArgOff);
}

// k_general's prologue and GeneralTerms (fused_general.hip) around the loop's GEN + CONV form, k_converge's words and report
// (fused_converge.hip).  The prologue is fused_prologue.inc's, with the pre factors beside the norms and the reduction's words,
// both parities, zeroed behind the plan (GeneralTerms' uniform members are set behind the barrier, where the loop reads them).
#define FUSED_PROLOGUE_POINT gt.pre[s][k] = a.pre[k] ? a.pre[k][(size_t)f * kd.maxN + ic] : 1.0f;
#define FUSED_PROLOGUE_WORDS if (tid < 4) reinterpret_cast<unsigned *>(smem + lay.total)[tid] = 0u;
template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_general_converge(CrfDev c, GeneralConvergeArgs a0)
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
    {
        const GeneralConvergeArgs &a = late(a0);
#pragma unroll
        for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    }

    if (N <= 0) {                         // nothing to infer (and nothing below may index an empty frame): 0 / 0.0f / 0 / 0
        const GeneralConvergeArgs &a = late(a0);
        if (a.with_map) clear_label_bits<NT>(c, f, 0, tid);
        if (tid == 0) report_convergence(a.out, f, 0, 0.0f, 0, 0);
        return;
    }

    unsigned pk[PPT][K][D1];              // (vertex id + 1) | place in the row << 16
    {
        const GeneralConvergeArgs &a = late(a0);
        const FusedLayout &lay = a.lay;
#include "fused_prologue.inc"
    }
    __syncthreads();

    Converge cv;
    {
        const GeneralConvergeArgs &a = late(a0);
        const FusedLayout &lay = a.lay;
        ChainLane cl{0u, 0u};
        if (CH != 0 && chain_k<CH>(lay, 0)) cl = chain_setup(smem, lay, V[0], tid);
        start_inference<PPT, K, NT>(pr, N, tid);
        place_products<PPT, K, CH, NT>(smem, lay, N, tid, pk, pr);

        gt.has_pre = 0;
        gt.has_mu = a.has_mu;
        float alpha[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (a.pre[k]) gt.has_pre |= 1 << k;
#pragma unroll
            for (int e = 0; e < 4; ++e) gt.mu[k][e] = a.mu[k][e];
            alpha[k] = a.kd[k].alpha;
        }
        cv = Converge{a.criterion, a.tol, lay.total, 0, 0, 0, 0u};
        mean_field<PPT, K, CH, NT, true, true, true>(smem, lay, V, N, tid, pr, cl, alpha, a.max_iter, a.relax, ins, -1, &gt, &cv);
    }

    const GeneralConvergeArgs &a = late(a0);
    store_results<PPT, K, NT>(c, f, N, tid, pr, a.with_map);
    if (tid == 0) report_convergence(a.out, f, cv.iterations, __uint_as_float(cv.delta), cv.changed, cv.converged);   // (uniform values)
}

}  // namespace

// launch_general's frames and terms (fused_general.hip) under launch_converge's stop rule and report (fused_converge.hip); a plan
// without room for the reduction's words: 0
int launch_general_converge(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq,
                            hipStream_t s)
{
    GeneralConvergeArgs a{};
    fill_converge_run(a, rq);
    return plan_variant<kGeneralConvergeMaxPPT>(c, kds, maxV, maxRow, kConvergeLds, a, [&](auto p, auto kk, auto ch) {
        fill_general_terms(a, c, rq.terms);
        launch_workgroups(k_general_converge<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT,
                          a.lay.total + kConvergeLds, s, c, a);
    });
}

}  // namespace lccrf

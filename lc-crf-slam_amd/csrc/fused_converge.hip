// fused_converge.hip -- the fused engine's inference (fused_engine.hip: one launch, one 1024-lane workgroup per frame, the mean-field
// state on chip) run UNTIL CONVERGED, at most max_iter iterations: include/lccrf.h sections 1h and 2e, notes/convergence.md.
//
// Why: every other way into inference runs a fixed iteration count.  A caller who wants settled labels either overpays every frame
// or steps the handle from the host -- one launch and one synchronisation per iteration, the launch-gap regime the fused engine
// exists to avoid -- and for a batch cannot hold a converged frame still at all.  Here a frame's whole state lives in one
// workgroup, the old and the new Q of a point meet in one lane's registers at the softmax, and the stop decision is uniform: a
// workgroup whose frame has converged stores its results and leaves the CU to the next frame.
//
// The loop is fused_loop.h's, in its CONV form: ordered row sums, chain rows, blur, softmax2, relax blending, store_results and the
// label bits are the fused engine's code, so Q_t is bit for bit what k_fused leaves after t iterations.  The reduction
// (fused_loop.h: converge_decide) costs two registers per lane, one barrier per iteration and 16 bytes of LDS behind the plan.
//
// Scope: handles and batches alike, frames of up to 4 x 1024 active points, K in {1, 2} 2-D terms, kernel 0 with short rows or
// chain rows, the self-contained prologue only (fused_prologue.inc: the one text k_fused includes too): 16 instantiations, kept in a
// unit of their own so that a change to this kernel leaves the fused engine's kernels the code they are.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kConvergeMaxPPT = 4;        // points per lane

struct ConvergeArgs {
    KernelDev kd[kMaxFusedK];
    FusedLayout lay;
    int max_iter, with_map, criterion;
    float relax, tol;
    ConvergeOut out;
};

// k_fused<1024, PPT, K, CH, 0> (fused_engine.hip) with the loop's convergence form: the same self-contained prologue
// (fused_prologue.inc), which here also zeroes the reduction's words, both parities.
#define FUSED_PROLOGUE_WORDS if (tid < 4) reinterpret_cast<unsigned *>(smem + cv.words)[tid] = 0u;
template <int PPT, int K, int CH>
__global__ void __launch_bounds__(kNT, 4) k_converge(CrfDev c, ConvergeArgs a)
{
    constexpr int D1 = kD1, NT = kNT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{nullptr, 0, 0, 0, 0};

    PointRegs<PPT, K> pr;
    int V[K];
#pragma unroll
    for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    const FusedLayout &lay = a.lay;
    Converge cv{a.criterion, a.tol, lay.total, 0, 0, 0, 0u};

    if (N <= 0) {                         // nothing to infer (and nothing below may index an empty frame): 0 / 0.0f / 0 / 0
        if (a.with_map) clear_label_bits<NT>(c, f, 0, tid);
        if (tid == 0) report_convergence(a.out, f, 0, 0.0f, 0, 0);
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
    mean_field<PPT, K, CH, NT, true, false, true>(smem, lay, V, N, tid, pr, cl, alpha, a.max_iter, a.relax, ins, -1, nullptr, &cv);

    store_results<PPT, K, NT>(c, f, N, tid, pr, a.with_map);
    if (tid == 0) report_convergence(a.out, f, cv.iterations, __uint_as_float(cv.delta), cv.changed, cv.converged);   // (uniform values)
}

}  // namespace

// frames that are not slam_shaped, beyond 4096 active points, or whose plan leaves no room for the reduction's words: 0
int launch_converge(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s)
{
    ConvergeArgs a{};
    fill_converge_run(a, rq);
    return plan_variant<kConvergeMaxPPT>(c, kds, maxV, maxRow, kConvergeLds, a, [&](auto p, auto kk, auto ch) {
        launch_workgroups(k_converge<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT,
                          a.lay.total + kConvergeLds, s, c, a);
    });
}

}  // namespace lccrf

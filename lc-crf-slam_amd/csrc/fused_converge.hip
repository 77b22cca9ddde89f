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
// chain rows, the self-contained prologue only: 16 instantiations, kept in a unit of their own so that the fused engine's kernels
// compile exactly as they did.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_variant.h"

namespace lccrf {

namespace {

using namespace fl;

constexpr int kConvergeMaxPPT = 4;        // points per lane
constexpr int kConvergeLds = 16;          // the reduction's four words behind the plan

struct ConvergeArgs {
    KernelDev kd[kMaxFusedK];
    FusedLayout lay;
    int max_iter, with_map, criterion;
    float relax, tol;
    ConvergeOut out;
};

// k_fused<1024, PPT, K, CH, 0> (fused_engine.hip) with the loop's convergence form: the same self-contained prologue -- every
// global load issued before anything waits, indices clamped instead of branched on.
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
        if (tid == 0) {
            a.out.iterations[f] = 0;
            a.out.delta[f] = 0.0f;
            a.out.changed[f] = 0;
            a.out.converged[f] = 0;
        }
        return;
    }

    constexpr int kNbrRounds = 4096 / NT, kRowRounds = 2048 / NT;   // covers V <= 1365 in registers; larger lattices finish in copy loops
    unsigned g_nbr[K][kNbrRounds];
    int g_row[K][kRowRounds];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const KernelDev &kd = a.kd[k];
        const unsigned *gn = kd.nbr16 + (size_t)f * D1 * kd.Epad;            // already (n1+1) | (n2+1) << 16
        const int *gr = kd.rowptr + (size_t)f * (kd.Epad + 1);
#pragma unroll
        for (int r = 0; r < kNbrRounds; ++r) {            // element idx = j*V + v, j-major like the LDS copy
            const int idx = min(tid + r * NT, D1 * V[k] - 1);
            const int j = idx >= 2 * V[k] ? 2 : (idx >= V[k] ? 1 : 0);
            g_nbr[k][r] = gn[(size_t)j * kd.Epad + (idx - j * V[k])];
        }
#pragma unroll
        for (int r = 0; r < kRowRounds; ++r) g_row[k][r] = gr[min(tid + r * NT, V[k])];
    }
    unsigned pk[PPT][K][D1];              // (vertex id + 1) | place in the row << 16
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        const int ic = min(tid + s * NT, N - 1);
        pr.un[s] = reinterpret_cast<const float2 *>(c.unary)[(size_t)f * c.maxN + ic];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const KernelDev &kd = a.kd[k];
            const size_t e0 = (size_t)f * kd.Epad + (size_t)ic * D1;
#pragma unroll
            for (int j = 0; j < D1; ++j) {
                pk[s][k][j] = kd.pk[e0 + j];
                pr.bary[s][k][j] = kd.bary[e0 + j];
            }
            pr.wn[s][k] = kd.norm[(size_t)f * kd.maxN + ic];
        }
    }
#pragma unroll
    for (int s = 0; s < PPT; ++s)
#pragma unroll
        for (int k = 0; k < K; ++k) pr.wn[s][k] = a.kd[k].w * pr.wn[s][k];   // pairwise3d.h:77 (w_*norm_[i])

    // ---- per-frame lattice tables into LDS --------------------------------------------
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned *nbr = reinterpret_cast<unsigned *>(smem + lay.nbr[k]);
        unsigned short *row = reinterpret_cast<unsigned short *>(smem + lay.row[k]);
#pragma unroll
        for (int r = 0; r < kNbrRounds; ++r) {
            const int idx = tid + r * NT;
            if (idx < D1 * V[k]) nbr[idx] = g_nbr[k][r];
        }
#pragma unroll
        for (int r = 0; r < kRowRounds; ++r)
            if (tid + r * NT <= V[k]) row[tid + r * NT] = (unsigned short)g_row[k][r];
        // lattices with more vertices than the register rounds cover (sparse frames): plain copy loops
        const KernelDev &kd = a.kd[k];
        const unsigned *gn = kd.nbr16 + (size_t)f * D1 * kd.Epad;
        for (int idx = tid + kNbrRounds * NT; idx < D1 * V[k]; idx += NT) {
            const int j = idx >= 2 * V[k] ? 2 : (idx >= V[k] ? 1 : 0);
            nbr[idx] = gn[(size_t)j * kd.Epad + (idx - j * V[k])];
        }
        const int *gr = kd.rowptr + (size_t)f * (kd.Epad + 1);
        for (int v = tid + kRowRounds * NT; v <= V[k]; v += NT) row[v] = (unsigned short)gr[v];
    }
    if (tid < 16) reinterpret_cast<float *>(smem + lay.zero)[tid] = 0.0f;
    if (tid < 4) reinterpret_cast<unsigned *>(smem + cv.words)[tid] = 0u;    // the reduction's words, both parities
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            reinterpret_cast<float2 *>(smem + lay.val[k][0])[0] = make_float2(0.f, 0.f);
            reinterpret_cast<float2 *>(smem + lay.val[k][1])[0] = make_float2(0.f, 0.f);
        }
    }
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
    if (tid == 0) {                       // (uniform values: every lane holds them)
        a.out.iterations[f] = cv.iterations;
        a.out.delta[f] = __uint_as_float(cv.delta);
        a.out.changed[f] = cv.changed;
        a.out.converged[f] = cv.converged;
    }
}

}  // namespace

int launch_inference_converged(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int max_iter, int criterion,
                               float tol, int with_map, float relax, const ConvergeOut &out, hipStream_t s)
{
    ConvergeArgs a{};
    a.max_iter = max_iter;
    a.with_map = with_map;
    a.criterion = criterion;
    a.relax = relax;
    a.tol = tol;
    a.out = out;
    // (a plan that leaves no room for the reduction's words: the caller streams)
    return plan_variant<kConvergeMaxPPT>(c, kds, maxV, maxRow, kConvergeLds, a, [&](auto p, auto kk, auto ch) {
        launch_workgroups(k_converge<decltype(p)::value, decltype(kk)::value, decltype(ch)::value>, c.F, kNT,
                          a.lay.total + kConvergeLds, s, c, a);
    });
}

}  // namespace lccrf

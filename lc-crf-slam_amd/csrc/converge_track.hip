// converge_track.hip -- convergence-driven inference (include/lccrf.h sections 1h and 2e) for everything the one-launch kernel of
// fused_converge.hip does not take: any label count, dimension, term count and size, terms with a matrix or a normalisation mode,
// locality mode, lattices beyond LDS.  The streaming engine's step runs unchanged; these kernels run BEHIND each step and
//   compare   the current Q of every running frame with the kept copy of its previous Q -- the largest |difference| through an
//             integer atomicMax on the float's bits (non-negative floats order as their bits), the flipped MAP labels through an
//             atomicAdd on a counter: both exact and order-free, so d_t and c_t are the values the definitions give --
//             and refresh the copy;
//   settle    per frame whether it has finished (the criterion met, or the cap reached), and count the frames still running into
//             one pinned word, the only thing the host reads per iteration.
// A finished frame's copy is no longer refreshed: it IS the frame's Q at the iteration it finished.  Frames never interact, so
// stepping a finished frame of a batch further is wasted work but harmless; launch_track_restore puts its kept Q back before the
// labels are formed.
#include "stream_common.h"
#include "device_math.h"

namespace lccrf {
namespace {

constexpr int kSettleLanes = 1024;

__global__ void __launch_bounds__(kBlock) k_track_begin(CrfDev c, ConvergeTrack tk, int max_iter)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= c.F) return;
    tk.acc[2 * f] = tk.acc[2 * f + 1] = 0u;
    tk.done[f] = (c.n_points[f] <= 0 || max_iter == 0) ? 1 : 0;
    tk.out.iterations[f] = 0;
    tk.out.delta[f] = 0.0f;
    tk.out.changed[f] = 0;
    tk.out.converged[f] = 0;
}

// dst[f][i][:] = src[f][i][:] for the points of every frame (restore: of the frames that finished before step t_last)
__global__ void __launch_bounds__(kBlock) k_track_copy(CrfDev c, ConvergeTrack tk, float *__restrict__ dst, const float *__restrict__ src,
                                                       int t_last)
{
    const int f = blockIdx.y;
    if (t_last > 0 && !(tk.done[f] && tk.out.iterations[f] < t_last)) return;
    const int n = c.n_points[f] * c.L;
    const size_t base = (size_t)f * c.maxN * c.L;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) dst[base + i] = src[base + i];
}

// one lane per point of a running frame
__global__ void __launch_bounds__(kBlock) k_track_compare(CrfDev c, ConvergeTrack tk)
{
    __shared__ unsigned sh[2];
    const int f = blockIdx.y, L = c.L;
    if (tk.done[f]) return;                               // (uniform in the workgroup)
    const int N = c.n_points[f];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0u;
    __syncthreads();
    unsigned d = 0u, flips = 0u;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
        const float *q = c.Q + ((size_t)f * c.maxN + i) * L;
        float *p = tk.prev + ((size_t)f * c.maxN + i) * L;
        flips += argmax_row(q, L) != argmax_row(p, L);     // densecrf3d.h:140-149 on both: the first maximum wins
        for (int l = 0; l < L; ++l) {
            const float x = q[l];
            d = max(d, __float_as_uint(fabsf(x - p[l])));
            p[l] = x;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                    // (every lane of the workgroup is here)
        d = max(d, (unsigned)__shfl_xor((int)d, o));
        flips += (unsigned)__shfl_xor((int)flips, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&sh[0], d);
        atomicAdd(&sh[1], flips);
    }
    __syncthreads();
    if (threadIdx.x == 0 && (sh[0] | sh[1])) {
        atomicMax(&tk.acc[2 * f], sh[0]);
        atomicAdd(&tk.acc[2 * f + 1], sh[1]);
    }
}

// ONE workgroup: every running frame's report for iteration t, whether it has finished, and the count of those that have not
__global__ void __launch_bounds__(kSettleLanes) k_track_settle(int F, ConvergeTrack tk, int t, int max_iter, int criterion, float tol)
{
    __shared__ int running;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    int mine = 0;
    for (int f = threadIdx.x; f < F; f += kSettleLanes) {
        if (tk.done[f]) continue;
        const unsigned d = tk.acc[2 * f], ch = tk.acc[2 * f + 1];
        const bool met = (!(criterion & LCCRF_STOP_DELTA) || __uint_as_float(d) <= tol) && (!(criterion & LCCRF_STOP_LABELS) || ch == 0u);
        tk.out.iterations[f] = t;
        tk.out.delta[f] = __uint_as_float(d);
        tk.out.changed[f] = (int)ch;
        tk.out.converged[f] = met ? 1 : 0;
        if (met || t >= max_iter) {
            tk.done[f] = 1;
        } else {
            tk.acc[2 * f] = tk.acc[2 * f + 1] = 0u;
            ++mine;
        }
    }
    if (mine) atomicAdd(&running, mine);
    __syncthreads();
    if (threadIdx.x == 0) *tk.running = running;
}

inline dim3 point_grid(const CrfDev &c)
{
    const long nb = ((long)active_points(c) + kBlock - 1) / kBlock;
    return dim3((unsigned)std::min(std::max(nb, 1L), 64L), (unsigned)c.F);
}

}  // namespace

void launch_track_begin(const CrfDev &c, const ConvergeTrack &tk, int max_iter, hipStream_t s)
{
    k_track_begin<<<(c.F + kBlock - 1) / kBlock, kBlock, 0, s>>>(c, tk, max_iter);
    k_track_copy<<<point_grid(c), kBlock, 0, s>>>(c, tk, tk.prev, c.Q, 0);
}

void launch_track_step(const CrfDev &c, const ConvergeTrack &tk, int t, int max_iter, int criterion, float tol, hipStream_t s)
{
    k_track_compare<<<point_grid(c), kBlock, 0, s>>>(c, tk);
    k_track_settle<<<1, kSettleLanes, 0, s>>>(c.F, tk, t, max_iter, criterion, tol);
}

void launch_track_restore(const CrfDev &c, const ConvergeTrack &tk, int t_last, hipStream_t s)
{
    k_track_copy<<<point_grid(c), kBlock, 0, s>>>(c, tk, c.Q, tk.prev, t_last);
}

}  // namespace lccrf

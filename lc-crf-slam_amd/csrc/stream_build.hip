// stream_build.hip -- lattice construction of the streaming engine: per kernel and frame the vertices, the entries' vertex ids and
// barycentric weights, the blur neighbour tables and the splat's CSR rows, by the hash build or the sorted build of locality mode.
// Compiled with -ffp-contract=off: the reference is an SSE2 build without FMA, so every a*b+c must stay two roundings.
// Reference being restated (paths under the reference's Thirdparty/DenseCRF/include/):
//   lattice construction   permutohedral_cpu.h:241-424   -> k_points / k_insert / k_offsets / k_neighbors
#include "stream_common.h"
#include "lattice_device.h"
#include <algorithm>
#include <cstdlib>

namespace lccrf {
namespace {

// grid coordinates of a lattice vertex in the basis of the blur directions, c_j = (x_d - x_j) / (d+1) ("locality mode, part two" below)
template <int D>
__device__ __forceinline__ void vertex_grid_coords(const int16_t (&key)[D], int (&c)[D])
{
    int xd = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) xd -= key[j];
#pragma unroll
    for (int j = 0; j < D; ++j) c[j] = (xd - key[j]) / (D + 1);          // exact: the coordinates are congruent mod d+1
}

// One thread per point (phantom lanes included): elevate, round, rank, barycentric.
// ref: permutohedral_cpu.h:294-366.
// VB: also leave, per workgroup, the bounds of the grid coordinates of every corner this workgroup's points touch (locality mode's
// vertex order, k_vsort_plan below) in vpartial[f][blockIdx.x][2 * kMaxD]
template <int D, bool VB>
__global__ void __launch_bounds__(kBlock) k_points(KernelDev kd, const int *__restrict__ n_points, int *__restrict__ vpartial, int *__restrict__ vbad)
{
    constexpr int D1 = D + 1;
    __shared__ int red[VB ? kBlock / 64 : 1][2 * D];
    const int f = blockIdx.y;
    const int N = n_points[f];
    const int Npad = (N + 3) & ~3;                       // blocks of four, :294
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const bool live = n < Npad;
    if (!VB && !live) return;
    int lo[D], hi[D];
#pragma unroll
    for (int j = 0; j < D; ++j) { lo[j] = 0x7fffffff; hi[j] = (int)0x80000000; }
    if (live) {
        float feat[D];
        const int src = (kd.perm && n < N) ? kd.perm[(size_t)f * kd.maxNpad + n] : n;   // locality mode: position n holds point perm[n]
        const float *fp = kd.feat + ((size_t)f * kd.maxN + src) * D;
#pragma unroll
        for (int j = 0; j < D; ++j) feat[j] = (n < N) ? fp[j] : 0.0f;   // phantom lanes, :299
        if (VB) {
            // Keys are int16 (the reference's `short`, permutohedral_cpu.h:304-366).  A feature thousands of cells wide wraps them, and a
            // wrapped key is no lattice point any more: the sorted build matches neighbours by code +- stride, the hash build by the
            // wrapped key itself -- they differ at the +-32768 seam (and when d + 1 divides 65536 the integrality check of k_ecode
            // cannot see the wrap: ADVICE r4).  Every |elevated coordinate| <= (d+1) sum |f_j scale_j|, a key is within 2 (d+1) of it:
            // a point that could leave the int16 range hands the frame to the hash build (pinned flag, conservative).
            float mag = 2.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) mag += fabsf(feat[j] * kd.scale[j]);
            if (!(mag * (float)D1 < 32000.0f) && vbad) *vbad = 1;
        }

        int16_t r0[D];
        uint8_t rk[D];
        float b[D1];
        point_record<D>(feat, kd.scale, kd.inv_dp1, r0, rk, b);

        int16_t *r0p = kd.rem0 + ((size_t)f * kd.maxNpad + n) * D;
        uint8_t *rkp = kd.rank + ((size_t)f * kd.maxNpad + n) * D;
        float *bp = kd.bary + (size_t)f * kd.Epad + (size_t)n * D1;
#pragma unroll
        for (int i = 0; i < D; ++i) { r0p[i] = r0[i]; rkp[i] = rk[i]; }
#pragma unroll
        for (int i = 0; i < D1; ++i) bp[i] = b[i];
        if (VB) {
#pragma unroll
            for (int rem = 0; rem < D1; ++rem) {
                int16_t key[D];
                int c[D];
#pragma unroll
                for (int i = 0; i < D; ++i) key[i] = vertex_coord<D>(r0[i], rk[i], rem);
                vertex_grid_coords<D>(key, c);
#pragma unroll
                for (int j = 0; j < D; ++j) { lo[j] = min(lo[j], c[j]); hi[j] = max(hi[j], c[j]); }
            }
        }
    }
    if (VB) {                                             // (every lane of the workgroup gets here: one barrier for all)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            int l = lo[j], h = hi[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                l = min(l, __shfl_xor(l, o, 64));
                h = max(h, __shfl_xor(h, o, 64));
            }
            if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][2 * j] = l; red[threadIdx.x >> 6][2 * j + 1] = h; }
        }
        __syncthreads();
        if (threadIdx.x < 2 * D) {
            int x = red[0][threadIdx.x];
            for (int w = 1; w < kBlock / 64; ++w) x = (threadIdx.x & 1) ? max(x, red[w][threadIdx.x]) : min(x, red[w][threadIdx.x]);
            vpartial[((size_t)f * gridDim.x + blockIdx.x) * 2 * kMaxD + threadIdx.x] = x;
        }
    }
}

// One thread per entry: insert its vertex key into the frame's hash table.  A slot ends up
// holding the LOWEST entry id carrying that key, i.e. the entry at which the reference's
// sequential HashTableCPU::find(create=true) would have created the vertex (:134-161,371-377).
template <int D>
__global__ void __launch_bounds__(kBlock) k_insert(KernelDev kd, const int *__restrict__ n_points, int F, XcdMap nb)
{
    constexpr int D1 = D + 1;
    const FrameBlock fb = frame_block(nb);               // many frames: one XCD per frame, its table stays in that L2
    const int f = fb.f;
    if (f >= F) return;
    const int Npad = (n_points[f] + 3) & ~3;
    const int e = fb.bx * kBlock + threadIdx.x;
    if (e >= Npad * D1) return;

    int16_t key[D];
    load_entry_key<D>(kd, f, e, key);
    const unsigned mask = (unsigned)kd.cap - 1u;
    unsigned h = hash_key<D>(key) & mask;
    int *slot = kd.slot + (size_t)f * kd.cap;
    for (;;) {
        const int prev = atomicCAS(&slot[h], kEmpty, e);
        if (prev == kEmpty || prev == e) break;
        int16_t other[D];
        load_entry_key<D>(kd, f, prev, other);
        bool same = true;
#pragma unroll
        for (int i = 0; i < D; ++i) same &= (other[i] == key[i]);
        if (same) { atomicMin(&slot[h], e); break; }
        h = (h + 1u) & mask;
    }
    kd.slot_of[(size_t)f * kd.Epad + e] = (int)h;
}

// flag[e] = 1 iff entry e is the first occurrence of its vertex.
__global__ void __launch_bounds__(kBlock) k_first_flag(KernelDev kd, const int *__restrict__ n_points)
{
    const int f = blockIdx.y;
    const int live = ((n_points[f] + 3) & ~3) * kd.D1;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e > kd.Epad) return;
    int v = 0;
    if (e < live) {
        const int s = kd.slot_of[(size_t)f * kd.Epad + e];
        v = (kd.slot[(size_t)f * kd.cap + s] == e);
    }
    kd.flag[(size_t)f * (kd.Epad + 1) + e] = v;
}

// Exclusive scan of n ints per frame, any n, by many workgroups: every workgroup scans a tile of kScanTile
// elements and leaves the tile's total (k_scan_tiles), one workgroup per frame scans the tile totals
// (k_scan_totals), every tile adds its prefix (k_scan_apply).  in/out strided by `stride` per frame; the grand
// total goes to total[f] if non-null.  (Round 1 scanned a frame with ONE workgroup: 0.75 ms per 700k entries.)
constexpr int kScanTile = 4096;           // 1024 lanes x 4 consecutive elements

__device__ __forceinline__ int wave_incl_scan_i32(int x)     // DPP: row_shr 1,2,4,8 then row_bcast:15 / :31
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return x;
}

// exclusive prefix of one value per lane over a 1024-lane workgroup; `total` = sum over the workgroup
__device__ __forceinline__ int block_excl_scan_1024(int x, int &total)
{
    __shared__ int wave_sum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan_i32(x);
    __syncthreads();
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    const int ws = lane < 16 ? wave_sum[lane] : 0;
    const int wincl = wave_incl_scan_i32(ws);
    total = __builtin_amdgcn_readlane(wincl, 15);
    return __builtin_amdgcn_readlane(wincl - ws, __builtin_amdgcn_readfirstlane(wave)) + incl - x;
}

__global__ void __launch_bounds__(1024) k_scan_tiles(const int *__restrict__ in, int *__restrict__ out, int n, int stride,
                                                     int *__restrict__ tile_sum, int tiles)
{
    const int f = blockIdx.y, t = blockIdx.x;
    in += (size_t)f * stride;
    out += (size_t)f * stride;
    const int i0 = t * kScanTile + threadIdx.x * 4;
    int x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = (i0 + u < n) ? in[i0 + u] : 0;
    int total;
    int run = block_excl_scan_1024(x[0] + x[1] + x[2] + x[3], total);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (i0 + u < n) out[i0 + u] = run;                // prefix inside the tile; k_scan_apply adds the tiles before it
        run += x[u];
    }
    if (threadIdx.x == 0) tile_sum[(size_t)f * tiles + t] = total;
}

__global__ void __launch_bounds__(1024) k_scan_totals(int *__restrict__ tile_sum, int tiles, int *__restrict__ total)
{
    const int f = blockIdx.x;
    int *ts = tile_sum + (size_t)f * tiles;
    int carry = 0;
    for (int base = 0; base < tiles; base += 1024) {      // (one round up to 4M elements per frame)
        const int i = base + threadIdx.x;
        const int x = i < tiles ? ts[i] : 0;
        int tot;
        const int ex = block_excl_scan_1024(x, tot);
        if (i < tiles) ts[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (total && threadIdx.x == 0) total[f] = carry;
}

__global__ void __launch_bounds__(1024) k_scan_apply(int *__restrict__ out, int n, int stride, const int *__restrict__ tile_sum,
                                                     int tiles)
{
    const int f = blockIdx.y, t = blockIdx.x;
    const int add = tile_sum[(size_t)f * tiles + t];
    out += (size_t)f * stride;
    const int i0 = t * kScanTile + threadIdx.x * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (i0 + u < n) out[i0 + u] += add;
}

// tile_sum: scratch of F * ceil(n / kScanTile) ints
void scan_frames(const int *in, int *out, int n, int stride, int *total, int *tile_sum, int F, hipStream_t s)
{
    const int tiles = (n + kScanTile - 1) / kScanTile;
    k_scan_tiles<<<dim3(tiles, F), 1024, 0, s>>>(in, out, n, stride, tile_sum, tiles);
    k_scan_totals<<<F, 1024, 0, s>>>(tile_sum, tiles, total);
    if (tiles > 1) k_scan_apply<<<dim3(tiles, F), 1024, 0, s>>>(out, n, stride, tile_sum, tiles);
}

// ---------------------------------------------------------------------------------------
// locality mode: an internal ordering of a frame's points along a Z-order curve of their lattice cells
// ---------------------------------------------------------------------------------------
// The blur pass gathers two neighbour values per vertex; with the reference's vertex numbering (insertion order = point
// order) the neighbours that belong to OTHER points' simplices sit anywhere in the frame's value array, and every miss
// moves a 128-byte line for 8 useful bytes (profiles/r3_fetchcal).  Numbering follows the order in which points are
// processed, so processing them cell by cell along a space-filling curve puts the vertices of neighbouring cells next to
// each other.  Only locality depends on this order, never a result: it is a counting sort on a 2^bits-bucket Z-order code
// (one pass, atomics; buckets of up to 64 points are then put in index order so the order is reproducible).

// cell of every real point: the remainder-0 lattice point's first D coordinates / (D+1), permutohedral_cpu.h:304-319;
// per-dimension min / max of every workgroup's cells go to ss.partial (reduced per frame by k_sort_plan)
template <int D>
__global__ void __launch_bounds__(kBlock) k_sort_cells(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    __shared__ int red[kBlock / 64][2 * D];
    const int f = blockIdx.y;
    const int N = n_points[f];
    const int n = blockIdx.x * kBlock + threadIdx.x;
    int cell[D];
    const bool live = n < N;
    {
        float feat[D];
        const float *fp = kd.feat + ((size_t)f * kd.maxN + (live ? n : 0)) * D;
#pragma unroll
        for (int j = 0; j < D; ++j) feat[j] = N > 0 ? fp[j] : 0.0f;
        float el[D + 1];
        float sm = 0.0f;
#pragma unroll
        for (int j = D; j > 0; --j) {
            const float cf = feat[j - 1] * kd.scale[j - 1];
            el[j] = sm - (float)j * cf;
            sm += cf;
        }
        el[0] = sm;
#pragma unroll
        for (int j = 0; j < D; ++j) cell[j] = __float2int_rn(kd.inv_dp1 * el[j]);
        if (ss.rm_points) {                               // the sorted build's companion: cells in the lattice's own basis, c_j ~ v_d - v_j
            const int vd = __float2int_rn(kd.inv_dp1 * el[D]);
#pragma unroll
            for (int j = 0; j < D; ++j) cell[j] = vd - cell[j];
        }
    }
    if (live) {
        int *cp = ss.cells + ((size_t)f * kd.maxNpad + n) * kMaxD;
#pragma unroll
        for (int j = 0; j < D; ++j) cp[j] = cell[j];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        int lo = live ? cell[j] : 0x7fffffff, hi = live ? cell[j] : (int)0x80000000;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][2 * j] = lo;
            red[threadIdx.x >> 6][2 * j + 1] = hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * D) {
        int x = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) x = (threadIdx.x & 1) ? max(x, red[w][threadIdx.x]) : min(x, red[w][threadIdx.x]);
        ss.partial[((size_t)f * gridDim.x + blockIdx.x) * 2 * kMaxD + threadIdx.x] = x;
    }
}

// One workgroup per frame: bounds of the frame's cells, then the plan of the Z-order code -- the `bits` code bits are
// dealt to the dimensions by their spans (the widest remaining span gets the next bit).  plan[f] = {lo[kMaxD], span[kMaxD], nb[kMaxD]}.
__global__ void __launch_bounds__(kBlock) k_sort_plan(int D, int nblocks, SortScratch ss)
{
    __shared__ int red[kBlock / 64][2 * kMaxD];
    __shared__ int bnd[2 * kMaxD];
    const int f = blockIdx.x;
    for (int j = 0; j < D; ++j) {
        int lo = 0x7fffffff, hi = (int)0x80000000;
        for (int b = threadIdx.x; b < nblocks; b += kBlock) {
            const int *pp = ss.partial + ((size_t)f * nblocks + b) * 2 * kMaxD;
            lo = min(lo, pp[2 * j]);
            hi = max(hi, pp[2 * j + 1]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][2 * j] = lo;
            red[threadIdx.x >> 6][2 * j + 1] = hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * D) {
        int x = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) x = (threadIdx.x & 1) ? max(x, red[w][threadIdx.x]) : min(x, red[w][threadIdx.x]);
        bnd[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int *plan = ss.plan + (size_t)f * kSortPlan;
        plan[3 * kMaxD] = plan[3 * kMaxD + 1] = 0;         // (k_sort_place's two counters, report only)
        long rem[kMaxD];
        int nb[kMaxD];
        for (int j = 0; j < D; ++j) {
            const int lo = bnd[2 * j], hi = bnd[2 * j + 1];
            const int span = hi >= lo ? hi - lo + 1 : 1;   // (an empty frame has no cells)
            plan[j] = hi >= lo ? lo : 0;
            plan[kMaxD + j] = span;
            rem[j] = span;
            nb[j] = 0;
        }
        for (int b = 0; b < ss.bits; ++b) {
            int best = 0;
            for (int j = 1; j < D; ++j)
                if (rem[j] > rem[best]) best = j;
            ++nb[best];
            rem[best] = (rem[best] + 1) >> 1;
        }
        for (int j = 0; j < D; ++j) plan[2 * kMaxD + j] = nb[j];
    }
}

// Z-order bucket of every point: each coordinate quantised to its share of the code bits, bits interleaved level by level
template <int D>
__global__ void __launch_bounds__(kBlock) k_sort_code(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int N = n_points[f];
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int *plan = ss.plan + (size_t)f * kSortPlan;
    const int *cp = ss.cells + ((size_t)f * kd.maxNpad + n) * kMaxD;
    if (ss.rm_points) {
        // points in (coarse) ROW-MAJOR order of their cell in the lattice's own basis -- the order the sorted build gives the vertices:
        // the points of consecutive vertices' rows are then close together too (splat), and so are the corners of consecutive points
        unsigned long long code = 0, range = 1;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            code += (unsigned long long)(unsigned)(cp[j] - plan[j]) * range;
            range *= (unsigned long long)(unsigned)plan[kMaxD + j];          // (spans of cells: a product beyond 2^64 only scrambles an order)
        }
        unsigned b = range >> ss.bits ? (unsigned)(code / ((range >> ss.bits) + 1)) : (unsigned)code;
        b = min(b, (1u << ss.bits) - 1u);                 // (a product of spans beyond 2^64 wraps: any bucket will do, inside the histogram)
        ss.code[(size_t)f * kd.maxNpad + n] = (int)b;
        atomicAdd(&ss.hist[(size_t)f * ((1 << ss.bits) + 1) + b], 1);
        return;
    }
    unsigned q[D];
    int nb[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        nb[j] = plan[2 * kMaxD + j];
        q[j] = (unsigned)((((unsigned long long)(unsigned)(cp[j] - plan[j])) << nb[j]) / (unsigned)plan[kMaxD + j]);
    }
    unsigned code = 0;
    int pos = 0;
    for (int level = 0; level < ss.bits && pos < ss.bits; ++level)
#pragma unroll
        for (int j = 0; j < D; ++j)
            if (nb[j] > level) code |= ((q[j] >> level) & 1u) << pos++;
    ss.code[(size_t)f * kd.maxNpad + n] = (int)code;
    atomicAdd(&ss.hist[(size_t)f * ((1 << ss.bits) + 1) + code], 1);
}

// arrival order of the scatter is arbitrary: ss.cells (dead by now) takes the unordered buckets ...
__global__ void __launch_bounds__(kBlock) k_sort_scatter(int maxNpad, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_points[f]) return;
    const int code = ss.code[(size_t)f * maxNpad + n];
    const int pos = atomicAdd(&ss.start[(size_t)f * ((1 << ss.bits) + 1) + code], 1);   // start[c] ends up at the END of bucket c
    ss.cells[(size_t)f * maxNpad * kMaxD + pos] = n;
}

// ... and every point takes the place of its rank inside its bucket, so the order is reproducible (index order inside
// buckets of up to 64 points; larger buckets -- everything in one cell -- keep their arrival order: locality only)
__global__ void __launch_bounds__(kBlock) k_sort_place(int maxNpad, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int pos = blockIdx.x * kBlock + threadIdx.x;
    int *p = ss.perm + (size_t)f * maxNpad, *ip = ss.iperm + (size_t)f * maxNpad;
    int *counted = ss.plan + (size_t)f * kSortPlan + 3 * kMaxD;   // report only: {buckets of more than 64 points, the largest bucket}
    int len = 0;
    if (pos < maxNpad && pos >= n_points[f]) {           // phantom lanes and the unused tail: identity
        p[pos] = pos;
        ip[pos] = pos;
    } else if (pos < maxNpad) {
        const int *tmp = ss.cells + (size_t)f * maxNpad * kMaxD;
        const int *end = ss.start + (size_t)f * ((1 << ss.bits) + 1);
        const int i = tmp[pos], c = ss.code[(size_t)f * maxNpad + i];
        const int lo = c ? end[c - 1] : 0, hi = end[c];
        int at = pos;
        len = hi - lo;
        if (len <= 64) {
            at = lo;
            for (int q = lo; q < hi; ++q) at += tmp[q] < i;
        } else if (pos == lo) {
            atomicAdd(&counted[0], 1);                   // (one per bucket that keeps its arrival order)
        }
        p[at] = i;
        ip[i] = at;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o, 64));
    if ((threadIdx.x & 63) == 0 && len > __builtin_nontemporal_load(&counted[1])) atomicMax(&counted[1], len);   // (a look first, as k_eneighbors)
}

template <int D>
void sort_points_d(const KernelDev &kd, const CrfDev &c, const SortScratch &ss, hipStream_t s)
{
    const int F = c.F, nbk = (1 << ss.bits) + 1;
    const dim3 gp = grid_for(kd.maxNpad, F);
    (void)hipMemsetAsync(ss.hist, 0, (size_t)F * nbk * sizeof(int), s);
    k_sort_cells<D><<<gp, kBlock, 0, s>>>(kd, c.n_points, ss);
    k_sort_plan<<<F, kBlock, 0, s>>>(D, (int)gp.x, ss);
    k_sort_code<D><<<gp, kBlock, 0, s>>>(kd, c.n_points, ss);
    scan_frames(ss.hist, ss.start, nbk, nbk, nullptr, ss.tiles, F, s);
    k_sort_scatter<<<gp, kBlock, 0, s>>>(kd.maxNpad, c.n_points, ss);
    k_sort_place<<<gp, kBlock, 0, s>>>(kd.maxNpad, c.n_points, ss);
}

// ---- locality mode, part two: the VERTICES in row-major order of the lattice's own axes --------------------------------------
// A lattice vertex is x in Z^(d+1) with sum 0 and all coordinates congruent mod d+1 (its key = the first d of them).  In the basis
// of the blur directions u_j = (1, .., 1) - (d+1) e_j it is the integer point c with c_j = (x_d - x_j) / (d+1), j < d: blur axis
// j < d is the unit step along c_j and axis d the step along the main diagonal (permutohedral_cpu.h:408-421 in those
// coordinates).  Numbering the vertices in ROW-MAJOR order of c makes the neighbours of consecutive ids consecutive ids of
// another row: a wavefront's blur gather touches 9 distinct 128-byte lines instead of 19 (scripts/sim_vertex_order.py, the C5
// lattice) and the pass takes 19.5 instead of 23.2 us per 8 frames (scripts/ubench/blurorder.hip on the real tables).  Only
// locality depends on the numbering, never a result (a vertex's value is a sum over its own row, neighbours are matched by key).
// One-pass bucket sort on the top ~20 bits of the code (a histogram, its scan, a scatter); a bucket is ~200 consecutive codes -- a
// few lattice rows, one or two vertices -- and keeps its arrival order.

// One workgroup per frame: bounds of the grid coordinates -> row-major strides (coordinate 0 fastest) and the shift that maps a
// code to its bucket.  vplan[f] = {lo[kMaxD], stride[kMaxD], bucket scale, usable, range}; a lattice whose bounding box overflows 62 bits
// (features spread over thousands of cells in every dimension) raises *vbad and is rebuilt with the hash table.
constexpr int kVPlan = 2 * kMaxD + 3;
__global__ void __launch_bounds__(kBlock) k_vsort_plan(int D, int nblocks, SortScratch ss, int *__restrict__ bstat)
{
    __shared__ int red[kBlock / 64][2 * kMaxD];
    __shared__ int bnd[2 * kMaxD];
    const int f = blockIdx.x;
    for (int j = 0; j < D; ++j) {
        int lo = 0x7fffffff, hi = (int)0x80000000;
        for (int b = threadIdx.x; b < nblocks; b += kBlock) {
            const int *pp = ss.vpartial + ((size_t)f * nblocks + b) * 2 * kMaxD;
            lo = min(lo, pp[2 * j]);
            hi = max(hi, pp[2 * j + 1]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][2 * j] = lo;
            red[threadIdx.x >> 6][2 * j + 1] = hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * D) {
        int x = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) x = (threadIdx.x & 1) ? max(x, red[w][threadIdx.x]) : min(x, red[w][threadIdx.x]);
        bnd[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long *plan = ss.vplan + (size_t)f * kVPlan;
        unsigned long long range = 1;
        bool ok = true;
        for (int j = 0; j < D; ++j) {
            const int lo = bnd[2 * j], hi = bnd[2 * j + 1];
            // one EMPTY guard column per dimension: a step of +-1 off the edge of the box lands in it (or beyond `range`) and finds no
            // vertex, so the neighbour search needs no coordinate arithmetic (k_eneighbors)
            const unsigned long long span = hi >= lo ? (unsigned long long)((long long)hi - lo + 2) : 2ull;   // (an empty frame has no vertices)
            plan[j] = hi >= lo ? lo : 0;
            plan[kMaxD + j] = (long long)range;
            if (span > (1ull << 62) / range) ok = false;
            else range *= span;
        }
        // bucket of a code = floor(code * buckets / range) as a multiply-high: the whole histogram is used whatever the range (a
        // shift would leave up to half of it empty and make the buckets twice as long).  0 = the code itself (range <= buckets).
        // An unusable plan "codes" the entries by their own index (k_ecode): the same formula over [0, vcap) keeps them inside.
        const unsigned long long reff = ok ? range : (unsigned long long)ss.vcap, nbuckets = 1ull << ss.vbits;
        plan[2 * kMaxD] = reff <= nbuckets ? 0ll : (long long)((~0ull / reff) << ss.vbits);
        plan[2 * kMaxD + 1] = ok ? 1 : 0;
        plan[2 * kMaxD + 2] = (long long)reff;             // (unusable plan: whatever k_eneighbors derives from the meaningless strides stays inside too)
        if (!ok && ss.vbad) *ss.vbad = 1;                 // pinned host word: the host rebuilds these lattices with the hash
        // report only (cleared by the build's first memset): the code is its own bucket, and what the point sort counted for this CRF
        int *st = bstat + (size_t)f * kBuildStats;
        st[kBsDirect] = (ok && plan[2 * kMaxD] == 0) ? 1 : 0;
        st[kBsPtOver64] = ss.plan[(size_t)f * kSortPlan + 3 * kMaxD];
        st[kBsPtLargest] = ss.plan[(size_t)f * kSortPlan + 3 * kMaxD + 1];
    }
}

// ---- the SORTED build of locality mode (round 4): vertices found and numbered by sorting the entries ---------------------------
// Every entry e = (point, remainder) gets the row-major code of its vertex; a bucket sort on the code's top ~21 bits + an exact
// order inside each bucket by (code, entry) makes the entries of one vertex a RUN whose first element is the vertex's first
// occurrence: run starts -> scan -> ids in row-major order, with no hash table, no first-occurrence pass and no separate vertex
// sort; blur neighbours are then found by CODE (the neighbour along axis j has code +- stride_j) among the few vertices of the
// bucket that code falls in -- one contiguous read instead of a hash probe plus a key recomputation.  Everything downstream
// (offset, rep, V, nbr, the CSR kernels) sees the same arrays as after the hash build, with other ids.
constexpr int kLongBucket = 512;          // buckets beyond this are sorted by a workgroup of their own (identical or clustered features)
constexpr int kVPh = 64;                  // ints per frame of the phantom-entry list: count, then up to 3 (d+1) <= 27 positions
// one splat contribution: entry e of vertex v at position pos of the frame's CSR (k_eoffsets here, k_csr_order / k_csr_sort_long below)
__device__ __forceinline__ void csr_emit(const KernelDev &kd, size_t fe, int pos, int e, int v)
{
    kd.csr_pt[fe + pos] = e / kd.D1;
    kd.csr_w[fe + pos] = kd.bary[fe + e];
    kd.csr_pos[fe + e] = pos;
    if (kd.Epad < 65535) kd.pk[fe + e] = (unsigned)(v + 1) | ((unsigned)pos << 16);
}

__device__ __forceinline__ int vsort_bucket(const SortScratch &ss, int f, unsigned long long code)
{
    const unsigned long long scale = (unsigned long long)ss.vplan[(size_t)f * kVPlan + 2 * kMaxD];
    return scale ? (int)__umul64hi(code, scale) : (int)code;
}

template <int D>
__global__ void __launch_bounds__(kBlock) k_ecode(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int live = ((n_points[f] + 3) & ~3) * (D + 1);
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= live) return;
    const long long *plan = ss.vplan + (size_t)f * kVPlan;
    unsigned long long code = (unsigned long long)e;                      // (unusable plan: the host rebuilds with the hash; stay in bounds)
    if (plan[2 * kMaxD + 1]) {
        int16_t key[D];
        int c[D];
        load_entry_key<D>(kd, f, e, key);
        vertex_grid_coords<D>(key, c);
        code = 0;
        int xd = 0;
        bool exact = true;
#pragma unroll
        for (int j = 0; j < D; ++j) xd -= key[j];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            code += (unsigned long long)((long long)c[j] - plan[j]) * (unsigned long long)plan[kMaxD + j];
            exact &= (xd - key[j]) == c[j] * (D + 1);
        }
        // keys that wrapped around int16 (features thousands of cells wide: the reference's short arithmetic wraps the same way) are no
        // lattice points any more and the code would not tell them apart: such a frame is rebuilt with the hash, which compares keys
        if (!exact && ss.vbad) *ss.vbad = 1;
    }
    ss.vcode[(size_t)f * ss.vcap + e] = code;
    // the histogram's atomic hands back the entry's arrival number inside its bucket: the scatter below needs no second round of atomics
    kd.csr_pos[(size_t)f * kd.Epad + e] = atomicAdd(&ss.vhist[(size_t)f * ((1 << ss.vbits) + 1) + vsort_bucket(ss, f, code)], 1);
}

// bucket b = positions [vstart[b], vstart[b+1]).  slot_of takes the entries bucket by bucket (unordered inside), rep -- free until
// k_eoffsets -- the same entries under their ORIGINAL id: a vertex's row is ordered by original point index whatever the internal
// order of the points (quirk Q6), and that is the order the runs are given.
__global__ void __launch_bounds__(kBlock) k_escatter(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int live = ((n_points[f] + 3) & ~3) * kd.D1;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= live) return;
    const size_t fe = (size_t)f * kd.Epad;
    const int b = vsort_bucket(ss, f, ss.vcode[(size_t)f * ss.vcap + e]);
    const int pos = ss.vstart[(size_t)f * ((1 << ss.vbits) + 1) + b] + kd.csr_pos[fe + e];
    const int pt = e / kd.D1;
    kd.slot_of[fe + pos] = e;
    kd.rep[fe + pos] = kd.perm[(size_t)f * kd.maxNpad + pt] * kd.D1 + (e - pt * kd.D1);
}

__device__ __forceinline__ bool entry_less(unsigned long long ca, int oa, unsigned long long cb, int ob) { return ca < cb || (ca == cb && oa < ob); }

// exact order inside every bucket: (code, original entry id).  kd.slot (the hash table of the other build) takes the sorted entries.
__global__ void __launch_bounds__(kBlock) k_eorder(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int live = ((n_points[f] + 3) & ~3) * kd.D1;
    const int pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos >= live) return;
    const int *tmp = kd.slot_of + (size_t)f * kd.Epad, *toe = kd.rep + (size_t)f * kd.Epad;
    const unsigned long long *code = ss.vcode + (size_t)f * ss.vcap;
    const int *start = ss.vstart + (size_t)f * ((1 << ss.vbits) + 1);
    const int e = tmp[pos], oe = toe[pos];
    const unsigned long long ce = code[e];
    const int b = vsort_bucket(ss, f, ce);
    const int lo = start[b], hi = start[b + 1];
    int *sorted = kd.slot + (size_t)f * kd.cap;
    if (hi - lo > kLongBucket) {
        if (pos == lo) sorted[kd.Epad + atomicAdd(&kd.rowmax[f], 1)] = b;                 // (second half of the table: the list of long buckets)
        return;
    }
    int r = 0;
    for (int q = lo; q < hi; ++q) r += entry_less(code[tmp[q]], toe[q], ce, oe);
    sorted[lo + r] = e;
}

// One workgroup per long bucket: bitonic sort of its entries by (code, original id) in place, then out (as k_csr_sort_long).
constexpr int kSortBitmapWords = 15872;  // 62 KB of LDS: original ids spanning up to ~508 000
__global__ void __launch_bounds__(kBlock) k_esort_long(KernelDev kd, SortScratch ss, int *__restrict__ bstat)
{
    __shared__ unsigned bm[kSortBitmapWords];
    __shared__ int chunk_base[kBlock];
    __shared__ int s_mixed, s_min, s_max;
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    const int nlong = kd.rowmax[f];
    int *tmp = kd.slot_of + (size_t)f * kd.Epad, *toe = kd.rep + (size_t)f * kd.Epad;
    int *sorted = kd.slot + (size_t)f * kd.cap;
    const unsigned long long *code = ss.vcode + (size_t)f * ss.vcap;
    const int *start = ss.vstart + (size_t)f * ((1 << ss.vbits) + 1);
    int *st = bstat + (size_t)f * kBuildStats;            // report only: which way each long bucket went (lane 0: one atomic per bucket)
    int mine = 0;
    if (blockIdx.x == 0 && tid == 0) st[kBsLongBuckets] = nlong;
    for (int li = blockIdx.x; li < nlong; li += gridDim.x) {
        ++mine;
        const int b = sorted[kd.Epad + li];
        const int lo = start[b], n = start[b + 1] - lo;
        int *r = tmp + lo, *ro = toe + lo;
        // A giant bucket is usually ONE vertex (a whole uniformly coloured region of the image demo: 50 000 entries of the same code),
        // where the order wanted is the order of the original ids: a presence bitmap over the ids' range in LDS, prefix popcounts,
        // done -- O(n) instead of the 136 global-memory stages of the bitonic network below (0.8 ms per such bucket).
        if (tid == 0) { s_mixed = 0; s_min = INT_MAX; s_max = INT_MIN; }
        __syncthreads();
        {
            const unsigned long long c0 = code[r[0]];
            int mn = INT_MAX, mx = INT_MIN, mixed = 0;
            for (int i = tid; i < n; i += kBlock) {
                mixed |= code[r[i]] != c0;
                mn = min(mn, ro[i]);
                mx = max(mx, ro[i]);
            }
            if (mixed) s_mixed = 1;
            atomicMin(&s_min, mn);
            atomicMax(&s_max, mx);
        }
        __syncthreads();
        const int base_id = s_min, words = (s_max - s_min) / 32 + 1;
        if (tid == 0)
            atomicAdd(&st[s_mixed ? kBsNetMixed : n < 1024 ? kBsNetUniform : words <= kSortBitmapWords ? kBsBitmap : kBsNetWide], 1);
        if (!s_mixed && words <= kSortBitmapWords && n >= 1024) {       // (uniform; below ~1000 entries the network is cheaper than a walk over the span's words)
            for (int w = tid; w < words; w += kBlock) bm[w] = 0u;
            __syncthreads();
            for (int i = tid; i < n; i += kBlock) atomicOr(&bm[(ro[i] - base_id) >> 5], 1u << ((ro[i] - base_id) & 31));
            __syncthreads();
            const int chunk = (words + kBlock - 1) / kBlock;                 // words per lane
            int cnt = 0;
            for (int w = tid * chunk; w < min((tid + 1) * chunk, words); ++w) cnt += __popc(bm[w]);
            chunk_base[tid] = cnt;
            __syncthreads();
            if (tid == 0) {
                int run = 0;
                for (int t = 0; t < kBlock; ++t) { const int c = chunk_base[t]; chunk_base[t] = run; run += c; }
            }
            __syncthreads();
            for (int i = tid; i < n; i += kBlock) {
                const int b = ro[i] - base_id, w = b >> 5;
                int pos = chunk_base[w / chunk] + __popc(bm[w] & ((1u << (b & 31)) - 1u));
                for (int u = (w / chunk) * chunk; u < w; ++u) pos += __popc(bm[u]);
                sorted[lo + pos] = r[i];
            }
            __syncthreads();
            continue;
        }
        int np2 = 1;
        while (np2 < n) np2 <<= 1;
        for (int k = 2; k <= np2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < np2; i += kBlock) {
                    const int l = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);
                    if (l > i && l < n) {
                        const int a = r[i], c = r[l], oa = ro[i], oc = ro[l];
                        if (entry_less(code[c], oc, code[a], oa)) { r[i] = c; r[l] = a; ro[i] = oc; ro[l] = oa; }
                    }
                }
                __syncthreads();
            }
        }
        for (int i = threadIdx.x; i < n; i += kBlock) sorted[lo + i] = r[i];
        __syncthreads();
    }
    if (tid == 0 && mine > 0) atomicMax(&st[kBsMaxPerWg], mine);
}

// flag[pos] = 1 where a run (= a vertex) starts; the (at most 3 (d+1)) entries of the phantom points are listed by position --
// they make vertices but no products, and sit at the END of their runs (their original ids are the largest)
__global__ void __launch_bounds__(kBlock) k_eflag(KernelDev kd, const int *__restrict__ n_points, SortScratch ss)
{
    const int f = blockIdx.y;
    const int N = n_points[f], live = ((N + 3) & ~3) * kd.D1;
    const int pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos > kd.Epad) return;
    int v = 0;
    if (pos < live) {
        const int *sorted = kd.slot + (size_t)f * kd.cap;
        const unsigned long long *code = ss.vcode + (size_t)f * ss.vcap;
        const int e = sorted[pos];
        v = pos == 0 || code[sorted[pos - 1]] != code[e];
        if (e >= N * kd.D1) ss.vph[(size_t)f * kVPh + 1 + atomicAdd(&ss.vph[(size_t)f * kVPh], 1)] = pos;
    }
    kd.flag[(size_t)f * (kd.Epad + 1) + pos] = v;
}

// ids, representatives, and the CSR of splat contributions straight from the sorted runs: a run minus its trailing phantom entries
// IS the vertex's row in ascending original point order (what k_csr_count / fill / order / sort_long produce for the hash build)
__global__ void __launch_bounds__(kBlock) k_eoffsets(KernelDev kd, const int *__restrict__ n_points, SortScratch ss, int *__restrict__ bstat)
{
    const int f = blockIdx.y;
    const int N = n_points[f], live = ((N + 3) & ~3) * kd.D1;
    const int pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos >= live) return;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int e = kd.slot[(size_t)f * kd.cap + pos];
    const int first = kd.flag[f1 + pos];
    const int id = kd.prefix[f1 + pos] + first - 1;                       // (exclusive scan of the run starts)
    const int *ph = ss.vph + (size_t)f * kVPh;
    const int nph = ph[0];
    int before = 0;
    for (int u = 0; u < nph; ++u) before += ph[1 + u] < pos;               // phantom entries ahead of this position
    const int cpos = pos - before;
    kd.offset[fe + e] = id;
    if (first) {
        kd.rep[fe + id] = e;                                              // the run's first element = the vertex's first occurrence
        ss.vkey[(size_t)f * ss.vcap + id] = ss.vcode[(size_t)f * ss.vcap + e];
        kd.rowptr[f1 + id] = cpos;
        // (report only: a run that STARTS with a phantom entry holds nothing else -- a vertex with an empty row; at most 3 (d+1) of them)
        if (e >= N * kd.D1) atomicAdd(&bstat[(size_t)f * kBuildStats + kBsEmptyRows], 1);
    }
    if (pos == 0) {
        kd.rowptr[f1 + kd.V[f]] = live - nph;
        bstat[(size_t)f * kBuildStats + kBsPhantom] = nph;
    }
    if (e < N * kd.D1) csr_emit(kd, fe, cpos, e, id);
}

// vhist (free after its scan) takes, per bucket, the id of the bucket's first vertex: ids are bucket-major, so bucket b holds the
// vertices [bvert[b], bvert[b+1]) and the neighbour search reads one 8-byte pair instead of two positions and two prefixes
__global__ void __launch_bounds__(kBlock) k_ebucket_vertices(KernelDev kd, SortScratch ss)
{
    const int f = blockIdx.y, nbk = (1 << ss.vbits) + 1;
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nbk) return;
    ss.vhist[(size_t)f * nbk + b] = kd.prefix[(size_t)f * (kd.Epad + 1) + ss.vstart[(size_t)f * nbk + b]];   // (prefix[live] = V)
}

// One thread per vertex v, all d + 1 axes at once: n2_j(v) by code -- +1 along grid coordinate j (j < d), -1 along every coordinate
// (j = d); a step off the box lands in a guard column or beyond `range` and matches nothing -- among the vertices of the bucket the
// code falls in (ids are bucket-major: bucket b holds the vertices [bvert[b], bvert[b+1])).  The look-ups of the d + 1 axes are
// independent, so their loads are issued together (a thread per (axis, vertex) ran three dependent loads at a time: 0.46 ms per 8
// C5 frames).  The relation is mutual, so finding n2 fills both sides (the table was preset to -1).  ref: permutohedral_cpu.h:408-421.
template <int D>
__global__ void __launch_bounds__(kBlock) k_eneighbors(KernelDev kd, int F, XcdMap nb, SortScratch ss)
{
    constexpr int D1 = D + 1;
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int v = fb.bx * kBlock + threadIdx.x;
    if (v >= V) return;
    const long long *plan = ss.vplan + (size_t)f * kVPlan;
    const unsigned long long *vkey = ss.vkey + (size_t)f * ss.vcap;
    const int *bvert = ss.vhist + (size_t)f * ((1 << ss.vbits) + 1);
    const unsigned long long code = vkey[v], range = (unsigned long long)plan[2 * kMaxD + 2];
    unsigned long long target[D1], sum = 0;
    bool ok[D1];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const unsigned long long st = (unsigned long long)plan[kMaxD + j];
        target[j] = code + st;                            // + 1 along c_j
        ok[j] = target[j] < range;
        sum += st;
    }
    target[D] = code - sum;                               // - 1 along every coordinate
    ok[D] = code >= sum;
    int v0[D1], v1[D1];
    // axis 0 needs no bucket: it is the code's fastest coordinate and the ids follow the codes, so code + 1 -- if it exists -- is the
    // next id (one coalesced read of the neighbouring lane's key instead of a bucket pair and a key)
    v0[0] = v + 1;
    v1[0] = min(v + 2, V);
#pragma unroll
    for (int j = 1; j < D1; ++j) {
        const int b = ok[j] ? vsort_bucket(ss, f, target[j]) : 0;
        v0[j] = bvert[b];
        v1[j] = bvert[b + 1];
    }
    unsigned long long first[D1];
#pragma unroll
    for (int j = 0; j < D1; ++j) first[j] = vkey[min(v0[j], V - 1)];
    bool next0 = false;
    int dist[kNdistAxes] = {};           // |neighbour id - id| along the first axes (the splat's window, KernelDev::ndist)
#pragma unroll
    for (int j = 0; j < D1; ++j) {
        if (!ok[j] || v0[j] >= v1[j]) continue;
        int found = first[j] == target[j] ? v0[j] : -1;
        for (int u = v0[j] + 1; found < 0 && u < v1[j]; ++u)
            if (vkey[u] == target[j]) found = u;
        if (found < 0) continue;
        if (j == 0) {                    // axis 0 is the code's fastest coordinate: code + 1 is the next id
            next0 = true;
            if (found != v + 1 && kd.tbl_bad) kd.tbl_bad[1] = 1;
        }
        if (j < kNdistAxes) dist[j] = abs(found - v);
        if ((j == 1 || j == 2) && kd.nearoff) {          // the window passes' table: signed byte offsets (unused unless all of them fit)
            const int o = found - v;
            int8_t *no = kd.nearoff + ((size_t)f * 2 + (j - 1)) * kd.Epad * 2;
            const bool fits = o >= -127 && o <= 127;     // (the main diagonal, axis d, steps DOWN the codes: o < 0)
            no[2 * (size_t)v + 1] = (int8_t)(fits ? o : 0);               // my n2
            no[2 * (size_t)found] = (int8_t)(fits ? -o : 0);              // its n1
        }
        int *nbp = kd.nbr + ((size_t)f * D1 + j) * kd.Epad * 2;
        nbp[2 * v + 1] = found;          // my n2
        nbp[2 * found] = v;              // its n1
    }
    if (kd.fastn) kd.fastn[(size_t)f * kd.Epad + v] = next0 ? 1 : 0;
    if (kd.ndist) {
#pragma unroll
        for (int j = 1; j < (D1 < kNdistAxes ? D1 : kNdistAxes); ++j) {
            int m = dist[j];
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) m = max(m, __shfl_xor(m, w, 64));
            // (a look first: the maximum settles after a few wavefronts, and 70 000 atomics on one address cost 2 ms)
            if ((threadIdx.x & 63) == 0 && m > __builtin_nontemporal_load(&kd.ndist[j])) atomicMax(&kd.ndist[j], m);
        }
    }
}

// offset[e] = dense id of e's vertex; the first entry of each vertex registers as its
// representative.  Ids come out in first-insertion order, exactly the reference's ids.
__global__ void __launch_bounds__(kBlock) k_offsets(KernelDev kd, const int *__restrict__ n_points)
{
    const int f = blockIdx.y;
    const int live = ((n_points[f] + 3) & ~3) * kd.D1;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= live) return;
    const size_t fe = (size_t)f * kd.Epad;
    const int *prefix = kd.prefix + (size_t)f * (kd.Epad + 1);
    const int r = kd.slot[(size_t)f * kd.cap + kd.slot_of[fe + e]];
    const int id = prefix[r];
    kd.offset[fe + e] = id;
    if (r == e) kd.rep[fe + id] = e;
}

template <int D>
__device__ __forceinline__ int find_vertex(const KernelDev &kd, int f, const int16_t (&key)[D])
{
    const unsigned mask = (unsigned)kd.cap - 1u;
    unsigned h = hash_key<D>(key) & mask;
    const int *slot = kd.slot + (size_t)f * kd.cap;
    for (;;) {
        const int r = slot[h];
        if (r == kEmpty) return -1;
        int16_t other[D];
        load_entry_key<D>(kd, f, r, other);
        bool same = true;
#pragma unroll
        for (int i = 0; i < D; ++i) same &= (other[i] == key[i]);
        if (same) return kd.prefix[(size_t)f * (kd.Epad + 1) + r];
        h = (h + 1u) & mask;
    }
}

// One thread per (axis j, vertex v): the blur neighbours, ref: :408-421.  The relation is mutual -- B = n2_j(A)
// iff A = n1_j(B) -- so one hash probe per (axis, vertex) finds n2 and fills both sides; the table was preset to
// -1 (absent) by the caller.
template <int D>
__global__ void __launch_bounds__(kBlock) k_neighbors(KernelDev kd, int F, XcdMap nb)
{
    constexpr int D1 = D + 1;
    const FrameBlock fb = frame_block(nb);
    const int f = fb.f;
    if (f >= F) return;
    const int V = kd.V[f];
    const int idx = fb.bx * kBlock + threadIdx.x;
    if (idx >= V * D1) return;
    const int j = idx / V, v = idx - j * V;
    int16_t key[D], n2[D];
    load_entry_key<D>(kd, f, kd.rep[(size_t)f * kd.Epad + v], key);
#pragma unroll
    for (int t = 0; t < D; ++t) n2[t] = (int16_t)(key[t] + 1);
#pragma unroll
    for (int t = 0; t < D; ++t)          // axis d touches only the implied last coordinate
        if (t == j) n2[t] = (int16_t)(key[t] - D);
    const int b = find_vertex<D>(kd, f, n2);
    if (b < 0) return;
    int *nbp = kd.nbr + ((size_t)f * D1 + j) * kd.Epad * 2;
    nbp[2 * v + 1] = b;                  // my n2
    nbp[2 * b] = v;                      // its n1
}

// The compact neighbour table of the sorted build (KernelDev::nbrc): per block of kNbrcBlock = 64 vertices (one wavefront) and axis
// the smallest n1 and the smallest n2, and per vertex the two 16-bit offsets from them.  Ids follow the codes, so n1 / n2 grow with v
// and a block's neighbours span about a block; should a span not fit 16 bits the pinned word is raised and the blur keeps to the
// 32-bit table.  The host does not know V yet (a grid over the CAPACITY was 0.16 ms of empty workgroups at C5 x 8): kNbrcGrid
// workgroups per (frame, axis) walk the blocks below V, four per wavefront and round with their loads issued together (one block
// per round and a workgroup-wide minimum through LDS: 156 us per 4 C5 frames).
constexpr int kNbrcGrid = 64;
__device__ __forceinline__ int wave_min(int x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = min(x, __shfl_xor(x, m, 64));
    return x;
}
__global__ void __launch_bounds__(kBlock) k_nbr_compact(KernelDev kd, int limit)          // limit: 0xffff (the instrumented library's test hook lowers it)
{
    static_assert(kNbrcBlock == 64, "one wavefront per base");
    constexpr int U = 4;
    const int f = blockIdx.z, j = blockIdx.y;
    const int V = kd.V[f];
    const size_t fj = (size_t)f * kd.D1 + j;
    const int2 *tab = reinterpret_cast<const int2 *>(kd.nbr) + fj * kd.Epad;
    unsigned *out = reinterpret_cast<unsigned *>(kd.nbrc) + fj * kd.Epad;
    int2 *base = reinterpret_cast<int2 *>(kd.nbrc_base) + fj * (kd.Epad / kNbrcBlock + 1);
    const int lane = threadIdx.x & 63, wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nwaves = kNbrcGrid * (kBlock / 64);
    for (int b0 = wave * U; b0 * kNbrcBlock < V; b0 += nwaves * U) {
        int2 n[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = (b0 + u) * kNbrcBlock + lane;
            n[u] = v < V ? tab[v] : make_int2(-1, -1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = b0 + u, v = b * kNbrcBlock + lane;
            if (b * kNbrcBlock >= V) break;
            const int m0 = wave_min(n[u].x < 0 ? INT_MAX : n[u].x), m1 = wave_min(n[u].y < 0 ? INT_MAX : n[u].y);
            const int lo0 = m0 == INT_MAX ? 0 : m0, lo1 = m1 == INT_MAX ? 0 : m1;
            if (lane == 0) base[b] = make_int2(lo0, lo1);
            if (v >= V) continue;
            const int o0 = n[u].x < 0 ? 0xffff : n[u].x - lo0, o1 = n[u].y < 0 ? 0xffff : n[u].y - lo1;
            if ((n[u].x >= 0 && o0 >= limit) || (n[u].y >= 0 && o1 >= limit)) kd.tbl_bad[0] = 1;
            out[v] = (unsigned)(o0 & 0xffff) | ((unsigned)(o1 & 0xffff) << 16);
        }
    }
}

// nbr16 = (n1 + 1) | (n2 + 1) << 16 per (axis, vertex) for frames whose ids fit 16 bits (the fused engine's table)
__global__ void __launch_bounds__(kBlock) k_neighbors16(KernelDev kd)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * kd.D1) return;
    const int j = idx / V, v = idx - j * V;
    const int2 r = reinterpret_cast<const int2 *>(kd.nbr)[((size_t)f * kd.D1 + j) * kd.Epad + v];
    kd.nbr16[((size_t)f * kd.D1 + j) * kd.Epad + v] = (unsigned)(r.x + 1) | ((unsigned)(r.y + 1) << 16);
}

// two-hop table of the pass pair (first + 2p, first + 2p + 1) for single-frame engines (KernelDev::nbr2): everything k_blur2x2 looks
// up on its way, looked up once at build time, so that a launch of two passes is a table read and ONE level of gathers
__global__ void __launch_bounds__(kBlock) k_neighbors_2hop(KernelDev kd, int first, int npairs)
{
    const int f = blockIdx.y;
    const int V = kd.V[f];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= V * npairs) return;
    const int p = idx / V, v = idx - p * V;
    const int2 *nj = reinterpret_cast<const int2 *>(kd.nbr) + ((size_t)f * kd.D1 + first + 2 * p) * kd.Epad;
    const int2 *nj1 = nj + kd.Epad;
    const int2 ab = nj1[v], nv = nj[v];
    const int2 na = ab.x >= 0 ? nj[ab.x] : make_int2(-1, -1), nb = ab.y >= 0 ? nj[ab.y] : make_int2(-1, -1);
    int4 *out = reinterpret_cast<int4 *>(kd.nbr2) + (((size_t)f * npairs + p) * kd.Epad + v) * 2;
    out[0] = make_int4(nv.x, nv.y, ab.x, ab.y);
    out[1] = make_int4(na.x, na.y, nb.x, nb.y);
}

// ---- CSR of splat contributions: vertex -> (point, weight), points ascending ------------
// The reference splats sequentially over points (:653-661), so each vertex's sum is taken
// in ascending point order; an ordered CSR walk reproduces that sum bit for bit.

__global__ void __launch_bounds__(kBlock) k_csr_count(KernelDev kd, const int *__restrict__ n_points)
{
    const int f = blockIdx.y;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_points[f] * kd.D1) return;               // real points only
    atomicAdd(&kd.flag[(size_t)f * (kd.Epad + 1) + kd.offset[(size_t)f * kd.Epad + e]], 1);
}

// rowmax[f] = longest CSR row of the frame (lets the fused engine pick its splat strategy): one atomic per workgroup.
__global__ void __launch_bounds__(kBlock) k_row_max(KernelDev kd)
{
    __shared__ int wave_max[kBlock / 64];
    const int f = blockIdx.y;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const int *rp = kd.rowptr + (size_t)f * (kd.Epad + 1);
    int m = v < kd.V[f] ? rp[v + 1] - rp[v] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = max(m, wave_max[w]);
        if (m > 0) atomicMax(&kd.rowmax[f], m);
    }
}

__global__ void __launch_bounds__(kBlock) k_csr_fill(KernelDev kd, const int *__restrict__ n_points)
{
    const int f = blockIdx.y;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_points[f] * kd.D1) return;
    const size_t f1 = (size_t)f * (kd.Epad + 1);
    const int v = kd.offset[(size_t)f * kd.Epad + e];
    const int k = atomicSub(&kd.flag[f1 + v], 1) - 1;   // counts run down to zero
    // rows are ordered by ORIGINAL point index whatever the internal order of the points: list the entry under its original id
    int oe = e;
    if (kd.perm) {
        const int pt = e / kd.D1;
        oe = kd.perm[(size_t)f * kd.maxNpad + pt] * kd.D1 + (e - pt * kd.D1);
    }
    kd.slot_of[(size_t)f * kd.Epad + kd.rowptr[f1 + v] + k] = oe;   // slot_of reused: unsorted rows
}

// entry id in the internal order of an entry listed under its original id
__device__ __forceinline__ int internal_entry(const KernelDev &kd, int f, int oe)
{
    if (!kd.iperm) return oe;
    const int pt = oe / kd.D1;
    return kd.iperm[(size_t)f * kd.maxNpad + pt] * kd.D1 + (oe - pt * kd.D1);
}

// Rows come out of k_csr_fill in arrival order; the splat needs them in ascending entry order.  Short rows (the
// common case: a vertex holds a handful of contributions): every entry counts the smaller entries of its row.
// That is quadratic in the row length, so rows longer than kLongRow (clustered or identical features put tens of
// thousands of entries on one vertex) are only listed here and sorted by k_csr_sort_long, one workgroup per row.
constexpr int kLongRow = 128;

__global__ void __launch_bounds__(kBlock) k_csr_order(KernelDev kd, const int *__restrict__ n_points)
{
    const int f = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_points[f] * kd.D1) return;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int *rows = kd.slot_of + fe;
    const int e = rows[p];                               // (original id: what the row is ordered by)
    const int ei = internal_entry(kd, f, e);
    const int v = kd.offset[fe + ei];
    const int s = kd.rowptr[f1 + v], t = kd.rowptr[f1 + v + 1];
    if (t - s > kLongRow) {                              // flag[] is all zero again after k_csr_fill: reuse it as the list of
        if (p == s) kd.flag[f1 + atomicAdd(&kd.flag[f1 + kd.Epad], 1)] = v;   // long rows, its last slot as their count
        return;
    }
    int rank = 0;
    for (int q = s; q < t; ++q) rank += (rows[q] < e);
    csr_emit(kd, fe, s + rank, ei, v);
}

// One workgroup per long row: bitonic sort of the row's entry ids in place (global memory, the row belongs to this
// workgroup alone), O(n log^2 n) compare-exchanges instead of n^2 compares.
__global__ void __launch_bounds__(kBlock) k_csr_sort_long(KernelDev kd, const int *__restrict__ sort_plan, int *__restrict__ bstat)
{
    const int f = blockIdx.y;
    const size_t fe = (size_t)f * kd.Epad, f1 = (size_t)f * (kd.Epad + 1);
    const int nlong = kd.flag[f1 + kd.Epad];
    int *rows = kd.slot_of + fe;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // report only: the hash build's long rows and, in locality mode, what the point sort counted (the sorted build's counters do
        // not apply to these lattices: the host reports them as 0)
        int *st = bstat + (size_t)f * kBuildStats;
        st[kBsLongRows] = nlong;
        st[kBsPtOver64] = sort_plan ? sort_plan[(size_t)f * kSortPlan + 3 * kMaxD] : 0;
        st[kBsPtLargest] = sort_plan ? sort_plan[(size_t)f * kSortPlan + 3 * kMaxD + 1] : 0;
    }
    for (int li = blockIdx.x; li < nlong; li += gridDim.x) {
        const int v = kd.flag[f1 + li];
        const int s = kd.rowptr[f1 + v], n = kd.rowptr[f1 + v + 1] - s;
        int *r = rows + s;
        int np2 = 1;
        while (np2 < n) np2 <<= 1;
        // every compare-exchange orders its pair ascending (first step of a merge: partner = mirror image inside the
        // block of k, then half-cleaners), so the virtual +infinity elements behind n never have to move
        for (int k = 2; k <= np2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < np2; i += kBlock) {
                    const int l = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);
                    if (l > i && l < n) {
                        const int a = r[i], b = r[l];
                        if (a > b) { r[i] = b; r[l] = a; }
                    }
                }
                __syncthreads();
            }
        }
        for (int i = threadIdx.x; i < n; i += kBlock) csr_emit(kd, fe, s + i, internal_entry(kd, f, r[i]), v);
        __syncthreads();
    }
}

// the list of long rows, once per build
__global__ void __launch_bounds__(kBlock) k_long_rows(KernelDev kd)
{
    const int f = blockIdx.y;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= kd.V[f]) return;
    const size_t f1 = (size_t)f * (kd.Epad + 1);
    if (kd.rowptr[f1 + v + 1] - kd.rowptr[f1 + v] <= kLongRowMin) return;
    const int i = atomicAdd(&kd.longcnt[f], 1);
    if (i < kLongRowCap) kd.longrow[(size_t)f * kLongRowCap + i] = v;
}

template <int D>
void build_kernel_d(const KernelDev &kd, const CrfDev &c, hipStream_t s, const SortScratch *vsort, int *bstat)
{
    const int F = c.F, D1 = D + 1;
    const dim3 ge = grid_for(kd.Epad, F);
    if (vsort && kd.vorder) {
        // the sorted build (locality mode): entries sorted by the row-major code of their vertex
        const SortScratch &ss = *vsort;
        const int nbk = (1 << ss.vbits) + 1;
        // (rowmax: the count of long buckets, until k_row_max; behind it the build's counters of the F frames, cleared along)
        (void)hipMemsetAsync(kd.rowmax, 0, ((size_t)(bstat - kd.rowmax) + (size_t)F * kBuildStats) * sizeof(int), s);
        k_points<D, true><<<grid_for(kd.maxNpad, F), kBlock, 0, s>>>(kd, c.n_points, ss.vpartial, ss.vbad);
        k_vsort_plan<<<F, kBlock, 0, s>>>(D, (int)grid_for(kd.maxNpad, F).x, ss, bstat);
        (void)hipMemsetAsync(ss.vhist, 0, (size_t)F * nbk * sizeof(int), s);
        k_ecode<D><<<ge, kBlock, 0, s>>>(kd, c.n_points, ss);
        scan_frames(ss.vhist, ss.vstart, nbk, nbk, nullptr, ss.vtiles, F, s);
        k_escatter<<<ge, kBlock, 0, s>>>(kd, c.n_points, ss);
        k_eorder<<<ge, kBlock, 0, s>>>(kd, c.n_points, ss);
        k_esort_long<<<dim3(64, F), kBlock, 0, s>>>(kd, ss, bstat);
        (void)hipMemsetAsync(ss.vph, 0, (size_t)F * kVPh * sizeof(int), s);
        k_eflag<<<grid_for(kd.Epad + 1, F), kBlock, 0, s>>>(kd, c.n_points, ss);
        scan_frames(kd.flag, kd.prefix, kd.Epad + 1, kd.Epad + 1, kd.V, kd.rep, F, s); // (rep: the original ids are no longer needed, k_eoffsets rewrites it)
        k_eoffsets<<<ge, kBlock, 0, s>>>(kd, c.n_points, ss, bstat);
        (void)hipMemsetAsync(kd.nbr, 0xff, (size_t)F * D1 * kd.Epad * 2 * sizeof(int), s);      // every neighbour absent (-1)
        k_ebucket_vertices<<<grid_for(nbk, F), kBlock, 0, s>>>(kd, ss);
        XcdMap nb;
        const dim3 g = grid_xcd((long)kd.Epad, F, &nb);
        if (kd.ndist) (void)hipMemsetAsync(kd.ndist, 0, kNdistAxes * sizeof(int), s);
        if (kd.nearoff) (void)hipMemsetAsync(kd.nearoff, 0, (size_t)F * 2 * kd.Epad * 2, s);
        k_eneighbors<D><<<g, kBlock, 0, s>>>(kd, F, nb, ss);
        if (kd.nbrc && F >= kNbrcMinFrames && F <= kNbrcMaxFrames) {
            int limit = 0xffff;
#if LCCRF_INSTRUMENT
            if (const char *e = ab_env("LCCRF_NBRC_SPAN")) limit = std::min(std::max(atoi(e), 1), 0xffff);   // test hook: spans the table "cannot" hold
#endif
            k_nbr_compact<<<dim3(kNbrcGrid, D1, F), kBlock, 0, s>>>(kd, limit);
        }
    } else {
        (void)hipMemsetAsync(kd.slot, 0xff, (size_t)F * kd.cap * sizeof(int), s);
        k_points<D, false><<<grid_for(kd.maxNpad, F), kBlock, 0, s>>>(kd, c.n_points, nullptr, nullptr);
        {
            XcdMap nb;
            const dim3 g = grid_xcd(kd.Epad, F, &nb);
            k_insert<D><<<g, kBlock, 0, s>>>(kd, c.n_points, F, nb);
        }
        k_first_flag<<<grid_for(kd.Epad + 1, F), kBlock, 0, s>>>(kd, c.n_points);
        scan_frames(kd.flag, kd.prefix, kd.Epad + 1, kd.Epad + 1, kd.V, kd.rep, F, s); // (rep is written later, by k_offsets: free scratch)
        k_offsets<<<ge, kBlock, 0, s>>>(kd, c.n_points);
        (void)hipMemsetAsync(kd.nbr, 0xff, (size_t)F * D1 * kd.Epad * 2 * sizeof(int), s);      // every neighbour absent (-1)
        XcdMap nb;
        const dim3 g = grid_xcd((long)kd.Epad * D1, F, &nb);
        k_neighbors<D><<<g, kBlock, 0, s>>>(kd, F, nb);
    }
    if (kd.Epad < 65535) k_neighbors16<<<grid_for((long)kd.Epad * D1, F), kBlock, 0, s>>>(kd);
    if (kd.nbr2) {
        const int first = (vsort && kd.vorder && kd.tbl_bad) ? 1 : 0;     // the sorted build's splat takes pass 0 along (KernelDev::nbr2_first)
        const int npairs = (D1 - first) / 2;
        if (npairs > 0) k_neighbors_2hop<<<grid_for((long)kd.Epad * npairs, F), kBlock, 0, s>>>(kd, first, npairs);
    }
    if (!(vsort && kd.vorder)) {
        // CSR (the sorted build's runs are the rows already)
        (void)hipMemsetAsync(kd.flag, 0, (size_t)F * (kd.Epad + 1) * sizeof(int), s);
        k_csr_count<<<grid_for(kd.Epad, F), kBlock, 0, s>>>(kd, c.n_points);
        scan_frames(kd.flag, kd.rowptr, kd.Epad + 1, kd.Epad + 1, nullptr, kd.csr_pos, F, s);   // (csr_pos is written later, by k_csr_order)
        k_csr_fill<<<grid_for(kd.Epad, F), kBlock, 0, s>>>(kd, c.n_points);
        k_csr_order<<<grid_for(kd.Epad, F), kBlock, 0, s>>>(kd, c.n_points);
        k_csr_sort_long<<<dim3(64, F), kBlock, 0, s>>>(kd, vsort ? vsort->plan : nullptr, bstat);   // rows of more than kLongRow entries, if any
    }
    (void)hipMemsetAsync(kd.rowmax, 0, (size_t)F * sizeof(int), s);
    if (kd.Epad < 65535) k_row_max<<<grid_for(kd.Epad, F), kBlock, 0, s>>>(kd);   // only the one-workgroup engines ask (u16 ids)
    if (kd.longrow) {
        (void)hipMemsetAsync(kd.longcnt, 0, (size_t)F * sizeof(int), s);
        k_long_rows<<<grid_for(kd.Epad, F), kBlock, 0, s>>>(kd);
    }
}

}  // namespace

void launch_build_kernel(const KernelDev &kd, const CrfDev &c, hipStream_t s, const SortScratch *vsort, int *bstat)
{
    with_dims<1, 8>(kd.d, [&](auto d) { build_kernel_d<decltype(d)::value>(kd, c, s, vsort, bstat); });
}

void launch_sort_points(const KernelDev &kd, const CrfDev &c, const SortScratch &ss, hipStream_t s)
{
    with_dims<1, 8>(kd.d, [&](auto d) { sort_points_d<decltype(d)::value>(kd, c, ss, s); });
}

}  // namespace lccrf

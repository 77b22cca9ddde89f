// engine.h -- internal structures shared by the HIP kernels and the C-ABI layer.
//
// Vocabulary follows the reference (Thirdparty/DenseCRF): a CRF over N *points*
// (keypoints) with L *labels* and K pairwise *kernels*; every kernel owns a
// permutohedral *lattice* with V *vertices*; a point touches d+1 vertices, one per
// *remainder*; the pair (point, remainder) is an *entry* e = point*(d+1)+remainder.
// A *frame* is one independent CRF; a batch holds F frames with a common stride.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

#include "../../include/lccrf.h"

#ifndef LCCRF_INSTRUMENT
#define LCCRF_INSTRUMENT 0
#endif

namespace lccrf {

// A/B, cross-check and fault-injection switches -- environment variables that choose between code paths with identical results --
// exist in the INSTRUMENTED library only (`make INSTRUMENT=1` -> liblccrf_hip_instr.so, which tests and scripts load through
// LCCRF_LIB).  The release library reads no environment variable: a tracker inherits its environment, and none of these should be
// able to change its speed.  What a deployment may legitimately choose is an option of the API (lccrf_set_option).
#if LCCRF_INSTRUMENT
inline const char *ab_env(const char *name) { return getenv(name); }
#else
inline const char *ab_env(const char *) { return nullptr; }
#endif

constexpr int kMaxD = LCCRF_MAX_DIMS;
constexpr int kEmpty = -1;

constexpr int kNdistAxes = 4;
// counters of the streaming build: [F][kBuildStats] ints in one allocation with KernelDev::rowmax, behind its Fcap ints, so that one
// clear and one copy serve both (KernelState::bstat; handed to the build's kernels beside KernelDev, which no inference kernel's
// argument list may grow by; read by nothing but lccrf_get_build_report / lccrf_batch_get_build_report)
enum BuildStat {
    kBsDirect = 0, kBsLongBuckets, kBsBitmap, kBsNetUniform, kBsNetMixed, kBsNetWide, kBsMaxPerWg, kBsPhantom, kBsEmptyRows, kBsLongRows,
    kBsPtOver64, kBsPtLargest, kBuildStats
};
constexpr int kLongRowMin = 512;    // generic (L-label) splat: rows beyond this many entries go to a workgroup of their own (KernelDev::longrow)
constexpr int kLongRowCap = 4095;   // ... as long as there are no more than this many of them per frame
constexpr int kLongRowListMinPoints = 4096;   // ... in engines for frames beyond the one-workgroup kernels' range (the lists are 16 KB per frame)
constexpr int kNbrcBlock = 64;      // vertices per base of the compact neighbour table (KernelDev::nbrc): one wavefront
constexpr int kNbrcMinFrames = 3;   // ... which is built and read with 3 to 5 frames in flight (one frame: the passes go two per launch off the
constexpr int kNbrcMaxFrames = 5;   //   two-hop table; two frames: +-0) (C5, per frame and iteration: 3 / 4 / 5 frames
                                    //   28.4 -> 26.6 / 30.0 -> 24.3 / 29.1 -> 23.7 us; 6 / 7 / 8 / 16 frames, with the table loaded
                                    //   non-temporally: +-0 / +-0 / -0.3 / -1 % -- there the pass is bound by the gathers' lines, not bytes)

// Device view of one pairwise kernel across all frames of a batch.
// All per-frame arrays are strided by the capacities below (not by the actual N / V).
struct KernelDev {
    int d, D1;            // feature dims, d+1
    int maxN;             // per-frame stride of point arrays (features, norm)
    int maxNpad;          // maxN rounded up to a multiple of 4 (phantom points, quirk Q1)
    int Epad;             // entries per frame = maxNpad * D1 (also the vertex capacity)
    int cap;              // hash capacity per frame (power of two >= 2*Epad)
    int vstride;          // per-frame stride of val0/val1 = (Epad+2)*L of the owning CRF
    int vbase;            // = 2L of the owning CRF: vertex v, label l of a width-W pass sits at
                          //   vbase + v*W + l; [0,vbase) stays zero and [vbase-W, vbase) serves as vertex -1
    float w;              // kernel weight (PottsPotential3D::w_)
    float alpha;          // 1/(1+2^-d)                     permutohedral_cpu.h:681
    float inv_dp1;        // 1.0f/(d+1)                     permutohedral_cpu.h:249
    float scale[kMaxD];   // elevation scale factors        permutohedral_cpu.h:282-285

    const float *feat;    // [F][maxN][d]      input features (already / stdev)
    int16_t *rem0;        // [F][maxNpad][d]   nearest remainder-0 lattice point (first d coords)
    uint8_t *rank;        // [F][maxNpad][d]   rank of each coordinate
    float *bary;          // [F][Epad]         barycentric weight of every entry
    int *offset;          // [F][Epad]         vertex id of every entry (reference offset_)
    int *slot;            // [F][cap]          hash slots: lowest entry id with that key, or -1
    int *slot_of;         // [F][Epad]         slot index each entry landed in
    int *flag;            // [F][Epad+1]       scratch: first-occurrence flags / row counts / unsorted rows
    int *prefix;          // [F][Epad+1]       exclusive scan of flag == dense vertex id of a first entry
    int *rep;             // [F][Epad]         vertex id -> representative (first) entry
    int *V;               // [F]               number of vertices (reference M_)
    int *rowmax;          // [F]               longest CSR row (splat contributions of one vertex)
    int *nbr;             // [F][D1][Epad][2]  blur neighbours {n1,n2} per (axis, vertex), -1 absent
    int *nbr2;            // [F][D1/2][Epad][8] or null: two-hop table of the pass pairs (2p, 2p+1) for single-frame engines (one
                          //   launch per TWO blur passes, stream_filter.hip: k_blur2x2t): {v1, v2, a, b, a1, a2, b1, b2} with
                          //   (v1, v2) = axis-2p neighbours of v, (a, b) = its axis-(2p+1) neighbours, (a1, a2) / (b1, b2) = the
                          //   axis-2p neighbours of a / b; -1 absent
    int nbr2_ok;          // the streaming build filled nbr2 for the lattices now in HBM ...
    int nbr2_first;       // ... for the pass pairs (first + 2p, first + 2p + 1): first = 1 when the splat takes pass 0 along (fast0_ok)
    // compact form of nbr for the blur passes of the streaming engine (sorted build only): with the vertices in row-major order the
    // neighbours of consecutive vertices are (nearly) consecutive, so 16-bit offsets from a base per block of kNbrcBlock vertices
    // say the same as the 32-bit ids in half the bytes (a blur pass moves 20 instead of 24 bytes per vertex)
    unsigned short *nbrc; // [F][D1][Epad][2] or null: {n1, n2} - base of the vertex's block, 0xffff = absent
    int *nbrc_base;       // [F][D1][Epad / kNbrcBlock + 1][2]: smallest n1 / n2 of the block
    int *tbl_bad;         // two pinned host words raised by the sorted build: [0] a block's neighbours span more than 16 bits (nbrc is
                          //   unusable), [1] an axis-0 neighbour is not the next / previous id (fast0_ok must not be relied on)
    int nbrc_ok;          // nbrc describes the lattices now in HBM
    int fast0_ok;         // sorted build: axis 0 is the fastest coordinate of the row-major code, so a vertex's axis-0 neighbours are
                          //   v - 1 and v + 1 or absent, and the first blur pass can ride in the splat (k_splat2<true>) ...
    uint8_t *fastn;       // [F][Epad] or null: ... which reads this instead of the table: 1 = vertex v + 1 is v's axis-0 neighbour
    // ... and the next axes' neighbours are near ids too (C5: axis 1 within ~10, axis 2 within ~100 ids; rows and planes of the sparse
    // 6-D lattice hold a few vertices each): the sorted build measures the largest id distance per axis, and when the distances of
    // axes 1 (and 2) fit a workgroup's halo those passes ride in the splat as well, on an overlapped window in LDS (k_splat2w)
    int8_t *nearoff;      // [F][2][Epad][2] or null: axes 1 and 2, {n1 - v, n2 - v} as signed bytes, 0 = absent (valid when ndist <= 127:
                          //   the window passes read 2 instead of 8 table bytes per vertex)
    int *ndist;           // [kNdistAxes] or null: largest |neighbour id - id| along axes 0 .. kNdistAxes-1 over all frames (device)
    int splat_passes;     // blur passes the splat takes along for the lattices now in HBM: 0 (none), 1 (k_splat2<true>), 2 or 3 (k_splat2w)
    int splat_halo;       // ... the halo that takes on each side of a window (1 + distance of axis 1 [+ distance of axis 2])
    int splat_block;      // ... and the window (256 / 512 / 1024 vertices: 256 lanes x 1 / 2 / 4)
    int *rowptr;          // [F][Epad+1]       CSR: vertex -> range of splat contributions
    int *longcnt;         // [F]               number of rows longer than kLongRowMin; beyond kLongRowCap = "not listed": every row in line
    int *longrow;         // [F][kLongRowCap]  ... and their vertices (any order)
    int longrow_ok;       // the list describes the lattices now in HBM (the streaming build writes it; k_build_small does not)
    int long_mode;        // two-label splat: this kernel has listed rows or rows of more than ~4 entries on average (a coarse kernel over many
                          //   points): k_splat2l (1) or k_splat2v (2: ~16 entries per row and more) + k_splat_long instead of the fused splat (set by
                          //   the host once the sizes are known)
    int *csr_pt;          // [F][Epad]         contributing point, ascending within a row
    float *csr_w;         // [F][Epad]         its barycentric weight
    int *csr_pos;         // [F][Epad]         entry -> its position in csr_pt/csr_w (inverse of the row ordering)
    // compact copies for the fused engine's prologue (frames with Epad < 65535 only; undefined otherwise)
    unsigned *pk;         // [F][Epad]         (offset + 1) | csr_pos << 16 of every real entry
    unsigned *nbr16;      // [F][D1][Epad]     (n1 + 1) | (n2 + 1) << 16 per (axis, vertex), 0 = absent
    int *V_host, *rowmax_host;   // [F] pinned host mirrors of V / rowmax written by the fused build (or null)
    float *norm;          // [F][maxN]         1/(K*1 + 1e-20)  (PottsPotential3D::norm_)
    float *val0, *val1;   // [F][vstride]      lattice values (see vbase)
    // Locality mode (large frames on the streaming engine): the points of a frame are processed in an internal order --
    // position i holds original point perm[i] -- chosen so that points of neighbouring lattice cells sit next to each
    // other; every point-indexed array above (rem0, rank, bary, offset, norm, csr_pt ...) is in that order.  Results do
    // not depend on it: CSR rows stay ordered by ORIGINAL point index (quirk Q6), vertices are matched by key.  Null = off.
    const int *perm;      // [F][maxNpad]      position -> original point (identity on the phantom lanes)
    const int *iperm;     // [F][maxNpad]      original point -> position
    // ... and the VERTICES are numbered along the lattice's own axes (round 4; stream_build.hip: the sorted build): in the basis of
    // the blur directions the lattice is the integer grid Z^d, and ids in row-major order of those coordinates make the two
    // neighbours a blur gather wants consecutive ids of another row.
    int vorder;           // the lattice is built by sorting the entries on the row-major code of their vertex (no hash table)
};

// Device view of the CRF state of a batch.
struct CrfDev {
    int F, maxN, L, K;    // maxN = per-frame STRIDE (capacity) of every point array
    int activeN;          // largest n_points of the batch when the host knows it, else maxN
    const int *n_points;  // [F]
    float *unary;         // [F][maxN][L]
    float *Q;             // [F][maxN][L]   current_
    float *next;          // [F][maxN][L]   next_
    int16_t *map;         // [F][maxN]
    unsigned long long *map_bits;   // [F][bits_stride] or null: the MAP labels of a binary CRF, one bit per point (bit i%64 of
    int bits_stride;                //   word i/64) -- the wire format of the multi-GPU label gather; bits_stride = ceil(maxN/64)
    const int *perm;      // [F][perm_stride] or null: locality mode (see KernelDev::perm); unary / Q / next of THIS view are then
    int perm_stride;      //   in permuted order and the caller un-permutes Q on the way out
};
// points per frame that sizes a launch: the largest frame when the host knows it, else the capacity
inline int active_points(const CrfDev &c) { return c.activeN > 0 ? c.activeN : c.maxN; }

// The two-label splat's plan for the lattices now in HBM (set by Engine::learn_sizes(), read by the launcher in stream_filter.hip and
// by lccrf_get_splat_plan / lccrf_batch_get_splat_plan: one rule for both, so the report cannot drift from what is launched).
// Blur passes the splat takes along: the window's (KernelDev::splat_passes), at least pass 0 with the sorted build; none for a coarse
// kernel (long_mode) or a lattice of the hash build.
inline int splat_passes_taken(const KernelDev &kd)
{
    static const bool no_sb = ab_env("LCCRF_NO_SPLAT_BLUR") != nullptr;               // A/B switch: same results either way
    return (kd.vorder && kd.fast0_ok && !no_sb && !kd.long_mode) ? (kd.splat_passes > 1 ? kd.splat_passes : 1) : 0;
}
// the window splat: a lane per vertex up to this many frames in flight (two frames 25.3 / 24.5-25.1 / 25.0-26.4 us per frame-iteration
// with the threshold at 1 / 2 / 3, three frames 20.6 / 20.7 / 21.1-21.5: notes/r4_experiments.md)
constexpr int kSplatWideMaxFrames = 2;
constexpr int kSplatNarrowLanes = 256;
// ... and the instantiation k_splat2w<lanes, per_lane> of a window of 256 / 512 / 1024 vertices with F frames in flight; the grid is
// counted in workgroups of `lanes`.  Many frames in flight: 256 lanes x 1 / 2 / 4 vertices (C5 x 8, window 1024: 20.6 -> 18.9 us per
// frame-iteration against 1024 lanes x 1: workgroups of four wavefronts wait less at the barriers); one or two frames: one or two
// vertices per lane (a lane's four row walks in a row cost a single frame 33.3 -> 36.1).  One frame, window 1024: 663 workgroups of
// 1024 lanes are 1.3 rounds of the chip's 512 slots; 512 lanes x 2 vertices all run at once (33.6 -> 32.5 us).
struct SplatShape { int lanes, per_lane; };
inline SplatShape splat_window_shape(int window, int F)
{
    const int lanes = F > kSplatWideMaxFrames ? kSplatNarrowLanes : (window == 1024 && F == 1) ? 512 : window;
    return SplatShape{lanes, window / lanes};
}
inline void report_splat_plan(const KernelDev &kd, int F, lccrf_splat_plan *out)
{
    const int j0 = splat_passes_taken(kd);
    *out = lccrf_splat_plan{j0, j0 >= 2 ? kd.splat_halo : j0, 0, 0, 0, kd.long_mode};      // (pass 0 alone: one vertex either side)
    if (j0 >= 2) {
        const SplatShape sh = splat_window_shape(kd.splat_block, F);
        out->window = kd.splat_block;
        out->lanes = sh.lanes;
        out->vertices_per_lane = sh.per_lane;
    }
}

// The two-label step's BLUR plan: which way each of the d + 1 blur passes of a term goes, for the lattices now in HBM and F frames in
// flight with at most maxV vertices each.  launch_step_stream (stream_filter.hip) launches from it and lccrf_get_blur_plan /
// lccrf_batch_get_blur_plan report it: one rule for both, so the report cannot drift from what is launched.  Same bits on every route.
constexpr int kSliceBlurMaxFrames = 1;       // the last blur pass inside the slice (k_slice2<D1, true>) when passes go one per launch, up to this many frames in flight (with the sorted build: two frames +2 % without it, four and eight +-0)
constexpr int kPairFuseMaxFrames = 1;        // two passes per launch (measured: one C5 frame 52.5 -> 45.2 us per iteration; two or four frames in flight: +-0)
// ... or, whatever the number of frames, when the launch is SMALL: up to ~0.7 M vertices over all frames (one C5 frame: 0.59 M; two: +-0)
// the passes are launch- and latency-bound, e.g. 8 frames of 5000 points (30 000 vertices each): 9 launches of ~3.8 us per iteration
constexpr long kPairFuseMaxVertices = 700000;
// (a pass alone reads its table non-temporally: C5 with 5 / 6 / 7 frames in flight 23.7 -> 26.1 / 26.9 -> 25.7 / 27.0 -> 24.8 us per frame and iteration)
constexpr int kBlurNtMinFrames = 6;
static_assert(kNbrcMaxFrames < kBlurNtMinFrames, "the compact table is never read non-temporally: k_blur2c has no such form");
// the A/B switches of the instrumented library that bear on the plan: same results either way
struct BlurSwitches { bool no_pair_fuse, no_2hop_table, no_compact_nbr; };
inline const BlurSwitches &blur_switches()
{
    static const BlurSwitches sw{ab_env("LCCRF_NO_PAIR_FUSE") != nullptr, ab_env("LCCRF_NO_2HOP_TABLE") != nullptr,
                                 ab_env("LCCRF_NO_COMPACT_NBR") != nullptr};
    return sw;
}
inline bool pair_fuse(int F, int maxV)
{
    if (blur_switches().no_pair_fuse) return false;
    return F <= kPairFuseMaxFrames || (long)F * maxV <= kPairFuseMaxVertices;
}
// a pass with a launch of its own: off the compact table (sorted build, kNbrcMinFrames..kNbrcMaxFrames frames) or the 32-bit one ...
inline bool blur_alone_compact(const KernelDev &kd) { return kd.nbrc && kd.nbrc_ok && !blur_switches().no_compact_nbr; }
// ... which is then loaded non-temporally from this many frames on
inline bool blur_alone_nontemporal(int F) { return F >= kBlurNtMinFrames; }
enum BlurRoute : unsigned char {
    kBlurInSplat,         // rides in the splat (splat_passes_taken)
    kBlurPairTable,       // one of two passes in one launch off the two-hop table (k_blur2x2t)
    kBlurPairPlain,       // ... without a table (k_blur2x2)
    kBlurAlone32,         // a launch of its own on 32-bit ids (k_blur2<NT>)
    kBlurAloneCompact,    // ... on the compact table (k_blur2c)
    kBlurInSlice          // the last pass, inside the slice (k_slice2<D1, true>)
};
struct BlurPlan {
    unsigned char route[kMaxD + 1];   // of pass j < D1
    int table_pair[kMaxD + 1];        // kBlurPairTable, first pass of the pair: its index in KernelDev::nbr2
    int table_pairs;                  // pairs the table holds per frame (the stride k_blur2x2t is given)
    bool nontemporal;                 // the passes alone on 32-bit ids load their table non-temporally
    lccrf_blur_plan counts;
};
inline BlurPlan blur_plan(const KernelDev &kd, int F, int maxV)
{
    BlurPlan p{};
    const int D1 = kd.D1, j0 = splat_passes_taken(kd);
    const bool pairs = pair_fuse(F, maxV);
    // the pass left over by the pairs rides in the slice; with a few frames in flight (one pass per launch) the last pass does
    // (j0 == d + 1: a 2-D lattice's three passes can all ride in the splat)
    const bool in_slice = D1 <= 9 && j0 < D1 && (pairs ? ((D1 - j0) & 1) && D1 >= 3 : F <= kSliceBlurMaxFrames);
    const int n_own = in_slice ? D1 - 1 : D1;                                      // blur passes with a launch of their own end here
    const bool table = kd.nbr2 && kd.nbr2_ok && !blur_switches().no_2hop_table;
    const bool compact = blur_alone_compact(kd);
    lccrf_blur_plan &c = p.counts;
    c.first_table_pair = -1;
    p.table_pairs = (D1 - kd.nbr2_first) / 2;
    for (int j = 0; j < j0; ++j) p.route[j] = kBlurInSplat;
    c.in_splat = j0;
    for (int j = j0; j < n_own;) {
        if (pairs && j + 1 < n_own) {             // two passes per launch
            const int jt = j - kd.nbr2_first;     // the table holds the pairs (first, first + 1), (first + 2, first + 3) ...
            const bool t = table && jt >= 0 && !(jt & 1);
            p.route[j] = p.route[j + 1] = t ? kBlurPairTable : kBlurPairPlain;
            p.table_pair[j] = t ? jt / 2 : -1;
            if (t && c.first_table_pair < 0) c.first_table_pair = jt / 2;
            (t ? c.paired_table : c.paired_plain) += 2;
            j += 2;
        } else {
            p.route[j] = compact ? kBlurAloneCompact : kBlurAlone32;
            (compact ? c.alone_compact : c.alone_32bit) += 1;
            j += 1;
        }
    }
    if (in_slice) {
        p.route[D1 - 1] = kBlurInSlice;
        c.in_slice = 1;
    }
    p.nontemporal = blur_alone_nontemporal(F);
    c.nontemporal = c.alone_32bit > 0 && p.nontemporal;
    return p;
}

// scratch of the point sort (locality mode), owned by the engine
constexpr int kSortPlan = 3 * kMaxD + 2;
struct SortScratch {
    int bits;             // bucket bits of the counting sort (8..16)
    int rm_points;        // order the points row-major over their cells in the lattice's own basis (with the sorted build) instead of along a Z-order curve
    int *cells;           // [F][maxNpad][kMaxD] lattice cell of every point (int32); later the unordered buckets
    int *partial;         // [F][ceil(maxNpad/256)][2*kMaxD] per-workgroup min / max of the cells
    int *plan;            // [F][kSortPlan]      per dimension: lowest cell, span, code bits; then what k_sort_place counted (report only):
                          //                       buckets of more than 64 points, the largest bucket
    int *code;            // [F][maxNpad]        Z-order bucket of every point
    int *hist;            // [F][2^bits + 1]     bucket counts
    int *start;           // [F][2^bits + 1]     exclusive scan of hist, advanced to the bucket ends by the scatter
    int *tiles;           // [F][ceil((2^bits+1)/4096)] scan scratch
    int *perm, *iperm;    // [F][maxNpad]        the result
    // vertex order (per kernel, one after the other on the engine's stream)
    int vcap;                   // entries per frame the arrays below are sized for (>= Epad of every kernel)
    int vbits;                  // bucket bits of the entry sort (<= 21): ~4 buckets per entry
    unsigned long long *vcode;  // [F][vcap]           row-major code of every ENTRY's vertex
    unsigned long long *vkey;   // [F][vcap]           ... of every vertex, by id (ids are in code order bucket by bucket)
    int *vph;                   // [F][64]             positions of the phantom points' entries in the sorted order: count, then the list
    int *vbad;                  // pinned host word: raised when a frame's code space overflows 62 bits (the host then rebuilds with the hash)
    int *vhist, *vstart;        // [F][2^vbits + 1]    bucket counts, their scan (advanced to the bucket ends by the scatter)
    int *vtiles;                // [F][ceil((2^vbits+1)/4096)] scan scratch
    int *vpartial;              // [F][ceil(maxNpad/256)][2*kMaxD] per-workgroup min / max of the vertices' grid coordinates (k_points)
    long long *vplan;           // [F][2*kMaxD+3]      per dimension: lowest coordinate, stride; then bucket scale, usable, range
};

// ---- streaming engine (any size; every array in HBM) ---------------------------------
// locality mode: Z-order buckets of the points' lattice cells under kernel kd -> ss.perm / ss.iperm
void launch_sort_points(const KernelDev &kd, const CrfDev &c, const SortScratch &ss, hipStream_t s);
// dst[f][i][0..width) = src[f][perm[i]][0..width) (gather = 1) or dst[f][perm[i]][..] = src[f][i][..] (gather = 0), i < n_points[f]
void launch_permute_rows(const CrfDev &c, float *dst, const float *src, int width, int gather, hipStream_t s);
// bstat: [F][kBuildStats] behind kd.rowmax's capacity (BuildStat above), never null
void launch_build_kernel(const KernelDev &kd, const CrfDev &c, hipStream_t s, const SortScratch *vsort, int *bstat);
void launch_norm(const KernelDev &kd, const CrfDev &c, int maxV, hipStream_t s);
// unary[i][:] from labels (densecrf3d.h:116-129); the 2L+1 energies {u, n[L], p[L]} are passed by value (no table
// upload; `label` may be device or pinned host memory)
struct UnaryTable { float v[2 * LCCRF_MAX_LABELS + 1]; };
// codes / pairs (two labels; both or neither): see LabelCodes below -- written by the same launch, the codes in the unary array's order
void launch_unary_from_label_tbl(const CrfDev &c, const int16_t *label, const UnaryTable &tbl, hipStream_t s,
                                 unsigned char *codes = nullptr, float *pairs = nullptr);
void launch_start(const CrfDev &c, hipStream_t s);
// compat (include/lccrf.h section 1e; null: every term is Potts): K device pointers, compat[k] the [L][L] label-compatibility matrix
// of term k or null.  The batch paths pass null.
// pre (include/lccrf.h section 1g; null: every term is normalised AFTER the filter, as the reference's): K device pointers, pre[k]
// the [F][maxN] factor of term k's filter INPUT (its norm, or the square root of it) or null.  A non-null `pre` says that some term
// of the CRF is not normalised AFTER: the step then takes the general L-label branch at L = 2 as well, and `kds` are the caller's
// copies whose `norm` points at each term's factor behind the filter (the norm, its square root, or ones).  The batch paths pass null.
void launch_step_stream(const CrfDev &c, const KernelDev *kds, const int *maxV, float relax,
                        hipStream_t s, const float *const *compat = nullptr, const float *const *pre = nullptr);
// section 1g's per-point factors, out [F][maxN]: sqrtf(norm) of the frame's points (root = 1; correctly rounded), or 1.0f everywhere
void launch_norm_factor(const CrfDev &c, const float *norm, float *out, int root, hipStream_t s);
// the generic splat with its input rows multiplied by pre [F][kd.maxN] where they are loaded (stream_scaled.hip; in != null)
void launch_splat_scaled(const KernelDev &kd, const float *in, int in_stride, int L, int F, int maxV, const float *pre, hipStream_t s);
void launch_map(const CrfDev &c, hipStream_t s);
void launch_map_of(const CrfDev &c, const float *prob, int16_t *map, hipStream_t s);
void launch_exp_and_normalize(const CrfDev &c, const float *in, float *out, float scale, float relax, hipStream_t s);
void launch_step_init(const CrfDev &c, float *out, hipStream_t s);
// reverse = 1: the blur passes in reverse axis order (d .. 0) -- the TRANSPOSED filter alpha S^T B_0 .. B_d S of the one the
// forward applies (alpha S^T B_d .. B_0 S; every pass is symmetric, their product is not).  `out` may be `in` (the splat reads it first).
// blurred (optional): receives the kernel's value buffer (val0 or val1) that the slice read -- (B S in)[v][l] at
// [f * vstride + vbase + v * L + l], valid until the kernel's next splat (the feature gradient's corner dots read it there)
// compat (accumulate = 1 only): the term's [L][L] label-compatibility matrix or null -- out += w * norm * (compute(in) mu^T)
// pre: the [F][maxN] factor of the input rows or null (section 1g) -- compute(pre . in), formed inside the splat
void launch_filter(const KernelDev &kd, const CrfDev &c, int maxV, const float *in, float *out, int accumulate, hipStream_t s,
                   int reverse = 0, const float **blurred = nullptr, const float *compat = nullptr, const float *pre = nullptr);
// the same for a value width of 1 and without the slice: in [F][in_stride] (null: all ones, the normalisation's input); returns
// the blurred values, (B S in)[v] at [f * vstride + vbase + v]
const float *launch_filter_values1(const KernelDev &kd, const CrfDev &c, int maxV, const float *in, int in_stride, hipStream_t s,
                                   int reverse);
hipError_t time_blur_pass(const KernelDev &kd, int F, int maxV, int L, int reps, hipStream_t s, float *ms_per_launch);
// object API, device inputs (device_inputs.hip): dst[i][0..d) for i < n from a caller's [n][d] array (copy), from the pixel position
// (x, y) / posdev of point i = y * width + x (position), or from that plus an RGB pixel [n][3] / featuredev (uint8 or float image)
enum { kStageCopy = 0, kStagePosition = 1, kStageImageU8 = 2, kStageImageF32 = 3 };
void launch_stage_features(float *dst, const void *src, int n, int d, int mode, int width, float posdev, float featuredev,
                           hipStream_t s);
// out[f] = clamp(in[f], 0, maxN); *bad (pinned host memory) is set to 1 if anything had to be clamped
void launch_validate_npoints(const int *in, int *out, int F, int maxN, int *bad, hipStream_t s);

// ---- mean-field backward (csrc/meanfield_backward.hip; include/lccrf.h sections 1c - 1f and 2c - 2d) ------------------------
// One backward call, of a handle or of a batch (F frames of up to `rows` points; a handle is a batch of one): what every
// lccrf_*inference_backward* entry point fills in and hands to the one path behind them (api_backward.hip: backward_call).
struct BackwardRequest {           // (an aggregate: the members left out of a braced list are null / false)
    int T;                          // n_iterations
    float relax;
    const float *grad_prob;         // [F][rows][L] dL/dQ_T
    float *grad_unary;              // [F][rows][L] or null: dL/dU is then formed in the area (BackwardArea::gU)
    float *grad_weights;            // [F][K] or null
    float *const *grad_features;    // null, or K pointers, [F][rows][d_k] each or null (sections 1d / 2d)
    float *grad_compat;             // [F][K][L][L] or null (sections 1e / 1f: F = 1; section 2h)
    bool compat_form;               // the sweep takes section 1e's form: the terms' matrices are honoured (grad_compat needs it)
    float *grad_model;              // [K + K*L*L] or null (section 2h): the sums over the frames of dL/dw and dL/dmu (needs compat_form)
    // [F] int32 on the device or null (section 2j): frame f is differentiated at t_f = min(max(counts[f], 0), T) iterations, T the cap
    // every [T] part of the area is sized by; the kernels clamp, the host never reads the array.  With grad_compat /
    // grad_model it is section 2k, with grad_features section 2l.
    const int *counts;
};
// The area of one backward call, owned by the engine and zeroed when allocated: Q_0 .. Q_{T-1} of the replay, one [F][.][L] array
// per term, dL/dQ_t, the per-workgroup partials of the weight gradient, and the parts the request asks for beyond those.  Every
// [slice] array is `slice` floats: for a handle backward_stride(N, L) (N rounded up to a multiple of 4 rows, the phantom points'
// rows of quirk Q1 staying zero), for a batch F * maxN * L (the engine's own [F][maxN][L] layout).  The sweep reads no row at or
// beyond a frame's n_points (meanfield_backward.hip).  backward_layout() is the one place that knows the order and the sizes.
struct BackwardArea {
    size_t slice;         // floats per array
    float *hist;          // [T][slice]
    float *phi;           // [K][slice]
    float *G;             // [slice]
    float *partial;       // [max(T,1)][K][F][max(backward_blocks(rows, L), 1)]
    float *gU;            // [slice] when the request has no grad_unary, else null
    // the feature part (sections 1d and 2d), per term whose feature gradient is asked for, else null: dL/d(corner weight) of every
    // entry, laid out as KernelDev::bary, and right behind it the per-point sum behind the norm's gradient -- feat_floats in all,
    // zeroed by the caller (from gb on) before every sweep
    float *gb[LCCRF_MAX_KERNELS];   // [F][Epad]
    float *gn[LCCRF_MAX_KERNELS];   // [F][maxNpad]
    size_t feat_floats[LCCRF_MAX_KERNELS];
    // the compatibility part (section 1e), with BackwardRequest::compat_form, else null: gamma_t of the current iteration, and the
    // per-workgroup partials of dL/dmu accumulated over the iterations
    float *gam;           // [slice]
    float *cpart;         // [K][F][backward_compat_blocks(rows)][L][L]
    // the per-frame values behind the request's grad_model where the caller left their own array out (section 2h), else null
    float *gW;            // [F][K]
    float *gC;            // [F][K][L][L]
};
int backward_blocks(int n, int L);
size_t backward_stride(int n, int L);
int backward_compat_blocks(int n);
// The chunks a frame of n points is cut into for the partials of dL/dmu (section 1e): one per 256 rows, at least 1, at most 128 --
// backward_compat_blocks(n), the grid of a handle of n points.  A chunk is ceil(n / chunks) consecutive rows.
constexpr int kCompatMaxBlocks = 128;
__host__ __device__ inline int compat_chunks(int n)
{
    const int b = (n + 255) / 256;
    return b < 1 ? 1 : b > kCompatMaxBlocks ? kCompatMaxBlocks : b;
}
// The area of request `rq` on c.F frames of up to `rows` points: returns its size in bytes and, with ar != null, sets *ar to
// its parts in the area at `base` (sizing: both null).  Sizing and running go through this one function.
size_t backward_layout(const BackwardRequest &rq, const CrfDev &c, const KernelDev *kds, size_t slice, int rows, float *base,
                       BackwardArea *ar);
// the reverse sweep over the F = c.F frames of up to `rows` points each (the replay has filled ar.hist and ar.G = dL/dQ_T):
// dL/dU [F][c.maxN][L] goes to rq.grad_unary, or ar.gU without one (rows [n_points[f], rows) written 0), rq.grad_weights and
// rq.grad_features (rows [n_points[f], rows) written 0; the caller has zeroed ar.gb / ar.gn of every term asked for) as the
// request says.  Without feature gradients and compat_form the launches are those of sections 1c / 2c.
// compat (or null): K device pointers, the terms' [L][L] matrices or null, read with rq.compat_form only -- the sweep then takes
// section 1e's form (one k_compat_bwd launch per iteration and term more) and rq.grad_compat, if given, is overwritten.
// compat_form and grad_features together are section 1f: section 1e's form plus the launches section 1d adds.
// pre (or null): as launch_step_stream takes it (section 1g) -- kds[k].norm is then a_k, the factor behind the filter, the forward
// filters of the sweep scale their input rows by pre[k] = b_k, and k_bwd_combine multiplies the transposed filter's result by it.
// With grad_features only together with `modes` (sections 1m / 2i; the other entry points refuse the combination).
// modes (or null: every term AFTER): each term's lccrf_normalization and its TRUE norm n_k -- the feature part then differentiates the
// factors too: the splat side's row is b_k . Q_{t-1}, k_bwd_combine_adjoint (in k_bwd_combine<true>'s place, the same bits in G) adds
// the pre adjoint to ar.gn[k], and the norm part forms g_n by the term's mode (none for LCCRF_NORMALIZE_NONE).
// rq.grad_model (section 2h; null for a handle: not a launch more): dL/dw and dL/dmu of every frame -- in the caller's arrays, or in
// ar.gW / ar.gC where the caller left one out -- are summed over the frames in ascending order, one k_sum_frames launch each.
// rq.counts (section 2j; null: the launches and the arithmetic above, untouched): frame f is idle while t > t_f -- its G stays the
// caller's dL/dQ, nothing is added to its dL/dU, no partial is written for it; its filters run on (phi is scratch) -- its first step
// is t == t_f, and the weight gradient's reduction walks its t_f x blocks partials: a handle's bits at t_f.  In the compat form
// (section 2k) k_compat_bwd leaves an idle frame's cpart and phi alone and writes cpart at t == t_f, and k_compat_reduce gives a frame
// with t_f = 0 exact zeros without reading its cpart, which no iteration of the call wrote.  In the feature part (section 2l) the sweep's
// k_corner_dot launches and k_bwd_combine_adjoint leave an idle frame alone -- nothing is added to its ar.gb / ar.gn -- and the norm part
// runs for every frame: at t_f = 0 on the caller's zeros, which it turns into +0 in every row of dL/df.
struct BackwardModes {
    int mode[LCCRF_MAX_KERNELS];
    const float *norm[LCCRF_MAX_KERNELS];   // [F][maxN], KernelDev::norm of the engine's own views (not of step_kdevs())
};
void launch_backward_sweep(const CrfDev &c, const KernelDev *kds, const int *maxV, int rows, const BackwardRequest &rq,
                           const BackwardArea &ar, const float *const *compat, hipStream_t s, const float *const *pre = nullptr,
                           const BackwardModes *modes = nullptr);
// The replay AND the sweep of a request for dL/dU and / or dL/dw alone in ONE launch, a 1024-lane workgroup per frame
// (csrc/fused_backward.hip; include/lccrf.h section 1j): two labels, Potts terms normalised AFTER on lattices in HBM that fit the fused
// plan, frames of up to 2048 active points.  Reads rq.grad_prob itself (no copy into ar.G beforehand), keeps Q_0 .. Q_{T-1} in
// ar.hist, leaves Q_T in c.Q and writes what launch_backward_sweep would have, bit for bit.  Returns fused_report() of the shape it
// launched, or 0 with nothing launched: the frames are not ones the plan takes.
int launch_fused_backward(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows, const BackwardRequest &rq,
                          const BackwardArea &ar, hipStream_t s);
struct TermModel;
// ... and of a learnt model, or of a request in the compat form (csrc/fused_backward_general.hip; include/lccrf.h section 1k): terms
// with a matrix or a normalisation mode, dL/dU, dL/dw and dL/dmu per frame, no feature gradients.  kds: Engine::step_kdevs() (`norm` is
// each term's factor behind the filter); terms: Engine's model (matrices by value, the factors in front of the filters).  Writes
// rq.grad_unary (or ar.gU), rq.grad_weights (or ar.gW under rq.grad_model) and rq.grad_compat (or ar.gC) of every frame; the sums of
// rq.grad_model are the caller's to launch.  With rq.counts (section 2k) every frame's workgroup runs its own t_f iterations, the
// workgroups taking the frames by descending t_f (the order in ar.phi).  Returns fused_report() of the shape launched, or 0 with
// nothing launched.
int launch_fused_backward_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows,
                                  const BackwardRequest &rq, const BackwardArea &ar, const TermModel &terms, hipStream_t s);
// ... and of a request WITH feature gradients (csrc/fused_backward_features.hip; include/lccrf.h section 1l): Potts terms normalised
// AFTER, rq.T >= 1, no compat form, at least one array in rq.grad_features.  Writes what launch_fused_backward writes and
// rq.grad_features (rows [n_points[f], rows) written 0), bit for bit what launch_backward_sweep would have; ar.gb / ar.gn need no zeroing
// (the kernel's first iteration writes them).  With rq.counts (section 2l) every frame's workgroup runs its own t_f iterations, the
// workgroups taking the frames by descending t_f (the order in ar.phi); a frame with t_f = 0 gets +0 in every row of dL/df.  Returns
// fused_report() of the shape launched, or 0 with nothing launched.
int launch_fused_backward_features(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, int rows,
                                   const BackwardRequest &rq, const BackwardArea &ar, hipStream_t s);
// out[j] = sum over the frames, in ascending order, of x[f][j], j < n (section 2h; meanfield_backward.hip)
void launch_sum_frames(const float *x, int F, int n, float *out, hipStream_t s);
// Q of every frame whose count is below the cap <- hist[t_f] (section 2j: the replay steps every frame T times; Q_{t_f} is what stays)
void launch_restore_counted_q(const CrfDev &c, const BackwardArea &ar, int T, const int *counts, hipStream_t s);
// order[0 .. F) <- the frames by descending t_f = min(max(counts[f], 0), T), equal counts by ascending frame: a permutation of 0 .. F-1,
// formed on the device (section 2j: the one-launch backward hands its workgroups the longest frames first)
void launch_order_by_count(const int *counts, int F, int T, int *order, hipStream_t s);

// ---- one run, its terms, and what a converged one reports: what the launch requests below are made of ---------------------------
// One run: a fixed count of n_iter iterations, or -- until_converged -- at most n_iter under (criterion, tol) (include/lccrf.h
// sections 1h and 2e: LCCRF_STOP_* bits).
struct Schedule { int n_iter; int with_map; float relax; bool until_converged; int criterion; float tol; };
inline Schedule fixed_run(int n_iter, int with_map, float relax) { return Schedule{n_iter, with_map, relax, false, 0, 0.0f}; }
inline Schedule converged_run(int max_iter, int criterion, float tol, int with_map, float relax)
{
    return Schedule{max_iter, with_map, relax, true, criterion, tol};
}
// The terms of a CRF that are not all Potts terms normalised AFTER the filter (include/lccrf.h sections 1e, 1g and 2g).
// All null: the Potts kernels.  Filled by Engine::term_model(), which owns the arrays behind `mats` and `mats_dev`.
struct TermModel {
    const float *const *mats;      // null, or K HOST pointers: term k's [L][L] matrix or null -- the two-label kernels take the
                                   //   [2][2] ones by value (copy_matrices)
    const float *const *pre;       // null, or K device pointers: the [F][maxN] factor of term k's filter input or null (the kernels on
                                   //   lattices in HBM, whose `kds` are Engine::step_kdevs(); the one-launch ones form it themselves)
    const int *norm_mode;          // null (every term AFTER), or K lccrf_normalization values (the one-launch kernels)
    const float *const *mats_dev;  // null exactly when `mats` is, or K DEVICE pointers: term k's [L][L] matrix in HBM or null -- what
                                   //   k_multilabel_general reads (3 to 8 labels: up to 2 x 64 floats are not passed by value)
    bool general() const { return mats || pre || norm_mode; }
};
// the matrices as the general kernels' arguments carry them: mu[k] = term k's, row-major; returns has_mu (bit k: term k has one)
inline int copy_matrices(const TermModel &t, int K, float (*mu)[4])
{
    int has_mu = 0;
    for (int k = 0; k < K; ++k)
        if (t.mats && t.mats[k]) {
            has_mu |= 1 << k;
            for (int e = 0; e < 4; ++e) mu[k][e] = t.mats[k][e];
        }
    return has_mu;
}
// what a converged run reports per frame, [F] each in HBM
struct ConvergeOut {
    int *iterations;      // t
    float *delta;         // d_t
    int *changed;         // c_t
    int *converged;       // the criterion was met at t
};

// ---- fused build (SLAM sizes; one workgroup per (frame, kernel), hash table in LDS) ------
bool build_small_supported(const KernelDev *kds, int n, int max_points);
void launch_build_small(const KernelDev *kds, int n, int max_points, const CrfDev &c, hipStream_t s);

// ---- fused engine (SLAM sizes; one workgroup per frame, lattice values in LDS) --------
// the CRF both one-workgroup engines are written for: L = 2, one or two 2-D kernels (u16_tables: and Epad < 65535 in each)
bool slam_shaped(const CrfDev &c, const KernelDev *kds, bool u16_tables);
bool fused_supported(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow,
                     size_t *lds_bytes);
// The batch's prepared launch records of the two-frames-per-CU kernel (fused_lean.h: LeanPrepPlan) -- `buf` of `bytes` bytes owned
// by the caller (lean_prep_bytes(): what the current batch needs, 0 when the plan does not apply); the launch fills them when
// !valid (the caller clears `valid` whenever a lattice changes) and records ev0 / ev1 around that launch.
struct LeanPrep {
    unsigned char *buf = nullptr;
    size_t bytes = 0;
    bool valid = false, timed = false;
    unsigned long long key = 0, seen_key = 0;   // the plan / shape the blocks were written for; ... the last inference ran with (blocks are written by the second)
    unsigned runs = 0;                    // how many times the blocks were (re)written: tests
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
size_t lean_prep_bytes(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow);
// lccrf_get_engine's shape word: lanes per workgroup | points per lane << 16 | kernel 0 took the chain path << 20
inline int fused_report(int lanes, int ppt, int chain0) { return lanes | ppt << 16 | (chain0 ? 1 << 20 : 0); }
// One inference of the c.F frames of a handle (one) or a batch on lattices in HBM that fit the fused plan, in ONE launch, a workgroup
// per frame.  Which kernel: Potts terms on k_fused (fused_engine.hip: 1024 lanes, or 512 and two frames per CU) or, until converged,
// k_converge (fused_converge.hip: frames of up to 4096 active points); terms with a matrix or a factor on k_general / k_general_converge
// (fused_general.hip, fused_general_converge.hip: up to 2048 active points), whose `kds` are the caller's copies with `norm` pointing
// at each term's factor behind the filter (as launch_step_stream takes them).  The stop decision of a converged run is made inside
// the kernel; a plan that leaves no room for its reduction's words in LDS launches nothing.
// Label-derived unaries as the lean inference kernel reads them (k_fused_lean_lbl): what k_unary_from_label_tbl leaves beside the
// unary array -- a point's code in the unary array's point order, and the three pairs a code stands for.
constexpr int kLabelPairFloats = 12;
struct LabelCodes {
    const unsigned char *codes;   // [F][maxN]: 0 / 1 the label, 2 unknown or out of range; null: the unaries are not label-derived
    const float *pairs;           // [kLabelPairFloats]: by code the pair -energy, then by code the pair Q0 = softmax(-energy)
};
struct SizedRequest {
    Schedule run;
    TermModel terms;      // (norm_mode is not read: the factors are in HBM, terms.pre and kds[k].norm)
    ConvergeOut out;      // every frame's report (read only when run.until_converged)
    LeanPrep *prep;       // or null: k_fused's prepared launch records (no other kernel looks at them)
    LabelCodes lbl;       // codes == null: raw unaries (only the lean plan's run from prepared records looks at them)
};
struct SizedLaunch {
    int report;           // fused_report() of what was launched; 0: the frames are not ones the kernel takes and nothing was launched
    int shape;            // lanes per workgroup (= per frame) | workgroups per CU << 16 (k_multilabel, k_multilabel_general: | points per lane << 16)
};
// Frames of c.L = 3 .. 8 labels and a fixed count (the caller has checked the schedule) go to k_multilabel (fused_multilabel.hip: one
// 1024-lane workgroup per frame, Potts terms normalised AFTER; the caller reports engine 5) or, with rq.terms.general(), to
// k_multilabel_general (fused_multilabel_general.hip; kds: Engine::step_kdevs(); engine 6).
SizedLaunch launch_inference(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq,
                             hipStream_t s);
// Would k_multilabel take these frames?  3 .. 8 labels, one or two 2-D kernels whose tables fit the u16 records, at most the plan's
// active points for that label count, lattices that fit the two-label LDS plan (fused_multilabel.hip has the shipped range).
bool multilabel_supported(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow);
// ... and k_multilabel_general, whose shipped range is its own (fused_multilabel_general.hip)
bool multilabel_general_supported(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow);

// ---- convergence-driven inference on the streaming engine (include/lccrf.h sections 1h and 2e) ---------------------------------
// For everything the one-launch kernels do not take: the bookkeeping behind each step (converge_track.hip) -- per frame the kept
// copy of the previous Q (`prev`, [F][maxN][L] -- which IS the frame's Q at the iteration it finished, since a finished frame's
// copy is no longer refreshed), the accumulators of the iteration, and whether the frame has finished.
struct ConvergeTrack {
    float *prev;          // [F][maxN][L]
    unsigned *acc;        // [F][2]: bits of the largest |Q - prev| / flipped labels of the iteration (integer atomics: exact, order-free)
    int *done;            // [F]
    int *running;         // pinned host word: frames still running behind the last settle
    ConvergeOut out;
};
// behind launch_start: prev = Q_0, the accumulators and results zeroed, frames without points (or max_iter == 0) finished
void launch_track_begin(const CrfDev &c, const ConvergeTrack &tk, int max_iter, hipStream_t s);
// behind step t: compare and refresh the running frames, then settle each of them and count the ones still running
void launch_track_step(const CrfDev &c, const ConvergeTrack &tk, int t, int max_iter, int criterion, float tol, hipStream_t s);
// behind the last step t_last: Q = prev for the frames that finished before it
void launch_track_restore(const CrfDev &c, const ConvergeTrack &tk, int t_last, hipStream_t s);

// ---- frame engine (SLAM sizes; lattice build + normalisation + inference of a frame in ONE launch) ---------
bool frame_supported(const CrfDev &c, const KernelDev *kds);
// One run of the c.F frames from their inputs.  Which kernel: Potts terms on k_frame (frame_engine.hip, frame_lean.hip) or, until
// converged, k_frame_converge (frame_converge.hip); terms with a matrix or a mode on k_frame_general / k_frame_general_converge
// (frame_general.hip: frames of at most 2048 active points -- Engine::frame_ok -- the factors of every mode formed in the kernel from
// the norm it holds).  All but k_frame run one 1024-lane workgroup per frame and look at none of the shape options.
struct FrameRequest {
    Schedule run;
    TermModel terms;      // (pre is not read)
    int *status;          // pinned host word, zeroed by the caller: reads 1 afterwards if some frame did not fit the kernel's LDS plan
                          //   -- its lattices or, until converged, the reduction's 16 bytes behind its loop plan ...
    int *frame_status;    // device [F], or null: ... and holds 1 for exactly those frames; the caller runs them -- and only them -- on
                          //   the two-kernel path
    const int16_t *label; // != null (L = 2): the unary energies are derived in the kernel from the labels and ...
    const float *tbl5;    //   ... the 5 table entries {u, n0, n1, p0, p1}; otherwise read from c.unary
    unsigned *done;       // pinned host word or null: a single frame's kernel stores done_epoch there behind its results
    unsigned done_epoch;
    ConvergeOut out;      // every frame's report (read only when run.until_converged)
    // the shapes of k_frame
    bool allow_small;     // frames of up to 1024 points may run as 512-lane workgroups in half the CU's LDS (two frames per CU)
    unsigned *dual;       // device memory of frame_dual_bytes(F), zeroed once, or null: two-kernel frames are given two workgroups
    unsigned dual_epoch;  //   each -- one per lattice build (single frames: the other 255 CUs are idle anyway) -- under a launch-unique epoch != 0
    unsigned char *lean_rec;   // device memory of frame_lean_rec_bytes(F), or null: batches of full-size two-kernel frames (1025 .. 2048
                               //   points) may run two per CU as well (frame_lean.hip keeps the per-point records its loop re-reads there)
};
// Returns the shape it launched: 0 one frame per CU, 1 the small shape, 2 the lean one (a caller that sees many frames of a half-CU
// shape flagged turns that shape off).
int launch_frame(const CrfDev &c, const KernelDev *kds, const FrameRequest &rq, hipStream_t s);
bool frame_lean_wanted(const CrfDev &c);              // would launch_frame take the lean shape for this batch, given the area?
size_t frame_lean_rec_bytes(int frames);
size_t frame_dual_bytes(int frames);
// rows of `bytes` bytes each between a frame-strided array and a compact one: dst[i] = src[list[i]] (gather = 1) or
// dst[list[i]] = src[i] (gather = 0); strides in bytes, everything 4-byte aligned
void launch_copy_frames(void *dst, size_t dst_stride, const void *src, size_t src_stride, const int *list, int n_list,
                        size_t bytes, int gather, hipStream_t s);

// ---- unary builder (the step before the CRF) ------------------------
hipError_t run_unary_build(int device_id, int n_points, const float *Xw, const int32_t *obs_ptr, const int32_t *obs_kf,
                           const double *obs_kp, int n_kf, const float *kf_pose, const float *kf_intr,
                           const float *kf_bounds, const double *match_prob, const lccrf_crf_params *params,
                           float *observs_out, float *error_out, float *depth_out, int16_t *label_out);

// ---- BfMatch (src/Tracking.cc:1747-1766), csrc/bf_match.hip -------------------------------
hipError_t run_bf_match(int device_id, int n_query, const uint8_t *desc_query, int n_train, const uint8_t *desc_train,
                        double ratio, int32_t *train_of_query_out, int32_t *n_matches_out);

// ---- Optimizer::PoseOptimization (src/Optimizer.cc:239-450), csrc/pose_opt.hip; every pointer device-accessible ----
hipError_t launch_pose_optimization(int F, int maxN, const int *n_points, const float *Xw, const float *kp, const float *ur,
                                    const float *is2, const uint8_t *valid, const int16_t *label, const float *K4, float bf,
                                    const float *Tcw_in, float *Tcw_out, uint8_t *outlier, int *n_inliers, int *n_initial,
                                    hipStream_t s, const int *n_crf = nullptr);

}  // namespace lccrf

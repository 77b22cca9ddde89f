// fused_lean_label.hip -- the two-frames-per-CU inference kernel (fused_engine.hip: k_fused_lean, MODE 2) for label-derived unaries.
// A unit of its own: the kernels of fused_engine.hip, and their register figures, stay what they were.  DESIGN.md section 4.2.
#include "engine.h"
#include "device_math.h"
#include "fused_loop.h"
#include "fused_lean.h"
#include "fused_lean_label.h"
#include "dispatch.h"

namespace lccrf {

namespace {

using namespace fl;

// k_fused_lean<.., MODE 2> for label-derived unaries (engine.h: LabelCodes; what setUnaryEnergyFromLabel gives, the tracker's only
// call): a point's energy pair is one of three, so the prologue reads a byte per point instead of 8 -- four points' codes packed
// into one register that lives through the launch -- and takes Q0 = softmax(-unary) from the three pairs k_unary_from_label_tbl formed
// with the same arithmetic (no start_inference: 68 instructions per point); the loop forms -unary by selects from the three pairs in
// scalar registers where it is used, and re-reads no unaries (mean_field_lean<.., LBL>).  Same bits as k_fused_lean.
template <int NT, int PPT, int K, int CH, bool RELOAD>
__global__ void __launch_bounds__(NT, 4) k_fused_lean_lbl(CrfDev c, LeanLabelArgs a)
{
    constexpr int D1 = kD1;
    static_assert(PPT <= 4, "a lane's codes share one register");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = c.n_points[f];
    Instr ins{a.timing, a.timing_block, a.dbg, 0, a.timing_lane};
    FL_STAMP();

    PointRegs<PPT, K> pr;
    int V[K];
#pragma unroll
    for (int k = 0; k < K; ++k) V[k] = a.kd[k].V[f];
    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);   // (see k_fused_lean)
    auto lane_id = [&]() {
        int z = 0;
        asm volatile("" : "+v"(z));
        return wave_base + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
    };
    const FusedLayout &lay = a.lay;
    // ---- prologue from the prepared block, as k_fused_lean's: every load depends on the frame index only
    float wk[K];
    LeanSrc src;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const KernelDev &kd = a.kd[k];
        wk[k] = kd.w;
        src.nbr[k] = lean_rsrc(kd.nbr16 + (size_t)f * D1 * kd.Epad, (size_t)D1 * kd.Epad * 4);
        src.bary[k] = lean_rsrc(kd.bary + (size_t)f * kd.Epad, (size_t)kd.Epad * 4);
        src.norm[k] = lean_rsrc(kd.norm + (size_t)f * kd.maxN, (size_t)kd.maxN * 4);
        src.nbr_axis_bytes[k] = kd.Epad * 4;
        src.off_nbr[k] = src.off_bary[k] = src.off_norm[k] = 0;
    }
    src.unary = src.norm[0];                              // (never read)
    src.off_unary = 0;
    const LeanPrepPlan pp = lean_prep_plan(lay, K, a.Vcap, NT, PPT, true);
    const __amdgpu_buffer_rsrc_t rp = lean_rsrc(a.prep + (size_t)f * a.prep_stride, (size_t)a.prep_stride);
    const __amdgpu_buffer_rsrc_t rc = lean_rsrc(a.lbl.codes + (size_t)f * c.maxN, (size_t)c.maxN);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!chain_k<CH>(lay, k)) {                       // renumbered by row length: the block's table instead of the build's
            src.nbr[k] = lean_rsrc(a.prep + (size_t)f * a.prep_stride + pp.snbr_off[k], (size_t)D1 * pp.snbr_axis[k]);
            src.nbr_axis_bytes[k] = pp.snbr_axis[k];
        }
    }
    typedef unsigned lean_u2 __attribute__((ext_vector_type(2)));
    typedef unsigned lean_u4 __attribute__((ext_vector_type(4)));
    LeanLabel lb;
    const float *const tb = a.lbl.pairs;                     // (uniform: scalar loads)
    lb.n0x = tb[0], lb.n0y = tb[1], lb.n1x = tb[2], lb.n1y = tb[3], lb.n2x = tb[4], lb.n2y = tb[5];
    const float q0x = tb[6], q0y = tb[7], q1x = tb[8], q1y = tb[9], q2x = tb[10], q2y = tb[11];
    unsigned code[PPT];
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        code[s] = __builtin_amdgcn_raw_buffer_load_b8(rc, tid + s * NT, 0, 0);   // (a lane past the frame reads 0 or a stale byte: unused)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const lean_u3 w = __builtin_amdgcn_raw_buffer_load_b96(rp, tid * 12, ((s * K + k) * NT) * 12, 0);
            pr.ix[s][k][0] = w.x;
            pr.ix[s][k][1] = w.y;
            pr.ix[s][k][2] = w.z;
            // (RELOAD: the weights of the products in front of the loop; every iteration re-reads them, and w * norm with them, before
            // its X -- so the norms are not requested here)
            const lean_u3 b = __builtin_amdgcn_raw_buffer_load_b96(src.bary[k], (tid + s * NT) * (D1 * 4), 0, 0);
            pr.bary[s][k][0] = __uint_as_float(b.x);
            pr.bary[s][k][1] = __uint_as_float(b.y);
            pr.bary[s][k][2] = __uint_as_float(b.z);
            pr.wn[s][k] = RELOAD ? 0.0f : __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(src.norm[k], (tid + s * NT) * 4, 0, 0));
        }
    }
    const lean_u2 clw = __builtin_amdgcn_raw_buffer_load_b64(rp, tid * 8, pp.cl_off, 0);
    lean_u4 trow[K], tnbr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        trow[k] = tnbr[k] = lean_u4{0u, 0u, 0u, 0u};
        if (tid * 16 < pp.row_bytes[k]) trow[k] = __builtin_amdgcn_raw_buffer_load_b128(rp, tid * 16, pp.row_off[k], 0);
        if (tid * 16 < pp.nbr_bytes[k]) tnbr[k] = __builtin_amdgcn_raw_buffer_load_b128(rp, tid * 16, pp.nbr_off[k], 0);
    }
    FL_PSTAMP();                                          // (everything requested)
    if (N <= 0) {
        if (a.with_map) clear_label_bits<NT>(c, f, 0, lane_id());
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (tid * 16 < pp.row_bytes[k]) *reinterpret_cast<lean_u4 *>(smem + lay.row[k] + tid * 16) = trow[k];
        if (tid * 16 < pp.nbr_bytes[k]) *reinterpret_cast<lean_u4 *>(smem + lay.nbr[k] + tid * 16) = tnbr[k];
    }
    if (tid < 32) reinterpret_cast<float *>(smem + lay.zero)[tid] = 0.0f;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            reinterpret_cast<float2 *>(smem + lay.val[k][0])[0] = make_float2(0.f, 0.f);
            reinterpret_cast<float2 *>(smem + lay.val[k][1])[0] = make_float2(0.f, 0.f);
        }
    }
#pragma unroll
    for (int s = 0; s < PPT; ++s)
#pragma unroll
        for (int k = 0; k < K; ++k) pr.wn[s][k] = wk[k] * pr.wn[s][k];                    // pairwise3d.h:77 (w_*norm_[i]; RELOAD: unused)
    // startInference (densecrf_base.h:78-80): Q0 of the point's code
    lb.codes = 0;
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        pr.un[s] = make_float2(0.f, 0.f);                 // (never read)
        pr.q[s] = make_float2(0.f, 0.f);
        if (tid + s * NT < N) pr.q[s] = make_float2(lean_pick(code[s], q0x, q1x, q2x), lean_pick(code[s], q0y, q1y, q2y));
        lb.codes |= code[s] << (8 * s);
    }
    FL_PSTAMP();
    __syncthreads();
    FL_PSTAMP();
    ChainLane cl{clw.x, clw.y};
    FL_STAMP();
    float alpha[K];
#pragma unroll
    for (int k = 0; k < K; ++k) alpha[k] = a.kd[k].alpha;
    int t = lane_id();
    mean_field_lean<PPT, K, CH, NT, RELOAD, false, true, true>(smem, lay, V, N, t, pr, cl, alpha, wk, src, a.n_iter, a.relax, a.omr, ins, lb);
    t = lane_id();
    store_results<PPT, K, NT>(c, f, N, t, pr, a.with_map);
    FL_STAMP();
    if (kInstr && a.timing && (int)blockIdx.x == a.timing_block && t == a.timing_lane) a.timing[63] = ins.n;
}

}  // namespace

void launch_lean_label(const CrfDev &c, const LeanLabelArgs &a, int ppt, hipStream_t s)
{
    with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
        with_dims<0, 1>(a.lay.chain0 ? 1 : 0, [&](auto ch) {
            with_dims<1, 4>(ppt, [&](auto p) {
                constexpr int K = decltype(kk)::value, CH = decltype(ch)::value, P = decltype(p)::value;
                launch_workgroups(k_fused_lean_lbl<kNTSmall, P, K, CH, (P >= 3)>, c.F, kNTSmall, a.lay.total, s, c, a);
            });
        });
    });
}

}  // namespace lccrf

// fused_prologue.inc -- the fused engine's self-contained prologue: a frame's lattice tables into registers, its per-point records
// into registers, the tables into LDS, then the zero words and the two sentinel slots of every kernel.  Included as TEXT in front
// of the `__syncthreads()` of k_fused (MODE 0 / 1, fused_engine.hip), k_converge, k_general and k_general_converge -- not a header,
// and not a device function: as two shared __forceinline__ functions these lines compiled within every pinned figure and still ran
// k_converge and k_general 0.2 us slower per frame (fused_variant.h has the figures), as a kernel's own text they compile it
// instruction for instruction as the hand-kept copies did (notes/fused_general.md section 6).  The including kernel provides
//     template parameters   int PPT, int K
//     in scope              constexpr int NT, D1; the arguments `a` (with kd[]), `lay`, CrfDev c, the frame f, tid, N > 0, int V[K],
//                           PointRegs<PPT, K> pr, Instr ins, unsigned char *smem
//     declared              unsigned pk[PPT][K][D1]: (vertex id + 1) | place in the row << 16.  Filled here; k_general_converge
//                           keeps it beyond the block in which its `a` is bound
// Three places take a kernel's own lines, as macros that are empty unless the includer defines them (all three are undefined again
// at the end of this file):
//     FUSED_PROLOGUE_TERMS    behind the table loads, in front of the point records (k_general: GeneralTerms' uniform members)
//     FUSED_PROLOGUE_POINT    per point s and term k, behind the norm's load; kd and the clamped point index ic are in scope
//                             (k_general, k_general_converge: the factor in front of the filter)
//     FUSED_PROLOGUE_WORDS    behind the zero words' stores (k_converge, k_general_converge: the reduction's four words)
#ifndef FUSED_PROLOGUE_TERMS
#define FUSED_PROLOGUE_TERMS
#endif
#ifndef FUSED_PROLOGUE_POINT
#define FUSED_PROLOGUE_POINT
#endif
#ifndef FUSED_PROLOGUE_WORDS
#define FUSED_PROLOGUE_WORDS
#endif
    // All global loads of the prologue are issued before anything waits on them: the lattice
    // tables first (their LDS stores come last), then the per-point records.  Indices are clamped
    // instead of branched on, so that the loads stay back to back.
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
    FUSED_PROLOGUE_TERMS
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
            FUSED_PROLOGUE_POINT
        }
    }
    // pairwise3d.h:77 (w_*norm_[i]); with normalisation modes w * post[i]: w * n, w * sqrtf(n) or w * 1.0f (include/lccrf.h section 1g)
#pragma unroll
    for (int s = 0; s < PPT; ++s)
#pragma unroll
        for (int k = 0; k < K; ++k) pr.wn[s][k] = a.kd[k].w * pr.wn[s][k];
    FL_PSTAMP();

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
    FUSED_PROLOGUE_WORDS
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            reinterpret_cast<float2 *>(smem + lay.val[k][0])[0] = make_float2(0.f, 0.f);
            reinterpret_cast<float2 *>(smem + lay.val[k][1])[0] = make_float2(0.f, 0.f);
        }
    }
#undef FUSED_PROLOGUE_TERMS
#undef FUSED_PROLOGUE_POINT
#undef FUSED_PROLOGUE_WORDS

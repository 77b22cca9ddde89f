// host_engine.hip -- the bodies of host_engine.h: the host-side state machine of one handle or batch.
//
// Host-side glue only: device memory, pinned staging, launch order.  All arithmetic of the path runs in the kernels
// (stream_*.hip / fused_engine.hip); the only numbers computed here are the per-kernel constants of
// permutohedral_cpu.h:249,282-285,681 and the 2L+1 unary energies of densecrf3d.h:109-115, which the reference also computes
// once, outside its loops.
#include "host_engine.h"

#include <cmath>
#include <algorithm>
#include <cstring>

namespace lccrf {

void Engine::free_backward_area()
{
    if (!bwd_area) return;
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipFree(bwd_area);
    bwd_area = nullptr;
    bwd_area_bytes = 0;
}

// at least `need` bytes of area, zeroed on the call's stream when (re)allocated; a failed allocation leaves the engine without one
// and changes nothing else
int Engine::ensure_backward_area(size_t need)
{
    if (need <= bwd_area_bytes) return LCCRF_OK;
    free_backward_area();
    void *p = nullptr;
    const hipError_t ea = hipMalloc(&p, need);
    if (ea != hipSuccess) {
        (void)hipGetLastError();
        return fail(ea == hipErrorOutOfMemory ? LCCRF_E_NOMEM : LCCRF_E_HIP, "hipMalloc(%zu bytes) for the backward area: %s", need,
                    hipGetErrorString(ea));
    }
    bwd_area = static_cast<unsigned char *>(p);
    bwd_area_bytes = need;
    HIP_TRY(hipMemsetAsync(p, 0, need, stream));
    return LCCRF_OK;
}

// The area request `rq` takes on frames of up to `rows` points, in bytes (engine.h: backward_layout) ...
size_t Engine::backward_need(const BackwardRequest &rq, size_t slice, int rows) const
{
    return backward_layout(rq, crf, kdevs.data(), slice, rows, nullptr, nullptr);
}

// ... and the backward on it: inference(T, 0, relax) replayed on the step path (start + T x step), the F * rows * L floats of Q
// kept per iteration in arrays of `slice` floats, dL/dQ_T copied in, then the reverse sweep over frames of up to `rows` points.
int Engine::backward(const BackwardRequest &rq, size_t slice, int rows)
{
    const int K = (int)kernels.size(), T = rq.T;
    const size_t count = (size_t)F * rows * L;
    BackwardArea ar{};
    backward_layout(rq, crf, kdevs.data(), slice, rows, reinterpret_cast<float *>(bwd_area), &ar);
    int rc = start();                                 // (kCallerOrder: a handle's frames in locality mode are re-built the plain way once)
    if (!rc) rc = make_ready(kSized | kStepViews);
    if (rc) return rc;
    // LCCRF_OPT_FUSED_BACKWARD (include/lccrf.h section 1j): dL/dU and / or dL/dw of Potts terms normalised AFTER, on frames the fused
    // plan takes -- the replay and the sweep in one launch, the same bits (fused_backward.hip).  Decided for the whole batch, over its
    // largest frame and lattices; behind every check and the area, so a rejected call leaves the handle as it was either way.
    // With rq.counts (section 2j) too: each frame's workgroup then runs its own t_f iterations.
    const bool plain_form = !rq.compat_form && !rq.grad_compat && !rq.grad_model;   // (not the compat form: no dL/dmu, no sums, no matrix)
    bool no_features = true;
    for (int k = 0; k < K && rq.grad_features; ++k) no_features &= rq.grad_features[k] == nullptr;
    const bool dU_dw_only = plain_form && no_features;
    if (opt.fused_backward && dU_dw_only && count && !model.general() && !perm_on &&
        launch_fused_backward(crf, kdevs.data(), maxV.data(), maxRow.data(), rows, rq, ar, stream)) {
        HIP_TRY(hipGetLastError());
        report.backward(LCCRF_BACKWARD_FUSED);
        return LCCRF_OK;
    }
    // LCCRF_OPT_FUSED_BACKWARD_LEARNT (section 1k): the complement among the requests without feature gradients -- a learnt model
    // (a matrix, or a mode other than AFTER), or the compat form (dL/dmu, also of Potts terms) -- decided in the same place and the
    // same way (fused_backward_general.hip).  The sums over the frames (section 2h) are the sweep's two launches, behind the kernel.
    // With rq.counts (section 2k) too, as k_backward takes them: each frame's workgroup runs its own t_f iterations.
    if (opt.fused_backward_learnt && no_features && count && (model.general() || rq.compat_form) && !perm_on &&
        launch_fused_backward_general(crf, step_kdevs(), maxV.data(), maxRow.data(), rows, rq, ar, model.terms((size_t)K), stream)) {
        if (rq.grad_model) {
            launch_sum_frames(rq.grad_weights ? rq.grad_weights : ar.gW, F, K, rq.grad_model, stream);
            launch_sum_frames(rq.grad_compat ? rq.grad_compat : ar.gC, F, K * L * L, rq.grad_model + K, stream);
        }
        HIP_TRY(hipGetLastError());
        report.backward(LCCRF_BACKWARD_FUSED);
        return LCCRF_OK;
    }
    // LCCRF_OPT_FUSED_BACKWARD_FEATURES (section 1l): a request with at least one feature array, not in the compat form, on Potts terms
    // normalised AFTER and T >= 1 (T = 0 streams: the memset below to exactly 0 is already right) -- decided in the same place and the
    // same way (fused_backward_features.hip).  The kernel initialises the area's gb / gn itself: no memset in front of it.
    // With rq.counts (section 2l) too: each frame's workgroup runs its own t_f iterations, and one with t_f = 0 writes its dL/df as +0.
    if (opt.fused_backward_features && !no_features && plain_form && count && T >= 1 && !model.general() && !perm_on &&
        launch_fused_backward_features(crf, kdevs.data(), maxV.data(), maxRow.data(), rows, rq, ar, stream)) {
        HIP_TRY(hipGetLastError());
        report.backward(LCCRF_BACKWARD_FUSED);
        return LCCRF_OK;
    }
    for (int t = 0; t < T; ++t) {
        if (count) HIP_TRY(hipMemcpyAsync(ar.hist + (size_t)t * slice, crf.Q, count * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if ((rc = step(rq.relax))) return rc;
    }
    // (section 2j: the replay stepped every frame T times -- wasted work on a frame that stopped earlier, not a different result -- and
    // the Q left behind is the frame's own Q_{t_f}, out of the history)
    if (rq.counts && count) launch_restore_counted_q(crf, ar, T, rq.counts, stream);
    // (section 2h: the per-frame values behind grad_model live in the area where the caller left their own array out)
    float *const grad_weights = rq.grad_weights ? rq.grad_weights : ar.gW, *const grad_compat = rq.grad_compat ? rq.grad_compat : ar.gC;
    if (grad_compat && K && (!count || T == 0))       // nothing depends on the matrices: exactly 0, in every frame
        HIP_TRY(hipMemsetAsync(grad_compat, 0, (size_t)F * K * L * L * sizeof(float), stream));
    if (!count) {                                     // nothing to differentiate: dL/dw = 0
        if (grad_weights && K) HIP_TRY(hipMemsetAsync(grad_weights, 0, (size_t)F * K * sizeof(float), stream));
        if (rq.grad_model && K) HIP_TRY(hipMemsetAsync(rq.grad_model, 0, (size_t)K * (1 + L * L) * sizeof(float), stream));
        report.backward(LCCRF_BACKWARD_STREAM);
        return LCCRF_OK;
    }
    for (int k = 0; k < K && rq.grad_features; ++k) {
        if (!rq.grad_features[k]) continue;
        if (T == 0)                                   // nothing depends on the features: exactly 0
            HIP_TRY(hipMemsetAsync(rq.grad_features[k], 0, (size_t)F * rows * kernels[k].dev.d * sizeof(float), stream));
        else
            HIP_TRY(hipMemsetAsync(ar.gb[k], 0, ar.feat_floats[k] * sizeof(float), stream));
    }
    HIP_TRY(hipMemcpyAsync(ar.G, rq.grad_prob, count * sizeof(float), hipMemcpyDeviceToDevice, stream));
    // (sections 1m / 2i: feature gradients of terms that are not all AFTER -- the sweep is told the modes and the true norms)
    BackwardModes bm{};
    for (int k = 0; k < K; ++k) bm.mode[k] = model.mode(k), bm.norm[k] = kdevs[k].norm;
    launch_backward_sweep(crf, step_kdevs(), maxV.data(), rows, rq, ar, model.compat_arg(), stream, model.pre_arg(),
                          model.n_modes && !no_features ? &bm : nullptr);
    HIP_TRY(hipGetLastError());
    report.backward(LCCRF_BACKWARD_STREAM);
    return LCCRF_OK;
}

int Engine::need_io()
{
    if (io_a) return LCCRF_OK;
    const size_t nl = (size_t)Fcap * maxN * L;
    int rc;
    if ((rc = mem.alloc(&io_a, nl))) return rc;
    if ((rc = mem.alloc(&io_b, nl))) return rc;
    if ((rc = mem.alloc(&io_map, (size_t)Fcap * maxN))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return LCCRF_OK;
}

int Engine::perm_min_points()
{
    static const char *e = ab_env("LCCRF_PERM_MIN");                         // A/B switch (same results): locality mode from this many points
    static const int v = e ? std::max(atoi(e), 64) : kPermMinPointsDefault;
    return v;
}

int Engine::ensure_sort_scratch()
{
    // (complete or nothing: an allocation that fails half way -- E_NOMEM -- must not leave a later build with some of the
    // arrays null; what a failed attempt did allocate stays with the arena until the engine goes -- ADVICE r4)
    if (sort_scratch_complete) return LCCRF_OK;
    int bits = 8;
    while (bits < 16 && (1 << bits) < 2 * maxN) ++bits;
    sort.bits = bits;
    const size_t nbk = ((size_t)1 << bits) + 1, Fz = (size_t)Fcap;
    int rc;
    if ((rc = mem.alloc(&sort.cells, Fz * maxNpad * kMaxD))) return rc;
    if ((rc = mem.alloc(&sort.partial, Fz * ((maxNpad + 255) / 256 + 1) * 2 * kMaxD))) return rc;
    if ((rc = mem.alloc(&sort.plan, Fz * kSortPlan))) return rc;
    if ((rc = mem.alloc(&sort.code, Fz * maxNpad))) return rc;
    if ((rc = mem.alloc(&sort.hist, Fz * nbk))) return rc;
    if ((rc = mem.alloc(&sort.start, Fz * nbk))) return rc;
    if ((rc = mem.alloc(&sort.tiles, Fz * ((nbk + 4095) / 4096 + 1)))) return rc;
    if ((rc = mem.alloc(&sort.perm, Fz * maxNpad))) return rc;
    if ((rc = mem.alloc(&sort.iperm, Fz * maxNpad))) return rc;
    if ((rc = mem.alloc(&Qp, Fz * maxN * L))) return rc;
    if ((rc = mem.alloc(&unary_p, Fz * maxN * L))) return rc;
    // the vertex order of every kernel (one kernel at a time on the engine's stream: one set of arrays sized for the largest)
    int vcap = 0;
    for (auto &ks : kernels) vcap = std::max(vcap, ks.dev.Epad);
    for (auto &ks : spare) vcap = std::max(vcap, ks.dev.Epad);
    sort.vcap = vcap;
    int vbits = 10;
    while (vbits < 21 && (1 << vbits) < 4 * vcap) ++vbits;
    sort.vbits = vbits;
    const size_t vnbk = ((size_t)1 << vbits) + 1;
    if ((rc = mem.alloc(&sort.vcode, Fz * vcap))) return rc;
    if ((rc = mem.alloc(&sort.vkey, Fz * vcap))) return rc;
    if ((rc = mem.alloc(&sort.vph, Fz * 64))) return rc;
    if ((rc = mem.alloc_pinned(&sort.vbad, 1))) return rc;
    *sort.vbad = 0;
    if ((rc = mem.alloc(&sort.vhist, Fz * vnbk))) return rc;
    if ((rc = mem.alloc(&sort.vstart, Fz * vnbk))) return rc;
    if ((rc = mem.alloc(&sort.vtiles, Fz * ((vnbk + 4095) / 4096 + 1)))) return rc;
    if ((rc = mem.alloc(&sort.vpartial, Fz * ((maxNpad + 255) / 256 + 1) * 2 * kMaxD))) return rc;
    if ((rc = mem.alloc(&sort.vplan, Fz * (2 * kMaxD + 3)))) return rc;
    sort_scratch_complete = true;
    return LCCRF_OK;
}

int Engine::init(int device_id, int frames, int max_points, int n_labels)
{
    device = device_id;
    Fcap = F = frames;
    maxN = max_points;
    maxNpad = (max_points + 3) & ~3;
    L = n_labels;
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    mem.stream = stream;
    for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
    const size_t nl = (size_t)Fcap * maxN * L;
    int rc;
    if ((rc = mem.alloc(&npoints_own, Fcap))) return rc;
    if ((rc = mem.alloc(&unary_own, nl))) return rc;
    if ((rc = mem.alloc(&crf.Q, nl))) return rc;
    if ((rc = mem.alloc(&crf.next, nl))) return rc;
    if ((rc = mem.alloc(&crf.map, (size_t)Fcap * maxN))) return rc;
    crf.bits_stride = (maxN + 63) / 64;
    if (n_labels == 2 && (rc = mem.alloc(&crf.map_bits, (size_t)Fcap * std::max(crf.bits_stride, 1)))) return rc;
    if ((rc = mem.alloc(&label_own, (size_t)Fcap * maxN))) return rc;
    if ((rc = mem.alloc_pinned(&V_host, (size_t)LCCRF_MAX_KERNELS * Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&row_host, (size_t)LCCRF_MAX_KERNELS * row_stride()))) return rc;
    if ((rc = mem.alloc_pinned(&long_host, (size_t)LCCRF_MAX_KERNELS * Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&late_status, 1))) return rc;
    *late_status = 0;
    if ((rc = mem.alloc_pinned(&done_word, 1))) return rc;
    *done_word = 0;
    if ((rc = mem.alloc(&frame_status, Fcap))) return rc;
    if ((rc = mem.alloc(&fb_list, Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&frame_status_host, Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&fb_list_host, Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&npoints_bad, 1))) return rc;
    *npoints_bad = 0;
    if ((rc = mem.alloc(&conv_dev, (size_t)7 * Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&conv_host, (size_t)4 * Fcap))) return rc;
    if ((rc = mem.alloc_pinned(&conv_running, 1))) return rc;
    *conv_running = 0;
    crf.F = F;
    crf.maxN = maxN;
    crf.L = L;
    crf.K = 0;
    crf.n_points = npoints_own;
    crf.unary = unary_own;
    return LCCRF_OK;
}

void Engine::destroy()
{
    flight = Flight::kUnknown;
    if (stream) (void)hipStreamSynchronize(stream);
    free_backward_area();
    if (fb) {
        fb->destroy();
        delete fb;
        fb = nullptr;
    }
    mem.release();
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    if (ev_order) (void)hipEventDestroy(ev_order);
    model.release();
    if (lean_prep.ev0) (void)hipEventDestroy(lean_prep.ev0);
    if (lean_prep.ev1) (void)hipEventDestroy(lean_prep.ev1);
    lean_prep = LeanPrep{};
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

// Allocate the lattice of one more pairwise kernel (all frames).
int Engine::add_kernel(int d, float w, bool own_features, bool stage)
{
    if ((int)kernels.size() >= LCCRF_MAX_KERNELS)
        return fail(LCCRF_E_CAPACITY, "at most %d pairwise kernels", LCCRF_MAX_KERNELS);
    if (d < 1 || d > LCCRF_MAX_DIMS) return fail(LCCRF_E_INVALID, "feature dims %d not in [1,%d]", d, LCCRF_MAX_DIMS);
    for (size_t i = 0; i < spare.size(); ++i) {     // a recycled engine already owns a lattice of this shape
        if (spare[i].dev.d == d && (!stage || spare[i].feat_stage) && (!own_features || spare[i].feat_own)) {
            KernelState ks = spare[i];
            spare.erase(spare.begin() + i);
            ks.dev.w = w;
            ks.dev.feat = ks.feat_own;
            ks.maxV = ks.dev.Epad;
            ks.maxRow = 0;
            ks.build_counted = false;
            ks.root_valid = false;
            kernels.push_back(ks);
            sync_views();
            return LCCRF_OK;
        }
    }
    KernelState ks;
    KernelDev &k = ks.dev;
    k.d = d;
    k.D1 = d + 1;
    k.maxN = maxN;
    k.maxNpad = maxNpad;
    k.Epad = maxNpad * k.D1;
    k.cap = next_pow2(2L * k.Epad);
    // lattice values of a frame: [0, L) unused, [L, 2L) the all-zero "absent neighbour" (vertex -1), vertex v at
    // vbase + v*L; with L = 2 and an even stride, vertex pairs (2t, 2t+1) are 16-byte aligned (k_blur2)
    k.vstride = (k.Epad + 2) * L;
    k.vbase = 2 * L;
    k.w = w;
    // permutohedral_cpu.h:681 / :249 / :282-285 (quirk Q4): same expressions, same types
    k.alpha = 1.0f / (1 + powf(2, -d));
    k.inv_dp1 = 1.0f / (d + 1);
    const float inv_std_dev = sqrt(2.0 / 3.0) * (d + 1);
    for (int i = 0; i < d; ++i) k.scale[i] = (float)(1.0 / sqrt((double)((i + 2) * (i + 1))) * inv_std_dev);
    const size_t Fz = (size_t)Fcap, E = (size_t)k.Epad;
    int rc;
    if ((rc = mem.alloc(&k.rem0, Fz * maxNpad * d))) return rc;
    if ((rc = mem.alloc(&k.rank, Fz * maxNpad * d))) return rc;
    if ((rc = mem.alloc(&k.bary, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.offset, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.slot, Fz * k.cap))) return rc;
    if ((rc = mem.alloc(&k.slot_of, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.flag, Fz * (E + 1)))) return rc;
    if ((rc = mem.alloc(&k.prefix, Fz * (E + 1)))) return rc;
    if ((rc = mem.alloc(&k.rep, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.V, Fz))) return rc;
    if ((rc = mem.alloc(&k.rowmax, Fz * (1 + kBuildStats)))) return rc;     // (rowmax, then the build's counters)
    ks.bstat = k.rowmax + Fz;
    if ((rc = mem.alloc(&k.nbr, Fz * k.D1 * E * 2))) return rc;
    // one frame in flight, large frames (the object API's handles are sized for SLAM frames, which run on the one-workgroup engines):
    // the blur passes go two per launch and read a two-hop neighbour table
    if (Fcap == 1 && L == 2 && allow_perm && (rc = mem.alloc(&k.nbr2, (size_t)(k.D1 / 2) * E * 8))) return rc;
    if (L == 2 && allow_perm && maxN >= perm_min_points()) {
        if (!tbl_bad) {
            if ((rc = mem.alloc_pinned(&tbl_bad, 2))) return rc;
            tbl_bad[0] = tbl_bad[1] = 0;
        }
        k.tbl_bad = tbl_bad;
        if ((rc = mem.alloc(&k.fastn, Fz * E))) return rc;
        if ((rc = mem.alloc(&k.ndist, (size_t)kNdistAxes))) return rc;
        if ((rc = mem.alloc(&k.nearoff, Fz * 2 * E * 2))) return rc;
        if (!ndist_host && (rc = mem.alloc_pinned(&ndist_host, (size_t)LCCRF_MAX_KERNELS * kNdistAxes))) return rc;
    }
    // large frames, a few in flight: the sorted build also leaves the neighbour table in its compact form (16-bit offsets), for
    // the batches of kNbrcMinFrames..kNbrcMaxFrames frames this engine may see
    if (k.tbl_bad && Fcap >= kNbrcMinFrames) {
        const size_t Fc = (size_t)std::min(Fcap, kNbrcMaxFrames);
        if ((rc = mem.alloc(&k.nbrc, Fc * k.D1 * E * 2))) return rc;
        if ((rc = mem.alloc(&k.nbrc_base, Fc * k.D1 * (E / kNbrcBlock + 1) * 2))) return rc;
    }
    if ((rc = mem.alloc(&k.rowptr, Fz * (E + 1)))) return rc;
    // (frames of the one-workgroup engines' range keep their rows in LDS there; on the streaming engine they are summed in line: a
    // batch engine for 16 384 SLAM frames would carry 270 MB of lists per kernel)
    if (maxN > kLongRowListMinPoints) {
        if ((rc = mem.alloc(&k.longrow, Fz * kLongRowCap))) return rc;
        if ((rc = mem.alloc(&k.longcnt, Fz))) return rc;
    }
    if ((rc = mem.alloc(&k.csr_pt, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.csr_w, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.csr_pos, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.pk, Fz * E))) return rc;
    if ((rc = mem.alloc(&k.nbr16, Fz * k.D1 * E))) return rc;
    if ((rc = mem.alloc(&k.norm, Fz * maxN))) return rc;
    if ((rc = mem.alloc(&k.val0, Fz * k.vstride))) return rc;
    if ((rc = mem.alloc(&k.val1, Fz * k.vstride))) return rc;
    if (own_features) {
        if ((rc = mem.alloc(&ks.feat_own, Fz * maxN * d))) return rc;
        k.feat = ks.feat_own;
    }
    if (stage)
        if ((rc = mem.alloc_pinned(&ks.feat_stage, Fz * maxN * d))) return rc;
    ks.maxV = k.Epad;
    kernels.push_back(ks);
    sync_views();
    return LCCRF_OK;
}

// Park everything for the next user of this engine (object API handle cache).
void Engine::recycle()
{
    // (a synchronisation that starts after the kernel has ended costs ~10 us: the runtime queues a barrier packet and
    // waits for its round trip; the done word has already told us that nothing is in flight)
    // getMap() saw every label land: the kernel's last stores (V_out, frame_status, the done word) follow within a microsecond or
    // two.  Nobody waits for them here (the tracker's next frame is 33 ms away); the next user of this handle settles it before it
    // touches anything the kernel could still read or write (ensure_parked_idle, called by lccrf_create).
    const bool due = stream && flight == Flight::kLabelsSeen;
    if (stream && !due && flight != Flight::kDoneSeen) (void)hipStreamSynchronize(stream);
    flight = due ? Flight::kParkedDoneDue : Flight::kUnknown;
    free_backward_area();
    for (auto &ks : kernels) spare.push_back(ks);
    kernels.clear();
    F = Fcap;
    crf.unary = unary_own;
    crf.n_points = npoints_own;
    forget_inputs();
    unary_deferred = false;
    perm_on = vorder_on = perm_banned = false;        // (the next user's lattices decide afresh)
    unary_is_label = unary_p_valid = label_codes_valid = false;
    engine_pref = 0;
    report = RunReport{};
    model.clear(*this);                               // (the next user's terms start as Potts terms normalised AFTER the filter)
    sync_views();
}

void Engine::sync_views()
{
    kdevs.resize(kernels.size());
    maxV.resize(kernels.size());
    maxRow.resize(kernels.size());
    for (size_t i = 0; i < kernels.size(); ++i) {
        kernels[i].dev.V_host = V_host + i * Fcap;
        kernels[i].dev.rowmax_host = row_host + i * row_stride();
        kernels[i].dev.perm = perm_on ? sort.perm : nullptr;
        kernels[i].dev.iperm = perm_on ? sort.iperm : nullptr;
        kernels[i].dev.vorder = (perm_on && vorder_on && sort.vkey && kernels[i].dev.Epad <= sort.vcap) ? 1 : 0;
        kdevs[i] = kernels[i].dev;
        maxV[i] = kernels[i].maxV;
        maxRow[i] = kernels[i].maxRow;
    }
    model.views_changed();
    crf.K = (int)kernels.size();
    crf.F = F;
    crf.activeN = activeN;
    crf.perm = perm_on ? sort.perm : nullptr;
    crf.perm_stride = maxNpad;
}

// Lattice + normalisation of kernels [k0, k0+n) for every frame (PottsPotential3D ctor).
// SLAM-size frames take the fused build (one launch for all of them when they share d);
// anything else the streaming build (19 launches per kernel).
int Engine::build_kernels(int k0, int n, bool may_reorder)
{
    for (int k = k0; k < k0 + n; ++k) {
        kernels[k].maxV = kernels[k].dev.Epad;
        kernels[k].root_valid = false;                  // (section 1g: the roots of the norm this build replaces)
    }
    if (k0 == 0) {                                     // a build of every kernel decides the internal point order afresh
        static const bool no_perm = ab_env("LCCRF_NO_PERM") != nullptr;   // A/B and cross-check switch: same results either way
        const int NAp = active_points(crf);
        const bool want = allow_perm && !no_perm && !perm_banned && (!perm_scoped || may_reorder) && n > 0 && n == (int)kernels.size() && NAp >= perm_min_points();
        if (want || perm_on) {                         // whatever was derived in the old order is stale
            if (unary_is_label) unary_deferred = true;
            unary_p_valid = label_codes_valid = false;
        }
        perm_on = false;
        // ... and, with the points permuted, whether the lattices are built by SORTING the entries on the row-major code of their
        // vertex (ids along the lattice's axes: the blur pass touches half as many lines) -- yes unless switched off: with the
        // points in row-major order too it wins at every number of frames in flight (notes/r4_experiments.md section 2)
        static const char *env_vo = ab_env("LCCRF_VERTEX_ORDER");               // A/B switch: 1 on, 0 off (same results)
        const int vo = env_vo ? (atoi(env_vo) ? 1 : 2) : opt.vertex_order;
        vorder_on = want && !vorder_broken && vo != 2;
        sync_views();
        if (want) {
            int rcs = ensure_sort_scratch();
            if (rcs) return rcs;
            int src = 0;                               // one order for the whole CRF (Q is shared): the kernel with most dimensions decides
            for (int k = 1; k < n; ++k)
                if (kernels[k].dev.d > kernels[src].dev.d) src = k;
            // with the sorted build the points follow the vertices: (coarse) row-major order of their cells in the lattice's own basis
            // instead of the Z-order curve (C5 x 8: splat 30.5 -> 27.7, slice 24.2 -> 19.5 us, build 1.93 -> 1.76 ms)
            sort.rm_points = vorder_on ? 1 : 0;
            launch_sort_points(kdevs[src], crf, sort, stream);
            HIP_TRY(hipGetLastError());
            perm_on = true;
        }
    }
    sync_views();
    const bool no_small = ab_env("LCCRF_NO_FUSED_BUILD") != nullptr;   // debug / cross-check switch
    int k = k0;
    while (k < k0 + n) {
        int m = 1;
        const int NA = active_points(crf);
        // (locality mode: the one-workgroup build knows nothing of the internal point order -- ADVICE r4: with the threshold lowered
        // below its range it would have built in the caller's order under an engine that iterates in the permuted one)
        const bool small_ok = !no_small && !perm_on;
        if (small_ok && k + 1 < k0 + n && build_small_supported(&kdevs[k], 2, NA)) m = 2;
        if (small_ok && build_small_supported(&kdevs[k], m, NA)) {
            for (int u = 0; u < m; ++u) kernels[k + u].dev.nbr2_ok = kernels[k + u].dev.nbrc_ok = kernels[k + u].dev.fast0_ok = kernels[k + u].dev.longrow_ok = 0;
            for (int u = 0; u < m; ++u) kernels[k + u].build_counted = false;
            launch_build_small(&kdevs[k], m, NA, crf, stream);   // writes V / rowmax to the pinned mirrors itself
        } else {
            m = 1;
            kernels[k].dev.nbr2_ok = kernels[k].dev.nbr2 != nullptr;      // (the streaming build fills the two-hop table when there is one)
            kernels[k].dev.longrow_ok = kdevs[k].longrow_ok = kernels[k].dev.longrow != nullptr;   // (... and lists the long rows: the normalisation below reads the list)
            kernels[k].dev.nbrc_ok = kernels[k].dev.nbrc != nullptr && kernels[k].dev.vorder && F >= kNbrcMinFrames && F <= kNbrcMaxFrames;   // (... and the sorted build the compact one)
            kernels[k].dev.fast0_ok = kernels[k].dev.tbl_bad != nullptr && kernels[k].dev.vorder;
            kernels[k].dev.nbr2_first = kernels[k].dev.fast0_ok;              // (what build_kernel_d derives from the same two fields)
            launch_build_kernel(kdevs[k], crf, stream, perm_on ? &sort : nullptr, kernels[k].bstat);
            launch_norm(kdevs[k], crf, kernels[k].maxV, stream);
            HIP_TRY(hipMemcpyAsync(V_host + (size_t)k * Fcap, kernels[k].dev.V, sizeof(int) * F, hipMemcpyDeviceToHost, stream));
            // (rowmax and, behind its Fcap ints, the build's counters of the F frames: one copy)
            HIP_TRY(hipMemcpyAsync(row_host + k * row_stride(), kernels[k].dev.rowmax, sizeof(int) * ((size_t)Fcap + (size_t)F * kBuildStats), hipMemcpyDeviceToHost, stream));
            kernels[k].build_counted = true;
            if (kernels[k].dev.longrow)
                HIP_TRY(hipMemcpyAsync(long_host + (size_t)k * Fcap, kernels[k].dev.longcnt, sizeof(int) * F, hipMemcpyDeviceToHost, stream));
            if (kernels[k].dev.fast0_ok)
                HIP_TRY(hipMemcpyAsync(ndist_host + (size_t)k * kNdistAxes, kernels[k].dev.ndist, sizeof(int) * kNdistAxes, hipMemcpyDeviceToHost, stream));
        }
        k += m;
    }
    HIP_TRY(hipGetLastError());
    sync_views();                                       // (nbr2_ok)
    sizes_known = false;
    return LCCRF_OK;
}

// After the builds: learn max V per kernel so inference grids are sized to the lattice.
// Build every kernel added since the last build (object API: add_pairwise only stages features).
int Engine::flush_builds(bool may_reorder)
{
    const int n = (int)kernels.size();
    if (built_upto >= n) return LCCRF_OK;
    const int k0 = built_upto;
    built_upto = n;
    return build_kernels(k0, n - k0, may_reorder);
}

int Engine::learn_sizes(bool may_reorder)
{
    int rc0 = flush_builds(may_reorder);
    if (rc0) return rc0;
    if (sizes_known) return LCCRF_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    if (*npoints_bad) {
        *npoints_bad = 0;
        return fail(LCCRF_E_CAPACITY, "a bound n_points[f] lies outside [0, max_points=%d] (the kernels clamped it)", maxN);
    }
    if (sort.vbad && *sort.vbad) {                     // a frame's vertices do not fit a 62-bit row-major code: hash build from now on
        *sort.vbad = 0;
        vorder_broken = true;
        int rcb = build_kernels(0, (int)kernels.size(), may_reorder);
        if (rcb) return rcb;
        HIP_TRY(hipStreamSynchronize(stream));
    }
#if LCCRF_INSTRUMENT
    if (tbl_bad && ab_env("LCCRF_FAST0_BREAK")) tbl_bad[1] = 1;      // test hook: as if the build had found an axis-0 neighbour elsewhere
#endif
    if (tbl_bad && (tbl_bad[0] || tbl_bad[1])) {
        // [0] a block's neighbours span more than 16 bits: the blur reads the 32-bit table; [1] an axis-0 neighbour that is not the
        // next / previous id (cannot happen with exact codes -- checked all the same): the first blur pass keeps its own launch
        for (auto &ks : kernels) {
            if (tbl_bad[0]) ks.dev.nbrc_ok = 0;
            if (tbl_bad[1]) ks.dev.fast0_ok = 0;
        }
#if LCCRF_INSTRUMENT
        if (tbl_bad[0]) fprintf(stderr, "lccrf: compact neighbour table abandoned (a block's neighbours span more than its offsets hold)\n");
        if (tbl_bad[1]) fprintf(stderr, "lccrf: first blur pass keeps its own launch (an axis-0 neighbour is not an adjacent id)\n");
#endif
        tbl_bad[0] = tbl_bad[1] = 0;
    }
    for (size_t k = 0; k < kernels.size(); ++k) {
        // how many blur passes ride in the splat (sorted build): pass 0 always (adjacent ids); passes 1 and 2 when the largest id
        // distances of their neighbours fit the halo of a window of up to 1024 vertices that keeps >= 3/4 of its lanes productive
        KernelDev &kd = kernels[k].dev;
        kd.splat_passes = kd.fast0_ok ? 1 : 0;
        kd.splat_halo = 1;
        kd.splat_block = 0;
        static const char *env_sp = ab_env("LCCRF_SPLAT_PASSES");               // A/B switch (same results): at most this many
        const int cap = env_sp ? atoi(env_sp) : 3;
        if (kd.fast0_ok && cap >= 2) {
            const int *nd = ndist_host + k * kNdistAxes;
            int halo = 1;
            for (int j = 1; j < std::min(kd.D1, std::min(cap, 3)); ++j) {
                if (nd[j] < 1 || nd[j] > 127 || halo + nd[j] > 1024 / 8) break;
                halo += nd[j];
                kd.splat_passes = j + 1;
                kd.splat_halo = halo;
            }
            // single frames pair the passes behind the splat off a two-hop table built for the pairs (1,2), (3,4) ...: 1 or 3 passes
            if (kd.splat_passes == 2 && kd.nbr2 && kd.D1 > 3) { kd.splat_passes = 1; kd.splat_halo = 1; }
            if (kd.splat_passes >= 2) kd.splat_block = kd.splat_halo * 8 <= 256 ? 256 : kd.splat_halo * 8 <= 512 ? 512 : 1024;
        }
        int m = 0, r = 0, nlong = 0;
        for (int f = 0; f < F; ++f) {
            m = std::max(m, V_host[k * Fcap + f]);
            r = std::max(r, row_host[k * row_stride() + f]);
            if (kd.longrow_ok) nlong = std::max(nlong, long_host[k * Fcap + f]);
        }
        // a coarse kernel over many points (listed rows, or more than ~4 entries per row on average): the row-walking splat with
        // its loads up front + a workgroup per listed row, no blur pass in the splat
        const int NAr = active_points(crf);
        kd.long_mode = kd.longrow_ok && (nlong > 0 || (long)NAr * kd.D1 > 4L * std::max(m, 1));
        if (kd.long_mode && (long)NAr * kd.D1 >= 16L * std::max(m, 1)) kd.long_mode = 2;       // ... a wavefront per vertex from ~16 entries per row
        kernels[k].maxV = m;
        kernels[k].maxRow = r;
    }
    sync_views();
    sizes_known = true;
    invalidate_lean_prep();                            // (every path that changes a lattice clears sizes_known and so comes through here)
    fused_fits = engine_pref != 1 && !perm_on && fused_supported(crf, kdevs.data(), maxV.data(), maxRow.data(), &fused_lds);
    multi_fits = engine_pref != 1 && !perm_on && multilabel_supported(crf, kdevs.data(), maxV.data(), maxRow.data());
    learnt_fits = engine_pref != 1 && !perm_on && multilabel_general_supported(crf, kdevs.data(), maxV.data(), maxRow.data());
    choose_sized_engine();
    if (engine_pref == 2 && !fused_fits && sized_engine != 5 && sized_engine != 6)
        return fail(LCCRF_E_CAPACITY, "fused engine requested but the problem does not fit one workgroup's LDS");
    return LCCRF_OK;
}

// setUnaryEnergyFromLabel (densecrf3d.h:100-130) is deferred: the 2L+1 energies travel as a kernel
// argument and either the one-launch-per-frame kernel derives the unaries itself or ensure_unary()
// launches the small kernel when somebody needs the array.  `label` must stay readable until then.
UnaryTable Engine::label_table(const float *conf) const
{
    // densecrf3d.h:109-115.  log(float) binds to the float overload at the reference's call
    // site (src/Tracking.cc:21-43 sees `using namespace std` from include/Tracking.h:55).
    UnaryTable tb;
    tb.v[0] = -logf(1.0f / L);
    for (int i = 0; i < L; ++i) {
        tb.v[1 + i] = -logf((1.0f - conf[i]) / (L - 1));
        tb.v[1 + L + i] = -logf(conf[i]);
    }
    return tb;
}

void Engine::defer_unary_from_label(const int16_t *label, const float *conf)
{
    const UnaryTable tb = label_table(conf);
    crf.unary = unary_own;
    unary_deferred = true;
    unary_is_label = true;
    label_codes_valid = false;                        // (until ensure_unary() has written them for these labels and this table)
    deferred_label = label;
    deferred_tbl = tb;
    unary_set = true;
}

// raw unary energies [F][maxN][L] at `p` (the engine's own array, filled by the caller's copy, or a bound device array: read only)
void Engine::bind_unary(const float *p)
{
    crf.unary = const_cast<float *>(p);
    unary_deferred = unary_is_label = unary_p_valid = label_codes_valid = false;
    unary_set = true;
}

int Engine::ensure_unary()
{
    if (!unary_deferred) return LCCRF_OK;
    unary_deferred = false;
    // two labels: the points' codes and the three pairs go out with the energies (no memory for them: the energies alone)
    label_codes_valid = false;
    if (L == 2 && !label_codes) {
        unsigned char *pc = nullptr;
        float *pp = nullptr;
        if (mem.alloc(&pc, (size_t)Fcap * maxN, false) == LCCRF_OK && mem.alloc(&pp, (size_t)kLabelPairFloats) == LCCRF_OK) {
            label_codes = pc;
            label_pairs = pp;
        } else {
            (void)hipGetLastError();
        }
    }
    const bool lbl = L == 2 && label_codes && crf.unary == unary_own;
    launch_unary_from_label_tbl(crf, deferred_label, deferred_tbl, stream, lbl ? label_codes : nullptr, lbl ? label_pairs : nullptr);
    HIP_TRY(hipGetLastError());
    label_codes_valid = lbl;
    return LCCRF_OK;
}

int Engine::start()
{
    if (!unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    // (kCallerOrder: object API after a locality-mode inference(): label-derived energies sit in that order)
    if (int rc = make_ready(kSettled | kCallerOrder | kUnaries)) return rc;
    launch_start(crf, stream);
    started = true;
    return LCCRF_OK;
}

int Engine::step(float relax)
{
    if (!started) return fail(LCCRF_E_STATE, "stepInference before startInference");
    // (kUnaries: label-derived energies follow the lattices' point order: re-derived after a re-build)
    const int rc = make_ready(kSettled | kCallerOrder | kSized | kUnaries | kStepViews);
    if (rc) return rc;
    launch_step_stream(crf, step_kdevs(), maxV.data(), relax, stream, model.compat_arg(), model.pre_arg());
    return LCCRF_OK;
}

// Can the whole frame (lattices + normalisation + inference) run as ONE launch (frame_engine.hip)?
bool Engine::frame_ok() const
{
    static const bool no_frame = ab_env("LCCRF_NO_FRAME") != nullptr;   // cross-check switch: two-kernel path, same results
    // terms with a matrix or a mode: only under LCCRF_OPT_FRAME_GENERAL, two labels, frames of the general kernels' size (frame_general.hip)
    if (model.general() && !(opt.frame_general && L == 2 && active_points(crf) <= kGeneralMaxPoints)) return false;
    return !no_frame && engine_pref == 0 && !kernels.empty() && frame_supported(crf, kdevs.data());
}

// One launch per frame; whether every frame fitted the kernel's LDS plan is known at the next
// synchronisation point (resolve_late), which re-runs the batch on the two-kernel path if not.
int Engine::run_frame(const Schedule &run)
{
    const int with_map = run.with_map;
    const bool stop = run.until_converged;
    const bool general = model.general();             // (frame_ok: under LCCRF_OPT_FRAME_GENERAL only) frame_general.hip's kernels
    *late_status = 0;
    // (label-derived energies already written for lattices in locality mode sit in the INTERNAL point order: the frame kernel, which
    //  works in the caller's order, derives them from the labels again)
    const bool from_label = (unary_deferred || (unary_is_label && perm_on)) && L == 2;
    const bool one_shape = stop || general;           // one 1024-lane workgroup per frame: no hand-off area, no record area
    unsigned *dual = nullptr;
    // The tracker's case (one frame, 255 idle CUs) and small batches (a quarter as many frames as CUs, or fewer): every
    // frame gets two workgroups, one per lattice build.
    if (crf.K == 2 && F <= kDualMaxFrames && !opt.single_wg && !one_shape) {
        if (!dual_area) {
            int rc = mem.alloc(reinterpret_cast<char **>(&dual_area), frame_dual_bytes(std::min(Fcap, kDualMaxFrames)));
            if (rc) return rc;
        }
        dual = dual_area;
        if (++dual_epoch == 0) dual_epoch = 1;
    }
    static const bool no_done_word = ab_env("LCCRF_NO_DONE_WORD") != nullptr;   // A/B switch: wait on the stream instead
    const bool by_word = late_ok && F == 1 && !no_done_word;
    if (by_word && ++done_epoch == 0) done_epoch = 1;
    const bool by_label = by_word && with_map && L == 2 && map_host && map_host == crf.map && activeN > 0;
    if (by_label) memset(map_host, 0xff, (size_t)activeN * sizeof(int16_t));
    // full-size frames, two per CU (frame_lean.hip): the record area its loop re-reads is allocated when a batch first wants it
    // (sized for the frames BOUND, not for the handle's capacity -- 96 KB per frame: a handle created for 16384 frames that runs 1024 takes
    //  0.1 GB, not 1.6; a later, larger batch gets a new area, the old one stays with the handle until it is destroyed -- ADVICE r5)
    if (!one_shape && frame_lean_ok && lean_rec_frames < F && frame_lean_wanted(crf)) {
        // (no memory for the area: the batch keeps the one-frame-per-CU kernel, which needs none)
        lean_rec = nullptr;
        lean_rec_frames = 0;
        const int want = std::min(Fcap, std::max(F, 256));
        if (mem.alloc(reinterpret_cast<char **>(&lean_rec), frame_lean_rec_bytes(want), false)) {   // (written before it is read: no zeroing)
            lean_rec = nullptr;
            frame_lean_ok = false;
            (void)hipGetLastError();
        } else {
            lean_rec_frames = want;
        }
    }
    // a matrix or a mode on some term: the matrices travel by value from the pinned copies the setters keep, the factors of every
    // mode are formed in the kernel (no ensure_factors(): nothing of it is in HBM); until converged: the report leaves with the results
    const FrameRequest rq{run, model.terms(kernels.size()), late_status, frame_status, from_label ? deferred_label : nullptr, deferred_tbl.v,
                          by_word ? done_word : nullptr, done_epoch, conv_out(), frame_small_ok, dual, dual_epoch,
                          !one_shape && frame_lean_ok ? lean_rec : nullptr};
    const int shape = launch_frame(crf, kdevs.data(), rq, stream);
    HIP_TRY(hipGetLastError());
    frame_small_used = shape == 1;
    frame_lean_used = shape == 2;
    report.frame_run(shape, stop);
    if (stop) conv_valid = true;
    late = run;

    flight = by_label ? Flight::kPendingLabels : by_word ? Flight::kPendingDone : Flight::kPending;
    started = true;
    last_with_map = with_map;
    return LCCRF_OK;
}

int Engine::inference(int n_iter, int with_map, float relax)
{
    if (n_iter < 0) return fail(LCCRF_E_INVALID, "n_iterations < 0");
    if (!unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    int rc = resolve_late();
    if (rc) return rc;
    // Object API: nothing has been built yet (add_pairwise only stages features) -> do not build, run the
    // frame in one launch.  If a probe already forced the lattices into HBM, iterate on those instead.
    if (late_ok && frame_ok() && !(built_upto == (int)kernels.size() && sizes_known))
        return run_frame(fixed_run(n_iter, with_map, relax));
    return inference_sized(fixed_run(n_iter, with_map, relax), kMayReorder);   // (large frames: lattices built from here may use locality mode)
}

// The one place where an engine's lazily made state is brought up to date (host_engine.h: Need), in the order of the bits.
// kCallerOrder -- object API, large frames: DenseCRF::inference() runs in locality mode (internal point order, sorted build); the entry
// points that expose or continue from per-point lattice state in the CALLER's order -- stepInference, PairwisePotential::apply, the
// lattice / norm / unary probes -- get the plain build instead: built that way if they come first (they never ask for kMayReorder),
// re-built once, and the handle banned from locality mode, if not.  A batch's backward (lccrf_batch_inference_backward) wants the
// same of every frame's lattices, but for this call only: whatever it builds is built under the ban, which is lifted again on the
// way out -- the next lccrf_batch_build / _run decides the point order afresh.  "A batch" is read off !perm_scoped, which small handles
// and the sub-engine `fb` share: harmless, as lccrf_create sets allow_perm and perm_scoped together, so nothing there is ever in
// locality mode.  start() and step() on a batch find nothing to re-build: backward_call has made the batch plain before them.
int Engine::make_ready(unsigned needs)
{
    const bool call_ban = (needs & kCallerOrder) && !perm_scoped, reorder = (needs & kMayReorder) != 0;
    int rc = (needs & kSettled) ? resolve_late() : LCCRF_OK;
    if (!rc && (needs & kCallerOrder) && (perm_on || call_ban)) {
        perm_banned = true;
        if (perm_on) {
            invalidate_lattices();
            rc = flush_builds();
        }
    }
    if (!rc && (needs & kSized)) rc = learn_sizes(reorder);   // (builds what is pending: the internal point order is known after this)
    else if (!rc && (needs & kBuilt)) rc = flush_builds(reorder);
    if (!rc && (needs & kUnaries)) rc = ensure_unary();
    if (!rc && (needs & kStepViews)) rc = model.ensure_factors(*this);
    if (call_ban) perm_banned = false;
    return rc;
}

// lccrf_batch_run: per frame the PottsPotential ctors + inference(n, with_map)
int Engine::run(int n_iter, int with_map, float relax)
{
    if (n_iter < 0) return fail(LCCRF_E_INVALID, "n_iterations < 0");
    if (!unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    int rc = resolve_late();
    if (rc) return rc;
    if (frame_ok()) return run_frame(fixed_run(n_iter, with_map, relax));
    invalidate_lattices();                            // two-kernel path: rebuild for the current inputs, then infer
    return inference_sized(fixed_run(n_iter, with_map, relax));
}

// lccrf_batch_get_engine (behind kSettled): lattices in HBM and the last run not the one-launch route -> what an inference on them
// runs (or ran) on, sized_engine behind kSized; a converged run overrides that (RunReport::in_use).
int Engine::engine_in_use(int *out)
{
    const bool hbm = built && report.engine != 3;
    if (int rc = hbm ? make_ready(kSized) : LCCRF_OK) return rc;
    *out = report.in_use(hbm ? sized_engine : 0);
    return LCCRF_OK;
}

// The fused engine's kernels on the lattices in HBM (behind kSized | kStepViews): the one launch, and what the engine records of it.
// False: the frames are not ones the kernel takes and nothing was launched.  (The k_converge route leaves fused_shape as it was.)
bool Engine::launch_sized(const Schedule &run, LeanPrep *prep)
{
    const bool lbl = label_codes_valid && unary_is_label && !unary_deferred && !perm_on && crf.unary == unary_own;
    const SizedRequest rq{run, model.terms(kernels.size()), conv_out(), prep,
                          LabelCodes{lbl ? label_codes : nullptr, lbl ? label_pairs : nullptr}};
    const SizedLaunch r = launch_inference(crf, step_kdevs(), maxV.data(), maxRow.data(), rq, stream);
    if (!r.report) return false;
    report.sized_run(sized_engine, r, run.until_converged, rq.terms.general());
    started = true;
    if (run.until_converged) conv_valid = true;
    return true;
}

int Engine::inference_sized(const Schedule &run, unsigned more_needs)
{
    const int rc = make_ready(kSized | kUnaries | kStepViews | more_needs);
    if (rc) return rc;
    report.ran_on(sized_engine, false);
    last_with_map = run.with_map;
    if (perm_on || sized_engine == 1) {
        const CrfDev v = begin_iteration();
        for (int it = 0; it < run.n_iter; ++it) launch_step_stream(v, step_kdevs(), maxV.data(), run.relax, stream, model.compat_arg(), model.pre_arg());
        end_iteration(run.with_map);
        HIP_TRY(hipGetLastError());
        return LCCRF_OK;
    }
    // Potts terms (sized_engine 2): the two-frames-per-CU kernel runs from prepared launch records (fused_lean.h: LeanPrepPlan): one
    // block per frame, owned here, (re)written by the first inference behind a build -- learn_sizes() clears `valid` whenever a lattice
    // has changed.  The general kernel (4; fused_general.hip, on the factors' views of ensure_factors()) does not look at them.
    const size_t prep_need = sized_engine == 2 ? lean_prep_bytes(crf, kdevs.data(), maxV.data(), maxRow.data()) : 0;
    if (prep_need > lean_prep.bytes) {
        lean_prep.valid = false;
        lean_prep.buf = nullptr;                       // (an outgrown block stays with the arena until the handle goes)
        lean_prep.bytes = 0;
        unsigned char *p = nullptr;
        if (mem.alloc(&p, prep_need, false) == LCCRF_OK) {
            lean_prep.buf = p;
            lean_prep.bytes = prep_need;
        } else {
            (void)hipGetLastError();                   // no room: the self-contained kernel runs instead, same results
        }
        if (!lean_prep.ev0) {
            (void)hipEventCreate(&lean_prep.ev0);
            (void)hipEventCreate(&lean_prep.ev1);
        }
    }
    if (!launch_sized(run, prep_need ? &lean_prep : nullptr))
        return fail(LCCRF_E_STATE, "the fused engine's %s was chosen for a frame it does not take", sized_engine == 4 ? "general kernel" : sized_engine == 5 ? "multi-label kernel" : sized_engine == 6 ? "multi-label general kernel" : "kernel");
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

// The view a streaming iteration runs on, behind kSized | kUnaries, with Q started on it.  In locality mode that is the internal-order
// view (Qp, and the raw unaries permuted); end_iteration() un-permutes Q on the way out (densecrf_base.h:65-73 otherwise), then the map.
CrfDev Engine::begin_iteration()
{
    CrfDev v = crf;
    if (perm_on) {
        v.Q = Qp;
        if (!unary_is_label) {
            // a BOUND unary array ("bound, not copied") may have been updated in place since the last call: permute it
            // afresh every time, as the other engines read it live; only the engine's own copy is cached
            if (!unary_p_valid || crf.unary != unary_own) launch_permute_rows(crf, unary_p, crf.unary, L, 1, stream);
            unary_p_valid = true;
            v.unary = unary_p;
        }
    }
    launch_start(v, stream);
    started = true;
    return v;
}

void Engine::end_iteration(int with_map)
{
    if (perm_on) launch_permute_rows(crf, crf.Q, Qp, L, 0, stream);
    if (with_map) launch_map(crf, stream);
}

// ---- convergence-driven inference (include/lccrf.h sections 1h and 2e) ------------------------------------------------------
int Engine::check_converged_args(int max_iter, int criterion, float tol, float relax)
{
    if (criterion < 1 || criterion > (LCCRF_STOP_DELTA | LCCRF_STOP_LABELS))
        return fail(LCCRF_E_INVALID, "criterion %d is not a mask of LCCRF_STOP_DELTA (1) and LCCRF_STOP_LABELS (2)", criterion);
    if (max_iter < 0) return fail(LCCRF_E_INVALID, "max_iterations < 0");
    if (!std::isfinite(tol) || tol < 0.0f) return fail(LCCRF_E_INVALID, "tol must be finite and >= 0");
    if (!std::isfinite(relax)) return fail(LCCRF_E_INVALID, "relax is not finite");
    return LCCRF_OK;
}

// On lattices in HBM, built and sized as inference_sized() does it (never the one-launch build + inference kernel, and the prepared
// launch records are left alone): the frames the fused plan takes in ONE launch with the stop decision inside the kernel -- Potts
// terms normalised AFTER on k_converge, a batch's terms with a matrix or a mode on k_general_converge -- the rest on the streaming
// step with the bookkeeping of converge_track.hip behind it.
int Engine::inference_converged(const Schedule &run)
{
    int rc = check_converged_args(run.n_iter, run.criterion, run.tol, run.relax);
    if (rc) return rc;
    if (!unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    if ((rc = make_ready(kSettled | kSized | kMayReorder | kUnaries | kStepViews))) return rc;   // (large frames: may use locality mode)
    last_with_map = run.with_map;
    conv_valid = false;
    // Potts terms on k_converge; a BATCH whose terms carry a matrix or a mode, on the frames choose_sized_engine() names, on
    // k_general_converge (the factors' views: kStepViews above) -- a handle's converged call keeps the streaming step (include/lccrf.h
    // section 1h).  Nothing launched (a plan without room for the reduction's words): the streaming step as well.
    if (!perm_on && (sized_engine == 2 || (sized_engine == 4 && (F > 1 || batch_owned))) && launch_sized(run, nullptr)) {
        HIP_TRY(hipGetLastError());
        return LCCRF_OK;
    }
    report.ran_on(1, true);
    if ((rc = converge_stream(run))) return rc;
    conv_valid = true;
    return LCCRF_OK;
}

// lccrf_run_converged / lccrf_batch_run_converged (sections 1i and 2f): from inputs alone.  A frame the one-launch kernel takes is
// built, normalised and inferred until converged in ONE launch (run_frame with until_converged: what it leaves is run_frame's, plus the
// report); whether every frame fitted is known at the next synchronisation point, where resolve_late() re-runs the flagged ones with
// inference_converged().  Anything else builds into HBM and takes inference_converged() at once -- as does a handle whose lattices
// are already built and sized (a probe put them there), the rule of Engine::inference.
int Engine::run_converged(const Schedule &run)
{
    int rc = check_converged_args(run.n_iter, run.criterion, run.tol, run.relax);
    if (rc) return rc;
    if (!unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    if ((rc = resolve_late())) return rc;
    if (late_ok && built_upto == (int)kernels.size() && sizes_known) return inference_converged(run);
    if (frame_ok()) return run_frame(run);
    invalidate_lattices();                            // two-kernel path: rebuild for the current inputs, then infer
    return inference_converged(run);
}

// The streaming path: start, then per iteration the unchanged step, the comparison and the settle kernel, ONE synchronisation of the
// call's stream and one pinned word read -- the frames still running.  These are the frames where an iteration is many launches
// anyway.  The kept copy of the previous Q is io_a.
int Engine::converge_stream(const Schedule &run)
{
    const int max_iter = run.n_iter;
    int rc = need_io();
    if (rc) return rc;
    const CrfDev cp = begin_iteration();              // (locality mode: iterate and compare in the internal order, as inference_sized())
    const ConvergeTrack tk{io_a, reinterpret_cast<unsigned *>(conv_dev + 4 * (size_t)Fcap), conv_dev + 6 * (size_t)Fcap, conv_running,
                           conv_out()};
    launch_track_begin(cp, tk, max_iter, stream);
    int t_last = 0;
    for (int t = 1; t <= max_iter; ++t) {
        launch_step_stream(cp, step_kdevs(), maxV.data(), run.relax, stream, model.compat_arg(), model.pre_arg());
        launch_track_step(cp, tk, t, max_iter, run.criterion, run.tol, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        t_last = t;
        if (*conv_running == 0) break;
    }
    if (F > 1 && t_last > 1) launch_track_restore(cp, tk, t_last, stream);
    end_iteration(run.with_map);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

// the four result arrays of the frames bound into conv_host, behind everything queued on the engine's stream
int Engine::read_convergence()
{
    if (!conv_valid) return fail(LCCRF_E_STATE, "no converged inference has run on the current inputs");
    for (int a = 0; a < 4; ++a)
        HIP_TRY(hipMemcpyAsync(conv_host + (size_t)a * Fcap, conv_dev + (size_t)a * Fcap, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return LCCRF_OK;
}

}  // namespace lccrf

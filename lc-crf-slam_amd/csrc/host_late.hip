// host_late.hip -- settling a late-bound one-launch run (host_engine.h): taking its labels as they land, the done word, the re-run
// of the frames that did not fit its kernel, and the parked handle whose last word is still due.
#include "host_engine.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>

namespace lccrf {

namespace {

// Bounded spin on a pinned done word: true once it shows `epoch` (the frame kernel's last store), false after `limit`; the clock is
// read every `check_every` spins (a power of two).  Either way an acquire fence orders the reads that follow behind the word.
inline bool poll_done_word(const unsigned *word, unsigned epoch, std::chrono::microseconds limit, unsigned check_every)
{
    const volatile unsigned *w = word;
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (unsigned spins = 1; !(seen = (*w == epoch)); ++spins) {
        if ((spins & (check_every - 1)) == 0 && std::chrono::steady_clock::now() - t0 > limit) break;
        cpu_relax();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return seen;
}
}  // namespace

// A parked engine whose last frame was taken label by label: its kernel is over once the done word shows this frame's epoch
// (the kernel's very last store); normally that happened long ago, otherwise wait for the stream the ordinary way.
void Engine::ensure_parked_idle()
{
    if (flight != Flight::kParkedDoneDue) return;
    flight = Flight::kUnknown;
    if (!poll_done_word(done_word, done_epoch, std::chrono::microseconds(50), 64) && stream) (void)hipStreamSynchronize(stream);
}

// getMap() with one frame in flight whose labels go straight into map_host: take them as they land.  True: `out` holds the n labels
// and the run counts as settled -- every label is there, so the frame fitted and the kernel is past its last read -- but not as
// formally finished: V_out, frame_status and the done word are stored behind the labels (and a helper workgroup may be in its
// epilogue): the handle counts as idle only once recycle() has seen the done word.  False: the ordinary path (resolve_late) is to run.
bool Engine::take_labels(int16_t *out, int n)
{
    if (flight != Flight::kPendingLabels) return false;
    flight = Flight::kPendingDone;
    const volatile int16_t *m = map_host;
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true, timed_out = false;
    unsigned spins = 0;
    for (int i = 0; i < n && ok; ++i) {
        int16_t v;
        while ((v = m[i]) == (int16_t)-1) {               // (bounded: whatever goes wrong is left to the ordinary path)
            if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) { ok = false; timed_out = true; break; }
            cpu_relax();
        }
        if (v < 0) ok = false;                            // -2: the frame did not fit the one-launch kernel
    }
    if (ok) {
        std::atomic_thread_fence(std::memory_order_acquire);
        memcpy(out, map_host, (size_t)n * sizeof(int16_t));
        flight = Flight::kLabelsSeen;
        return true;
    }
    if (timed_out) flight = Flight::kPending;             // (a delayed frame: do not spin another 2 ms on the done word, wait on the stream)
    return false;
}

// Before anything looks at (or continues from) the results of a late-bound inference.
// *seen_done (optional): the frame's results were observed through the done word -- the caller may read the pinned
// outputs without a stream synchronisation of its own.
int Engine::resolve_late(bool *seen_done)
{
    if (seen_done) *seen_done = false;
    if (!run_pending()) return LCCRF_OK;
    // bounded poll; a word that never comes is waited for the ordinary way
    const bool seen = flight != Flight::kPending && poll_done_word(done_word, done_epoch, std::chrono::milliseconds(2), 1024);
    flight = Flight::kUnknown;
    if (!seen) HIP_TRY(hipStreamSynchronize(stream));
    if (*npoints_bad) {                                // (the one-launch path never passes through learn_sizes())
        *npoints_bad = 0;
        return fail(LCCRF_E_CAPACITY, "a bound n_points[f] lies outside [0, max_points=%d] (the kernels clamped it)", maxN);
    }
    if (*late_status == 0) {
        if (seen_done) *seen_done = seen;
        return LCCRF_OK;
    }
    *late_status = 0;                                  // some frame did not fit the one-launch kernel
    if (seen) HIP_TRY(hipStreamSynchronize(stream));   // (the kernel has nothing left to do; the stream formally still holds it)
    HIP_TRY(hipMemcpy(frame_status_host, frame_status, sizeof(int) * F, hipMemcpyDeviceToHost));
    int n = 0;
    for (int f = 0; f < F; ++f)
        if (frame_status_host[f]) fb_list_host[n++] = f;
    report.settled(n, n > 0 && n < F);
    if (frame_small_used && 8 * n > F) frame_small_ok = false;   // these lattices want the whole CU: 1024 lanes from now on
    if (frame_lean_used && 8 * n > F) frame_lean_ok = false;
    int rc = LCCRF_OK;
    if (n >= F || n == 0) {                            // every frame (always so for the object API): two-kernel path in place
        invalidate_lattices();
        rc = rerun_on(*this);
    } else {
        rc = rerun_frames(n);                          // the batch stays a one-launch batch; only the flagged frames pay twice
    }
    if (rc) return rc;
    if (timed_inf) HIP_TRY(hipEventRecord(ev[3], stream));   // the timed region now ends behind the re-run
    if (after_rerun && (rc = after_rerun(after_rerun_ctx))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));             // callers read borrowed device buffers right behind a synchronisation point
    return LCCRF_OK;
}

// What the pending one-launch run is re-run with on the two-kernel path of `e` (this engine, or the sub-engine holding its flagged
// frames): the fixed count, or -- behind run_converged() -- the same stop rule.
int Engine::rerun_on(Engine &e)
{
    return late.until_converged ? e.inference_converged(late) : e.inference_sized(late);
}

// Two-kernel path for the frames fb_list_host[0, n) only, in a compact sub-engine; results scattered back.
int Engine::rerun_frames(int n)
{
    if (fb && fb->Fcap < n) {
        fb->destroy();
        delete fb;
        fb = nullptr;
    }
    if (!fb) {
        fb = new (std::nothrow) Engine;
        if (!fb) return fail(LCCRF_E_NOMEM, "host allocation failed");
        int rc = fb->init(device, std::min(Fcap, std::max(8, next_pow2(n))), maxN, L);
        for (size_t k = 0; k < kernels.size() && !rc; ++k) rc = fb->add_kernel(kernels[k].dev.d, kernels[k].dev.w, true, false);
        if (!rc && hipStreamSynchronize(fb->stream) != hipSuccess) rc = fail(LCCRF_E_HIP, "hipStreamSynchronize after allocation failed");
        if (rc) {
            fb->destroy();
            delete fb;
            fb = nullptr;
            return rc;
        }
    }
    Engine &g = *fb;
    const hipStream_t g_own = g.stream;
    g.stream = g.mem.stream = stream;                  // everything below (lazy allocations' zeroing included) is ordered on this engine's stream
    struct Restore { Engine &g; hipStream_t s; ~Restore() { g.stream = g.mem.stream = s; } } restore{g, g_own};
    g.F = n;
    g.activeN = activeN;
    g.engine_pref = engine_pref == 1 ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(fb_list, fb_list_host, sizeof(int) * n, hipMemcpyHostToDevice, stream));
    launch_copy_frames(g.npoints_own, 4, crf.n_points, 4, fb_list, n, 4, 1, stream);
    g.crf.n_points = g.npoints_own;
    for (size_t k = 0; k < kernels.size(); ++k) {
        const size_t row = (size_t)maxN * kernels[k].dev.d * sizeof(float);
        launch_copy_frames(g.kernels[k].feat_own, row, kernels[k].dev.feat, row, fb_list, n, row, 1, stream);
        g.kernels[k].dev.feat = g.kernels[k].feat_own;
        g.kernels[k].dev.w = kernels[k].dev.w;
    }
    // the model as it is now (a one-launch run under LCCRF_OPT_FRAME_GENERAL): the setters settle a pending run before they change
    // it, so this is the model the flagged frames were launched with -- it may differ from the last re-run's
    if (int rc = model.put_on(g, (int)kernels.size())) return rc;
    g.crf.unary = g.unary_own;
    if (unary_deferred || (unary_is_label && perm_on)) {   // (see run_frame: energies written in the internal point order are of no use here)
        launch_copy_frames(g.label_own, (size_t)maxN * 2, deferred_label, (size_t)maxN * 2, fb_list, n, (size_t)maxN * 2, 1, stream);
        g.unary_deferred = true;
        g.deferred_label = g.label_own;
        g.deferred_tbl = deferred_tbl;
    } else {
        const size_t row = (size_t)maxN * L * sizeof(float);
        launch_copy_frames(g.unary_own, row, crf.unary, row, fb_list, n, row, 1, stream);
        g.unary_deferred = false;
    }
    g.unary_set = true;
    g.invalidate_lattices();
    g.sync_views();
    HIP_TRY(hipGetLastError());
    int rc = rerun_on(g);
    if (rc) return rc;
    const size_t qrow = (size_t)maxN * L * sizeof(float);
    launch_copy_frames(crf.Q, qrow, g.crf.Q, qrow, fb_list, n, qrow, 0, stream);
    if (late.with_map) {
        launch_copy_frames(crf.map, (size_t)maxN * 2, g.crf.map, (size_t)maxN * 2, fb_list, n, (size_t)maxN * 2, 0, stream);
        if (crf.map_bits && g.crf.map_bits)
            launch_copy_frames(crf.map_bits, (size_t)crf.bits_stride * 8, g.crf.map_bits, (size_t)crf.bits_stride * 8, fb_list, n,
                               (size_t)crf.bits_stride * 8, 0, stream);
    }
    for (size_t k = 0; k < kernels.size(); ++k)
        launch_copy_frames(kernels[k].dev.V, 4, g.kernels[k].dev.V, 4, fb_list, n, 4, 0, stream);
    if (late.until_converged)                         // the re-run frames' reports: iterations, delta, changed, converged
        for (int a = 0; a < 4; ++a)
            launch_copy_frames(conv_dev + (size_t)a * Fcap, 4, g.conv_dev + (size_t)a * g.Fcap, 4, fb_list, n, 4, 0, stream);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

}  // namespace lccrf

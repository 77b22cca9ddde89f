// api_object.hip -- the object API of include/lccrf.h: sections 1, 1a and 1b (what a handle shares word for word with a batch --
// weights, matrices, normalisation modes, plans -- is in api_model.hip).
//
// Argument checks, pinned staging and launch order of one handle; the state machine behind it is the Engine (host_engine.h).
#include "api_common.h"

#include <cmath>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace lccrf;

// object API: up to this many points a handle's inputs (count, labels, features) are read by the kernels straight from pinned host
// memory -- the one-launch frame kernel's range (frame_supported: 4 x 1024 points), where an upload command costs more than the reads
constexpr int kObjectPinnedMaxPoints = 4096;

namespace {
// The reference builds and destroys a DenseCRF3D per frame (src/Tracking.cc:1920); doing that with
// device memory, a stream and pinned staging costs milliseconds.  Destroyed handles are therefore
// parked here and handed out again by lccrf_create when device, label count and capacity fit.
struct HandleCache {
    std::mutex m;
    std::vector<lccrf_crf *> parked;
    static constexpr size_t kMaxParked = 8;
} g_cache;

int capacity_for(int n) { return std::max(1024, ((n + n / 4 + 511) / 512) * 512); }
}  // namespace

int lccrf::apply_option(Engine &e, int option, int value)
{
    switch (option) {
    case LCCRF_OPT_SINGLE_WORKGROUP: e.opt.single_wg = value != 0; return LCCRF_OK;
    case LCCRF_OPT_FRAME_GENERAL: e.opt.frame_general = value != 0; return LCCRF_OK;    // (takes effect with the next inference / run)
    case LCCRF_OPT_FUSED_BACKWARD: e.opt.fused_backward = value != 0; return LCCRF_OK;  // (takes effect with the next backward call)
    case LCCRF_OPT_FUSED_BACKWARD_LEARNT: e.opt.fused_backward_learnt = value != 0; return LCCRF_OK;   // (the next backward call)
    case LCCRF_OPT_FUSED_BACKWARD_FEATURES: e.opt.fused_backward_features = value != 0; return LCCRF_OK;   // (the next backward call)
    case LCCRF_OPT_FUSED_MULTILABEL:                                                     // (takes effect with the next inference)
        e.opt.fused_multilabel = value != 0;
        e.choose_sized_engine();
        return LCCRF_OK;
    case LCCRF_OPT_VERTEX_ORDER:                                                         // (takes effect with the next build)
        if (value < 0 || value > 2) return fail(LCCRF_E_INVALID, "LCCRF_OPT_VERTEX_ORDER takes 0 (automatic), 1 (on) or 2 (off)");
        e.opt.vertex_order = value;
        return LCCRF_OK;
    default: return fail(LCCRF_E_INVALID, "unknown option %d", option);
    }
}

// A caller's array that a kernel or copy of handle h is about to touch: device memory of h's device, or host memory registered as
// pinned whose device address is the pointer itself -- anything else (plain pageable host memory above all) would fault the card
// with XNACK off, so it is refused here, before anything is enqueued.  When the runtime knows the allocation's extent, the `bytes`
// the call will touch must lie inside it.
int lccrf::check_device_array(const Engine &eng, const void *p, size_t bytes, const char *what)
{
    if (!bytes) return LCCRF_OK;
    if (!p) return fail(LCCRF_E_INVALID, "%s is NULL", what);
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    (void)hipGetLastError();                             // (an unknown pointer leaves an error behind; no later HIP_TRY may see it)
    if (e != hipSuccess || a.isManaged)
        return fail(LCCRF_E_INVALID, "%s (%p) is neither device memory nor pinned host memory", what, p);
    if (a.type == hipMemoryTypeDevice) {
        if (a.device != eng.device)
            return fail(LCCRF_E_INVALID, "%s (%p) is memory of device %d, the handle's is device %d", what, p, a.device, eng.device);
    } else if (a.type == hipMemoryTypeHost) {
        if (a.devicePointer != p)
            return fail(LCCRF_E_INVALID, "%s (%p) is pinned host memory whose device address differs (%p)", what, p, a.devicePointer);
    } else {
        return fail(LCCRF_E_INVALID, "%s (%p) is neither device memory nor pinned host memory", what, p);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) == hipSuccess) {
        const char *b = static_cast<const char *>(base), *q = static_cast<const char *>(p);
        if (q < b || (size_t)(q - b) > size || size - (size_t)(q - b) < bytes)
            return fail(LCCRF_E_INVALID, "%s: %zu bytes from %p run past the end of its allocation (%zu bytes from %p)", what, bytes, p,
                        size, base);
    } else {
        (void)hipGetLastError();
    }
    return LCCRF_OK;
}

extern "C" {

// --------------------------------------------------------------------------------------
// object API
// --------------------------------------------------------------------------------------
int lccrf_create(lccrf_handle *out, int device_id, int n_points, int n_labels)
{
    if (!out) return fail(LCCRF_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_points < 0) return fail(LCCRF_E_INVALID, "n_points < 0");
    if (n_labels < 1 || n_labels > LCCRF_MAX_LABELS) return fail(LCCRF_E_INVALID, "n_labels %d not in [1,%d]", n_labels, LCCRF_MAX_LABELS);
    int rc = use_device(device_id);
    if (rc) return rc;
    lccrf_crf *h = nullptr;
    {
        std::lock_guard<std::mutex> g(g_cache.m);
        for (size_t i = 0; i < g_cache.parked.size(); ++i) {
            lccrf_crf *c = g_cache.parked[i];
            if (c->eng.device == device_id && c->eng.L == n_labels && c->cap >= n_points &&
                c->cap <= std::max(4 * n_points, 4096)) {
                h = c;
                g_cache.parked.erase(g_cache.parked.begin() + i);
                break;
            }
        }
    }
    if (!h) {
        h = new (std::nothrow) lccrf_crf;
        if (!h) return fail(LCCRF_E_NOMEM, "host allocation failed");
        h->cap = capacity_for(n_points);
        rc = h->eng.init(device_id, 1, h->cap, n_labels);
        if (!rc) h->map_dev = h->eng.crf.map;             // (the engine's own label array; a handle starts with its labels in map_pin)
        // frames far beyond SLAM's (BASELINE config 5 through the reference's own interface): inference() in locality mode
        h->eng.allow_perm = h->eng.perm_scoped = h->cap >= Engine::perm_min_points();
        if (!rc) rc = h->eng.mem.alloc_pinned(&h->stage_i16, h->cap);
        if (!rc) rc = h->eng.mem.alloc_pinned(&h->stage_f32, (size_t)h->cap * n_labels);
        if (!rc) rc = h->eng.mem.alloc_pinned(&h->stage_n, 1);
        if (!rc) rc = h->eng.mem.alloc_pinned(&h->map_pin, h->cap);
        if (rc) {
            h->eng.destroy();
            delete h;
            return rc;
        }
    }
    h->eng.ensure_parked_idle();                          // (a reused handle: its last kernel has stored its done word, or we wait for it)
    h->N = n_points;
    h->eng.opt = Engine::Options::fresh();                // (a recycled handle does not inherit its last user's options ...
    h->eng.report = Engine::RunReport{};                  //  ... nor what its last run was)
    h->eng.activeN = n_points;
    h->eng.crf.map = h->map_pin;
    h->eng.map_host = h->map_pin;
    h->eng.crf.map_bits = nullptr;                       // the packed copy is the batch API's gather payload only
    h->eng.late_ok = true;
    h->label_stage_busy = false;    // a parked engine's stream is idle (recycle() synchronised it or saw the frame kernel's done word, its last store)
    // the kernels read the point count where the host wrote it (pinned, device-visible): no upload command on a path
    // whose every DMA packet costs microseconds of stream time (a parked engine's stream is idle, nothing reads the old value)
    *h->stage_n = n_points;
    h->eng.crf.n_points = h->stage_n;
    if (n_points > kObjectPinnedMaxPoints) {             // (large frames: every wavefront of every kernel reads the count)
        const hipError_t ec = hipMemcpyAsync(h->eng.npoints_own, h->stage_n, sizeof(int), hipMemcpyHostToDevice, h->eng.stream);
        if (ec != hipSuccess) {                          // (the handle is neither parked nor handed out yet: do not leak it -- ADVICE r4)
            h->eng.destroy();
            delete h;
            return fail(LCCRF_E_HIP, "hipMemcpyAsync(n_points): %s", hipGetErrorString(ec));
        }
        h->eng.crf.n_points = h->eng.npoints_own;
    }
    h->eng.sync_views();
    *out = h;
    return LCCRF_OK;
}

void lccrf_destroy(lccrf_handle h)
{
    if (!h) return;
    (void)hipSetDevice(h->eng.device);
    h->eng.recycle();
    {
        std::lock_guard<std::mutex> g(g_cache.m);
        if (g_cache.parked.size() < HandleCache::kMaxParked) {
            g_cache.parked.push_back(h);
            return;
        }
    }
    h->eng.destroy();
    delete h;
}

int lccrf_trim_cache(void)
{
    std::vector<lccrf_crf *> v;
    {
        std::lock_guard<std::mutex> g(g_cache.m);
        v.swap(g_cache.parked);
    }
    for (lccrf_crf *h : v) {
        (void)hipSetDevice(h->eng.device);
        h->eng.destroy();
        delete h;
    }
    trim_pose_stages();
    trim_unary_stage();
    trim_bf_stage();
    return (int)v.size();
}

int lccrf_set_option(lccrf_handle h, int option, int value)
{
    if (!h) return fail(LCCRF_E_INVALID, "handle is NULL");
    return apply_option(h->eng, option, value);
}

int lccrf_set_unary(lccrf_handle h, const float *unary)
{
    CHECK_H(h);
    if (!unary && h->N) return fail(LCCRF_E_INVALID, "unary is NULL");
    Engine &e = h->eng;
    const size_t n = (size_t)h->N * e.L;
    { int rl = e.resolve_late(); if (rl) return rl; }
    HIP_TRY(hipStreamSynchronize(e.stream));          // staging buffer may still be in flight
    if (n) {
        memcpy(h->stage_f32, unary, n * sizeof(float));
        HIP_TRY(hipMemcpyAsync(e.unary_own, h->stage_f32, n * sizeof(float), hipMemcpyHostToDevice, e.stream));
    }
    e.bind_unary(e.unary_own);
    return LCCRF_OK;
}

int lccrf_set_unary_from_label(lccrf_handle h, const int16_t *label, const float *conf)
{
    CHECK_H(h);
    if ((!label && h->N) || !conf) return fail(LCCRF_E_INVALID, "label/conf is NULL");
    Engine &e = h->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    if (e.L < 2) return fail(LCCRF_E_INVALID, "setUnaryEnergyFromLabel needs >= 2 labels");
    if (h->label_stage_busy) HIP_TRY(hipStreamSynchronize(e.stream));   // an earlier call's kernel may still read the staging buffer
    // No uploads: the 2L+1 energies travel as a kernel argument and the kernel reads the labels from
    // pinned host memory (each tiny DMA command costs ~10 us of stream time; this path is latency-bound).
    if (h->N) memcpy(h->stage_i16, label, (size_t)h->N * sizeof(int16_t));
    const int16_t *src = h->stage_i16;
    if (h->N > kObjectPinnedMaxPoints) {                  // (large frames: many kernels, thousands of wavefronts -- see lccrf_add_pairwise)
        HIP_TRY(hipMemcpyAsync(e.label_own, h->stage_i16, (size_t)h->N * sizeof(int16_t), hipMemcpyHostToDevice, e.stream));
        src = e.label_own;
    }
    e.defer_unary_from_label(src, conf);                  // launched (or folded into the frame kernel) by the first consumer
    h->label_stage_busy = true;
    return LCCRF_OK;
}

int lccrf_add_pairwise(lccrf_handle h, const float *features, int d, float w)
{
    CHECK_H(h);
    if (!features && h->N) return fail(LCCRF_E_INVALID, "features is NULL");
    Engine &e = h->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    int rc = e.add_kernel(d, w, true, true);
    if (rc) return rc;
    KernelState &ks = e.kernels.back();
    const size_t n = (size_t)h->N * d;
    if (n) memcpy(ks.feat_stage, features, n * sizeof(float));   // caller may free `features` right away
    // SLAM frames: the build reads the features once, straight from this pinned buffer (no upload command on a latency-bound path).
    // Frames beyond the one-launch kernel are built by a dozen kernels of thousands of wavefronts, several of which read the
    // features -- in locality mode as a gather -- and every one of which reads the point count: over PCIe that cost a 100 000-point
    // frame 0.36 ms (C5 through this API: 1.61 -> 1.25 ms host to host), so those are uploaded once.
    ks.dev.feat = ks.feat_stage;
    if (h->N > kObjectPinnedMaxPoints && n) {
        HIP_TRY(hipMemcpyAsync(ks.feat_own, ks.feat_stage, n * sizeof(float), hipMemcpyHostToDevice, e.stream));
        ks.dev.feat = ks.feat_own;
    }
    e.sync_views();
    // The lattice is built lazily, together with any other pending kernel, by the first call that
    // needs it (inference, a step, a parity probe): one launch builds all of them side by side.
    e.sizes_known = false;
    return LCCRF_OK;
}

int lccrf_add_appearance_kernel(lccrf_handle h, float w, const float *vobserv, const float *verror,
                                float sd_observ, float sd_error)
{
    CHECK_H(h);
    if ((!vobserv || !verror) && h->N) return fail(LCCRF_E_INVALID, "vobserv/verror is NULL");
    std::vector<float> f((size_t)h->N * 2 + 1);
    for (int i = 0; i < h->N; ++i) {                  // pairwise3d.h:41-44
        f[2 * i + 0] = vobserv[i] / sd_observ;
        f[2 * i + 1] = verror[i] / sd_error;
    }
    return lccrf_add_pairwise(h, f.data(), 2, w);
}

int lccrf_add_smooth_kernel(lccrf_handle h, float w, const float *xy, float sd2d)
{
    CHECK_H(h);
    if (!xy && h->N) return fail(LCCRF_E_INVALID, "xy is NULL");
    std::vector<float> f((size_t)h->N * 2 + 1);
    for (int i = 0; i < h->N; ++i) {                  // pairwise3d.h:64-66
        f[2 * i + 0] = xy[2 * i + 0] / sd2d;
        f[2 * i + 1] = xy[2 * i + 1] / sd2d;
    }
    return lccrf_add_pairwise(h, f.data(), 2, w);
}

int lccrf_start_inference(lccrf_handle h)
{
    CHECK_H(h);
    return h->eng.start();
}

int lccrf_step_inference(lccrf_handle h, float relax)
{
    CHECK_H(h);
    return h->eng.step(relax);
}

int lccrf_build_map(lccrf_handle h)
{
    CHECK_H(h);
    { int rl = h->eng.resolve_late(); if (rl) return rl; }
    launch_map(h->eng.crf, h->eng.stream);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

int lccrf_inference(lccrf_handle h, int n_iterations, int with_map, float relax)
{
    CHECK_H(h);
    return h->eng.inference(n_iterations, with_map, relax);
}

// section 1h (the argument checks come first: they need no handle and no device)
int lccrf_inference_converged(lccrf_handle h, int max_iterations, int criterion, float tol, int with_map, float relax)
{
    const int ra = Engine::check_converged_args(max_iterations, criterion, tol, relax);
    if (ra) return ra;
    CHECK_H(h);
    return h->eng.inference_converged(converged_run(max_iterations, criterion, tol, with_map, relax));
}

// section 1i
int lccrf_run_converged(lccrf_handle h, int max_iterations, int criterion, float tol, int with_map, float relax)
{
    const int ra = Engine::check_converged_args(max_iterations, criterion, tol, relax);
    if (ra) return ra;
    CHECK_H(h);
    return h->eng.run_converged(converged_run(max_iterations, criterion, tol, with_map, relax));
}

int lccrf_get_convergence(lccrf_handle h, int *iterations, float *delta, int *changed, int *converged)
{
    CHECK_H(h);
    Engine &e = h->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    const int rc = e.read_convergence();
    if (rc) return rc;
    if (iterations) *iterations = e.conv_host[0];
    if (delta) memcpy(delta, e.conv_host + e.Fcap, sizeof(float));
    if (changed) *changed = e.conv_host[2 * (size_t)e.Fcap];
    if (converged) *converged = e.conv_host[3 * (size_t)e.Fcap];
    return LCCRF_OK;
}

int lccrf_get_engine(lccrf_handle h, int *engine, int *shape)
{
    if (!h || !engine) return fail(LCCRF_E_INVALID, "handle / engine is NULL");
    if (h->eng.run_pending()) {                         // (a frame that did not fit the one-launch kernel reports what it was re-run on)
        CHECK_H(h);
        int rl = h->eng.resolve_late();
        if (rl) return rl;
    }
    const Engine::RunReport &r = h->eng.report;
    *engine = r.engine;
    if (shape) *shape = (r.engine == 2 || r.engine == 4 || r.engine == 5 || r.engine == 6) ? r.shape : 0;
    return LCCRF_OK;
}

int lccrf_get_map(lccrf_handle h, int16_t *map_out)
{
    CHECK_H(h);
    if (!map_out && h->N) return fail(LCCRF_E_INVALID, "map_out is NULL");
    Engine &e = h->eng;
    if (e.take_labels(map_out, h->N)) return LCCRF_OK;   // one frame in flight, its labels go straight into map_pin: taken as they land
    bool seen_done = false;
    { int rl = e.resolve_late(&seen_done); if (rl) return rl; }
    if (e.crf.map != h->map_pin) {                        // device labels (lccrf_device_buffers): a copy through the pinned array
        if (h->N) HIP_TRY(hipMemcpyAsync(h->map_pin, e.crf.map, (size_t)h->N * sizeof(int16_t), hipMemcpyDeviceToHost, e.stream));
        seen_done = false;
    }
    if (!seen_done) HIP_TRY(hipStreamSynchronize(e.stream));
    if (h->N) memcpy(map_out, h->map_pin, (size_t)h->N * sizeof(int16_t));   // written there by the kernels
    if (seen_done) e.done_seen();
    return LCCRF_OK;
}

static int copy_out_f32(lccrf_handle h, const float *dev, float *out, size_t n)
{
    Engine &e = h->eng;
    if (n) HIP_TRY(hipMemcpyAsync(h->stage_f32, dev, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    if (n) memcpy(out, h->stage_f32, n * sizeof(float));
    return LCCRF_OK;
}

int lccrf_get_probability(lccrf_handle h, float *prob_out)
{
    CHECK_H(h);
    if (!prob_out && h->N) return fail(LCCRF_E_INVALID, "prob_out is NULL");
    { int rl = h->eng.resolve_late(); if (rl) return rl; }
    return copy_out_f32(h, h->eng.crf.Q, prob_out, (size_t)h->N * h->eng.L);
}

// ---- the reference's plug-in points: PairwisePotential::apply and DenseCRF's protected virtuals -------------------------------
// One body per operation, shared by the host-array form (on the handle's io buffers) and the device-array form (section 1b): settle
// a pending inference, make the handle ready, then enqueue the kernel on the handle's stream (nothing for a handle of 0 points).
static int pairwise_apply_on(lccrf_crf *h, int kernel, float *d_out, const float *d_in, int accumulate)
{
    Engine &e = h->eng;
    const int rc = e.make_ready(Engine::kSettled | Engine::kCallerOrder | Engine::kSized | Engine::kStepViews);   // (builds staged lattices)
    if (rc || !h->N) return rc;
    launch_filter(e.step_kdevs()[kernel], e.crf, e.maxV[kernel], d_in, d_out, accumulate, e.stream, 0, nullptr, e.model.compat_ptr[kernel],
                  e.model.pre_arg() ? e.model.pre_arg()[kernel] : nullptr);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

static int exp_and_normalize_on(lccrf_crf *h, float *d_out, const float *d_in, float scale, float relax)
{
    const int rc = h->eng.resolve_late();
    if (rc || !h->N) return rc;
    launch_exp_and_normalize(h->eng.crf, d_in, d_out, scale, relax, h->eng.stream);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

static int step_init_on(lccrf_crf *h, float *d_next)
{
    Engine &e = h->eng;
    if (!e.unary_set) return fail(LCCRF_E_STATE, "unary energies not set");
    const int rc = e.make_ready(Engine::kSettled | Engine::kCallerOrder | Engine::kUnaries);
    if (rc || !h->N) return rc;
    launch_step_init(e.crf, d_next, e.stream);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

static int map_of_on(lccrf_crf *h, const float *d_prob, int16_t *d_map)
{
    const int rc = h->eng.resolve_late();
    if (rc || !h->N) return rc;
    launch_map_of(h->eng.crf, d_prob, d_map, h->eng.stream);
    HIP_TRY(hipGetLastError());
    return LCCRF_OK;
}

// host forms: the caller's `in` (and `out`, where the kernel reads it) -> the handle's io buffers io_a (io_b), behind everything
// queued on its stream; a result -> the caller's array
static int io_in(Engine &e, const void *in, const void *out, size_t bytes)
{
    const int rc = e.need_io();
    if (rc || !bytes) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));
    HIP_TRY(hipMemcpy(e.io_a, in, bytes, hipMemcpyHostToDevice));
    if (out) HIP_TRY(hipMemcpy(e.io_b, out, bytes, hipMemcpyHostToDevice));
    return LCCRF_OK;
}

static int io_out(Engine &e, void *out, const void *d_src, size_t bytes)
{
    if (!bytes) return LCCRF_OK;
    HIP_TRY(hipStreamSynchronize(e.stream));
    HIP_TRY(hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
    return LCCRF_OK;
}

int lccrf_pairwise_apply(lccrf_handle h, int kernel, float *out_values, const float *in_values)
{
    CHECK_H(h);
    CHECK_K(h, kernel);
    if ((!out_values || !in_values) && h->N) return fail(LCCRF_E_INVALID, "out_values / in_values is NULL");
    Engine &e = h->eng;
    const size_t n = (size_t)h->N * e.L * sizeof(float);
    int rc = io_in(e, in_values, out_values, n);          // (the filter adds to out)
    if (!rc) rc = pairwise_apply_on(h, kernel, e.io_b, e.io_a, 1);
    return rc ? rc : io_out(e, out_values, e.io_b, n);
}

int lccrf_exp_and_normalize(lccrf_handle h, float *out, const float *in, float scale, float relax)
{
    CHECK_H(h);
    if ((!out || !in) && h->N) return fail(LCCRF_E_INVALID, "out / in is NULL");
    Engine &e = h->eng;
    const size_t n = (size_t)h->N * e.L * sizeof(float);
    int rc = io_in(e, in, relax != 1.0f ? out : nullptr, n);   // the blend reads the old out (densecrf3d.h:91-94)
    if (!rc) rc = exp_and_normalize_on(h, e.io_b, e.io_a, scale, relax);
    return rc ? rc : io_out(e, out, e.io_b, n);
}

int lccrf_step_init(lccrf_handle h, float *next_out)
{
    CHECK_H(h);
    if (!next_out && h->N) return fail(LCCRF_E_INVALID, "next_out is NULL");
    Engine &e = h->eng;
    int rc = e.need_io();
    if (!rc) rc = step_init_on(h, e.io_a);
    return rc ? rc : io_out(e, next_out, e.io_a, (size_t)h->N * e.L * sizeof(float));
}

int lccrf_map_of(lccrf_handle h, const float *prob, int16_t *map_out)
{
    CHECK_H(h);
    if ((!prob || !map_out) && h->N) return fail(LCCRF_E_INVALID, "prob / map_out is NULL");
    Engine &e = h->eng;
    int rc = io_in(e, prob, nullptr, (size_t)h->N * e.L * sizeof(float));
    if (!rc) rc = map_of_on(h, e.io_a, e.io_map);
    return rc ? rc : io_out(e, map_out, e.io_map, (size_t)h->N * sizeof(int16_t));
}

int lccrf_lattice_filter(int device_id, const float *features, int n_points, int d, const float *in, int value_size,
                         float *out, int *n_vertices)
{
    if (n_points < 0) return fail(LCCRF_E_INVALID, "n_points < 0");
    if ((!features || !in || !out) && n_points) return fail(LCCRF_E_INVALID, "features / in / out is NULL");
    if (d < 1 || d > LCCRF_MAX_DIMS) return fail(LCCRF_E_INVALID, "feature dims %d not in [1,%d]", d, LCCRF_MAX_DIMS);
    lccrf_handle h = nullptr;
    int rc = lccrf_create(&h, device_id, n_points, value_size);        // value_size plays the part of the label count
    if (rc) return rc;
    Engine &e = h->eng;
    const size_t n = (size_t)n_points * value_size * sizeof(float);
    rc = lccrf_add_pairwise(h, features, d, 1.0f);
    if (!rc) rc = io_in(e, in, nullptr, n);
    if (!rc) rc = pairwise_apply_on(h, 0, e.io_b, e.io_a, 0);
    if (!rc) rc = io_out(e, out, e.io_b, n);
    if (!rc && n_vertices) *n_vertices = e.V_host[0];
    lccrf_destroy(h);
    return rc;
}

int lccrf_get_lattice_size(lccrf_handle h, int kernel, int *n_vertices)
{
    CHECK_H(h);
    CHECK_K(h, kernel);
    if (!n_vertices) return fail(LCCRF_E_INVALID, "n_vertices is NULL");
    { int rcf = h->eng.make_ready(Engine::kBuilt); if (rcf) return rcf; }
    HIP_TRY(hipStreamSynchronize(h->eng.stream));
    *n_vertices = h->eng.V_host[(size_t)kernel * h->eng.Fcap];
    return LCCRF_OK;
}

int lccrf_get_norm(lccrf_handle h, int kernel, float *norm_out)
{
    CHECK_H(h);
    CHECK_K(h, kernel);
    if (!norm_out && h->N) return fail(LCCRF_E_INVALID, "norm_out is NULL");
    { int rc = h->eng.make_ready(Engine::kCallerOrder | Engine::kBuilt); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(h->eng.stream));
    if (h->N) HIP_TRY(hipMemcpy(norm_out, h->eng.kernels[kernel].dev.norm, (size_t)h->N * sizeof(float), hipMemcpyDeviceToHost));
    return LCCRF_OK;
}

int lccrf_get_lattice(lccrf_handle h, int kernel, int32_t *offset_out, float *bary_out, int32_t *nbr_out)
{
    CHECK_H(h);
    CHECK_K(h, kernel);
    Engine &e = h->eng;
    { int rc = e.make_ready(Engine::kCallerOrder | Engine::kBuilt); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(e.stream));
    const KernelDev &k = e.kernels[kernel].dev;
    const size_t ne = (size_t)h->N * k.D1;
    if (offset_out && ne) HIP_TRY(hipMemcpy(offset_out, k.offset, ne * sizeof(int), hipMemcpyDeviceToHost));
    if (bary_out && ne) HIP_TRY(hipMemcpy(bary_out, k.bary, ne * sizeof(float), hipMemcpyDeviceToHost));
    if (nbr_out) {
        const int V = e.V_host[(size_t)kernel * e.Fcap];
        for (int j = 0; j < k.D1 && V; ++j)           // device rows are strided by Epad, output by V
            HIP_TRY(hipMemcpy(nbr_out + (size_t)j * V * 2, k.nbr + (size_t)j * k.Epad * 2, (size_t)V * 2 * sizeof(int),
                              hipMemcpyDeviceToHost));
    }
    return LCCRF_OK;
}

int lccrf_get_unary(lccrf_handle h, float *unary_out)
{
    CHECK_H(h);
    if (!unary_out && h->N) return fail(LCCRF_E_INVALID, "unary_out is NULL");
    // (kCallerOrder: energies derived from labels live in the lattices' point order)
    { int rc = h->eng.make_ready(Engine::kSettled | Engine::kCallerOrder | Engine::kUnaries); if (rc) return rc; }
    return copy_out_f32(h, h->eng.crf.unary, unary_out, (size_t)h->N * h->eng.L);
}

// --------------------------------------------------------------------------------------
// object API on device arrays (include/lccrf.h section 1b)
// --------------------------------------------------------------------------------------
static int check_device_array(const lccrf_crf *h, const void *p, size_t bytes, const char *what)
{
    return check_device_array(h->eng, p, bytes, what);
}

// the caller's features [N][d] (copy) or an image (position / RGB) -> a new term's own feature buffer, on the handle's stream
static int add_kernel_staged(lccrf_crf *h, int d, float w, const void *src, int mode, int width, float posdev, float featuredev)
{
    Engine &e = h->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    int rc = e.add_kernel(d, w, true, false);
    if (rc) return rc;
    KernelState &ks = e.kernels.back();
    launch_stage_features(ks.feat_own, src, h->N, d, mode, width, posdev, featuredev, e.stream);
    HIP_TRY(hipGetLastError());
    ks.dev.feat = ks.feat_own;
    e.sync_views();
    e.sizes_known = false;                               // (built lazily with any other pending term, as by lccrf_add_pairwise)
    return LCCRF_OK;
}

int lccrf_get_stream(lccrf_handle h, void **stream)
{
    if (!h || !stream) return fail(LCCRF_E_INVALID, "handle / stream is NULL");
    *stream = (void *)h->eng.stream;
    return LCCRF_OK;
}

int lccrf_synchronize(lccrf_handle h)
{
    CHECK_H(h);
    { int rl = h->eng.resolve_late(); if (rl) return rl; }   // (settles a one-launch inference: its fallback re-run included)
    HIP_TRY(hipStreamSynchronize(h->eng.stream));
    return LCCRF_OK;
}

int lccrf_set_unary_device(lccrf_handle h, const float *d_unary)
{
    CHECK_H(h);
    Engine &e = h->eng;
    const size_t n = (size_t)h->N * e.L;
    { int rc = check_device_array(h, d_unary, n * sizeof(float), "d_unary"); if (rc) return rc; }
    { int rl = e.resolve_late(); if (rl) return rl; }
    if (n) HIP_TRY(hipMemcpyAsync(e.unary_own, d_unary, n * sizeof(float), hipMemcpyDefault, e.stream));
    e.bind_unary(e.unary_own);
    return LCCRF_OK;
}

int lccrf_set_unary_from_label_device(lccrf_handle h, const int16_t *d_label, const float *conf)
{
    CHECK_H(h);
    Engine &e = h->eng;
    if (!conf) return fail(LCCRF_E_INVALID, "conf is NULL");
    if (e.L < 2) return fail(LCCRF_E_INVALID, "setUnaryEnergyFromLabel needs >= 2 labels");
    { int rc = check_device_array(h, d_label, (size_t)h->N * sizeof(int16_t), "d_label"); if (rc) return rc; }
    // conf: n_labels host values -- or device values (the reference's GPU interface hands device pointers only), read here
    float cf[LCCRF_MAX_LABELS];
    hipPointerAttribute_t a{};
    const hipError_t ea = hipPointerGetAttributes(&a, conf);
    (void)hipGetLastError();
    if (ea == hipSuccess && !a.isManaged && a.type == hipMemoryTypeDevice) {
        if (a.device != e.device) return fail(LCCRF_E_INVALID, "conf (%p) is memory of device %d, the handle's is device %d", conf, a.device, e.device);
        { int rc = check_device_array(h, conf, (size_t)e.L * sizeof(float), "conf"); if (rc) return rc; }
        HIP_TRY(hipMemcpy(cf, conf, (size_t)e.L * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        memcpy(cf, conf, (size_t)e.L * sizeof(float));
    }
    { int rl = e.resolve_late(); if (rl) return rl; }
    // enqueued now (not deferred like the host path's labels): the caller's array is read by this kernel only.  The energies go in
    // the caller's point order whatever the lattices' order -- they are raw unaries from here on (permuted like lccrf_set_unary's).
    CrfDev c = e.crf;
    c.unary = e.unary_own;
    c.perm = nullptr;
    if (h->N) {
        launch_unary_from_label_tbl(c, d_label, e.label_table(cf), e.stream);
        HIP_TRY(hipGetLastError());
    }
    e.bind_unary(e.unary_own);
    return LCCRF_OK;
}

int lccrf_add_pairwise_device(lccrf_handle h, const float *d_features, int d, float w)
{
    CHECK_H(h);
    if (d < 1 || d > LCCRF_MAX_DIMS) return fail(LCCRF_E_INVALID, "feature dims %d not in [1,%d]", d, LCCRF_MAX_DIMS);
    { int rc = check_device_array(h, d_features, (size_t)h->N * d * sizeof(float), "d_features"); if (rc) return rc; }
    return add_kernel_staged(h, d, w, d_features, kStageCopy, 1, 1.0f, 1.0f);
}

int lccrf_add_image_kernel(lccrf_handle h, int width, int height, float w, float posdev, const void *d_image, int image_format,
                           float featuredev)
{
    CHECK_H(h);
    if (width < 0 || height < 0 || (long)width * height != h->N)
        return fail(LCCRF_E_INVALID, "width * height (%d x %d) must equal the handle's n_points (%d)", width, height, h->N);
    if (!(posdev > 0.0f) || !std::isfinite(posdev)) return fail(LCCRF_E_INVALID, "posdev must be positive and finite");
    if (image_format == LCCRF_IMAGE_NONE) {
        if (d_image) return fail(LCCRF_E_INVALID, "LCCRF_IMAGE_NONE takes no image");
        return add_kernel_staged(h, 2, w, nullptr, kStagePosition, width, posdev, 1.0f);
    }
    if (image_format != LCCRF_IMAGE_U8 && image_format != LCCRF_IMAGE_F32)
        return fail(LCCRF_E_INVALID, "image_format %d is none of LCCRF_IMAGE_NONE / _U8 / _F32", image_format);
    if (!(featuredev > 0.0f) || !std::isfinite(featuredev)) return fail(LCCRF_E_INVALID, "featuredev must be positive and finite");
    const size_t elem = image_format == LCCRF_IMAGE_U8 ? 1 : sizeof(float);
    { int rc = check_device_array(h, d_image, (size_t)h->N * 3 * elem, "d_image"); if (rc) return rc; }
    return add_kernel_staged(h, 5, w, d_image, image_format == LCCRF_IMAGE_U8 ? kStageImageU8 : kStageImageF32, width, posdev,
                             featuredev);
}

int lccrf_device_buffers(lccrf_handle h, const float **d_unary, float **d_current, float **d_next, float **d_tmp, int16_t **d_map)
{
    CHECK_H(h);
    Engine &e = h->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    if (d_tmp) { int rc = e.need_io(); if (rc) return rc; }
    if (e.crf.map != h->map_dev) {                       // from now on the labels are written to HBM (map_host stays: no pinned fast path)
        if (h->N) HIP_TRY(hipMemcpyAsync(h->map_dev, h->map_pin, (size_t)h->N * sizeof(int16_t), hipMemcpyHostToDevice, e.stream));
        e.crf.map = h->map_dev;
    }
    if (d_unary) *d_unary = e.unary_own;
    if (d_current) *d_current = e.crf.Q;
    if (d_next) *d_next = e.crf.next;
    if (d_tmp) *d_tmp = e.io_b;
    if (d_map) *d_map = h->map_dev;
    return LCCRF_OK;
}

int lccrf_pairwise_apply_device(lccrf_handle h, int kernel, float *d_out, const float *d_in)
{
    CHECK_H(h);
    CHECK_K(h, kernel);
    const size_t n = (size_t)h->N * h->eng.L * sizeof(float);
    { int rc = check_device_array(h, d_out, n, "d_out"); if (rc) return rc; }
    { int rc = check_device_array(h, d_in, n, "d_in"); if (rc) return rc; }
    return pairwise_apply_on(h, kernel, d_out, d_in, 1);
}

int lccrf_exp_and_normalize_device(lccrf_handle h, float *d_out, const float *d_in, float scale, float relax)
{
    CHECK_H(h);
    const size_t n = (size_t)h->N * h->eng.L * sizeof(float);
    { int rc = check_device_array(h, d_out, n, "d_out"); if (rc) return rc; }
    { int rc = check_device_array(h, d_in, n, "d_in"); if (rc) return rc; }
    return exp_and_normalize_on(h, d_out, d_in, scale, relax);
}

int lccrf_step_init_device(lccrf_handle h, float *d_next)
{
    CHECK_H(h);
    const size_t n = (size_t)h->N * h->eng.L * sizeof(float);
    { int rc = check_device_array(h, d_next, n, "d_next"); if (rc) return rc; }
    return step_init_on(h, d_next);
}

int lccrf_map_of_device(lccrf_handle h, const float *d_prob, int16_t *d_map)
{
    CHECK_H(h);
    { int rc = check_device_array(h, d_prob, (size_t)h->N * h->eng.L * sizeof(float), "d_prob"); if (rc) return rc; }
    { int rc = check_device_array(h, d_map, (size_t)h->N * sizeof(int16_t), "d_map"); if (rc) return rc; }
    return map_of_on(h, d_prob, d_map);
}

}  // extern "C"

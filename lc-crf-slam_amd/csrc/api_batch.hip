// api_batch.hip -- the batch API of include/lccrf.h: section 2 and the batch calls of section 5; its gradients (2c, 2d, 2h) are in
// api_backward.hip, its weights, matrices and modes (2c, 2g) and its plans in api_model.hip.
//
// Argument checks, the three input paths with their pinned staging, the timed calls and the read-backs of one batch; the state
// machine behind it is the Engine (host_engine.h).
#include "api_common.h"

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

using namespace lccrf;

namespace {

// caller's arrays -> pinned staging by a few host threads (one core copies ~10 GB/s, the link takes ~55): a small process-wide pool
// of workers that sleep between batches; the calling thread takes its share of the chunks too.
class CopyPool {
public:
    struct Job { char *dst; const char *src; size_t bytes; };
    // Never throws (it sits under an extern "C" entry point): if a worker thread or the chunk list cannot be created
    // (std::system_error, std::bad_alloc) the calling thread copies the arrays itself.
    void run(const std::vector<Job> &arrays, int max_threads) noexcept
    {
        try {
            run_pooled(arrays, max_threads);
        } catch (...) {
            {
                std::lock_guard<std::mutex> g(m_);         // (nothing was published: the throwing statements come before jobs_ is set)
                jobs_ = nullptr;
            }
            for (const Job &j : arrays) memcpy(j.dst, j.src, j.bytes);
        }
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }

private:
    void run_pooled(const std::vector<Job> &arrays, int max_threads)
    {
        constexpr size_t kChunk = (size_t)512 << 10;
        std::vector<Job> chunks;
        size_t total = 0;
        for (const Job &j : arrays)
            for (size_t lo = 0; lo < j.bytes; lo += kChunk) {
                chunks.push_back({j.dst + lo, j.src + lo, std::min(kChunk, j.bytes - lo)});
                total += chunks.back().bytes;
            }
        const int want = (int)std::min<size_t>((size_t)std::max(max_threads, 1), (total + 4 * kChunk - 1) / (4 * kChunk));
        if (want <= 1 || chunks.size() < 2) {
            for (const Job &c : chunks) memcpy(c.dst, c.src, c.bytes);
            return;
        }
        std::unique_lock<std::mutex> lk(m_);
        while ((int)workers_.size() < want - 1) workers_.emplace_back([this] { worker(); });
        jobs_ = &chunks;
        next_ = 0;
        left_ = chunks.size();
        helpers_ = want - 1;
        ++epoch_;
        lk.unlock();
        cv_.notify_all();
        take();                                            // the caller works too
        lk.lock();
        done_.wait(lk, [this] { return left_ == 0 && busy_ == 0; });
        jobs_ = nullptr;
    }
    void take()
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            if (!jobs_ || next_ >= jobs_->size()) return;
            const Job c = (*jobs_)[next_++];
            lk.unlock();
            memcpy(c.dst, c.src, c.bytes);
            lk.lock();
            if (--left_ == 0) done_.notify_all();
        }
    }
    void worker()
    {
        unsigned long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return stop_ || (epoch_ != seen && helpers_ > 0); });
            if (stop_) return;
            seen = epoch_;
            --helpers_;
            ++busy_;
            lk.unlock();
            take();
            lk.lock();
            if (--busy_ == 0 && left_ == 0) done_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> workers_;
    const std::vector<Job> *jobs_ = nullptr;
    size_t next_ = 0, left_ = 0;
    int helpers_ = 0, busy_ = 0;
    unsigned long epoch_ = 0;
    bool stop_ = false;
};
// One pool (and one staging lock) per DEVICE: a host with one thread per GPU (tools/replay_multi.cpp) stages its ranks' batches side by
// side instead of queueing all of them behind one pool's workers; handles of one device still stage one at a time.
constexpr int kCopyPools = 16;
CopyPool g_copy_pool[kCopyPools];
std::mutex g_copy_pool_user[kCopyPools];

template <typename T>
int pinned_plain(Arena &mem, T **out, size_t count)      // ordinary (cached, DMA-friendly) pinned memory owned by the arena
{
    void *p = nullptr;
    HIP_TRY(hipHostMalloc(&p, (count ? count : 1) * sizeof(T), hipHostMallocDefault));
    mem.pinned.push_back(p);
    *out = static_cast<T *>(p);
    return LCCRF_OK;
}
}  // namespace

extern "C" {

// --------------------------------------------------------------------------------------
// batch API
// --------------------------------------------------------------------------------------
int lccrf_batch_create(lccrf_batch_handle *out, int device_id, const lccrf_batch_desc *desc)
{
    if (!out || !desc) return fail(LCCRF_E_INVALID, "out/desc is NULL");
    *out = nullptr;
    if (desc->max_frames < 1 || desc->max_points < 0) return fail(LCCRF_E_INVALID, "max_frames < 1 or max_points < 0");
    if (desc->n_labels < 1 || desc->n_labels > LCCRF_MAX_LABELS) return fail(LCCRF_E_INVALID, "n_labels out of range");
    if (desc->n_kernels < 0 || desc->n_kernels > LCCRF_MAX_KERNELS) return fail(LCCRF_E_INVALID, "n_kernels out of range");
    for (int k = 0; k < desc->n_kernels; ++k)
        if (desc->feat_dims[k] < 1 || desc->feat_dims[k] > LCCRF_MAX_DIMS)
            return fail(LCCRF_E_INVALID, "feat_dims[%d] = %d not in [1,%d]", k, desc->feat_dims[k], LCCRF_MAX_DIMS);
    int rc = use_device(device_id);
    if (rc) return rc;
    lccrf_batch *b = new (std::nothrow) lccrf_batch;
    if (!b) return fail(LCCRF_E_NOMEM, "host allocation failed");
    b->desc = *desc;
    b->eng.allow_perm = true;
    b->eng.batch_owned = true;
    b->eng.opt = Engine::Options::fresh();
    rc = b->eng.init(device_id, desc->max_frames, desc->max_points, desc->n_labels);
    for (int k = 0; k < desc->n_kernels && !rc; ++k) rc = b->eng.add_kernel(desc->feat_dims[k], desc->weights[k], true, false);
    if (!rc && hipStreamSynchronize(b->eng.stream) != hipSuccess)      // every allocation is zeroed before the handle is handed out
        rc = fail(LCCRF_E_HIP, "hipStreamSynchronize after allocation failed");
    if (rc) {
        b->eng.destroy();
        delete b;
        return rc;
    }
    *out = b;
    return LCCRF_OK;
}

void lccrf_batch_destroy(lccrf_batch_handle b)
{
    if (!b) return;
    (void)hipSetDevice(b->eng.device);
    if (b->pipe.up) (void)hipStreamSynchronize(b->pipe.up);
    if (b->pipe.down) (void)hipStreamSynchronize(b->pipe.down);
    b->eng.destroy();
    b->pipe.destroy();
    delete b;
}

int lccrf_batch_set_option(lccrf_batch_handle b, int option, int value)
{
    if (!b) return fail(LCCRF_E_INVALID, "handle is NULL");
    if (option == LCCRF_OPT_COPY_THREADS) {
        if (value < 1 || value > 64) return fail(LCCRF_E_INVALID, "LCCRF_OPT_COPY_THREADS takes 1 .. 64");
        b->pipe.copy_threads = value;
        return LCCRF_OK;
    }
    if (option == LCCRF_OPT_EVENT_TIMING) {
        b->eng.opt.event_timing = value != 0;
        if (!value) b->eng.timed_build = b->eng.timed_inf = false;
        return LCCRF_OK;
    }
    return apply_option(b->eng, option, value);
}

// The three batch-input entry points (lccrf_batch_set_inputs_host, _host_async, lccrf_batch_bind_inputs_device) run one sequence:
// (a) every argument check, with nothing touched yet -- a rejected call leaves the previous inputs bound and usable; (b) settle what
// the previous batch left pending and reset the batch; (c) the path's own copies; (d) batch_bind_inputs.
// n_points: the caller's host counts, checked against max_points (*active: the largest), or null for counts on the device.
static int batch_begin_inputs(lccrf_batch *b, int n_frames, const int32_t *n_points, bool have_unary, bool have_label,
                              const float *conf, int flags, const float *const *features, const char *features_name, int *active)
{
    Engine &e = b->eng;
    if (n_frames < 1 || n_frames > e.Fcap) return fail(LCCRF_E_CAPACITY, "n_frames %d not in [1,%d]", n_frames, e.Fcap);
    if (have_unary == have_label) return fail(LCCRF_E_INVALID, "exactly one of unary / label must be given");
    if (have_label && (!conf || e.L < 2)) return fail(LCCRF_E_INVALID, "label input needs conf[n_labels] and >= 2 labels");
    if (flags & ~LCCRF_HOST_PINNED) return fail(LCCRF_E_INVALID, "unknown flags 0x%x", flags);
    for (int k = 0; k < b->desc.n_kernels; ++k)
        if (!features[k]) return fail(LCCRF_E_INVALID, "%s[%d] is NULL", features_name, k);
    *active = 0;
    for (int f = 0; n_points && f < n_frames; ++f) {
        if (n_points[f] < 0 || n_points[f] > e.maxN) return fail(LCCRF_E_CAPACITY, "n_points[%d]=%d not in [0,%d]", f, n_points[f], e.maxN);
        *active = std::max(*active, n_points[f]);
    }
    { int rl = e.resolve_late(); if (rl) return rl; }
    e.F = n_frames;
    e.sync_views();
    e.forget_inputs();
    b->inputs_set = false;
    return LCCRF_OK;
}

// (d): bind the unaries (or the labels they are derived from) and the features -- the caller's device arrays, or with
// features == null the batch's own copies -- and publish the new inputs
static void batch_bind_inputs(lccrf_batch *b, int active, const float *unary, const int16_t *label, const float *conf,
                              const float *const *features)
{
    Engine &e = b->eng;
    e.activeN = active;
    e.crf.n_points = e.npoints_own;
    if (unary) e.bind_unary(unary);
    else e.defer_unary_from_label(label, conf);
    for (int k = 0; k < b->desc.n_kernels; ++k) e.kernels[k].dev.feat = features ? features[k] : e.kernels[k].feat_own;
    e.sync_views();
    b->inputs_set = true;
}

int lccrf_batch_set_inputs_host(lccrf_batch_handle b, int n_frames, const int32_t *n_points, const float *unary,
                                const int16_t *label, const float *conf, const float *const *features)
{
    CHECK_H(b);
    if (!n_points) return fail(LCCRF_E_INVALID, "n_points is NULL");
    if (b->desc.n_kernels && !features) return fail(LCCRF_E_INVALID, "features is NULL");
    int active = 0;
    int rc = batch_begin_inputs(b, n_frames, n_points, unary != nullptr, label != nullptr, conf, 0, features, "features", &active);
    if (rc) return rc;
    Engine &e = b->eng;
    HIP_TRY(hipStreamSynchronize(e.stream));
    HIP_TRY(hipMemcpy(e.npoints_own, n_points, sizeof(int) * n_frames, hipMemcpyHostToDevice));
    const size_t per = (size_t)e.maxN;
    if (unary) HIP_TRY(hipMemcpy(e.unary_own, unary, sizeof(float) * n_frames * per * e.L, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy(e.label_own, label, sizeof(int16_t) * n_frames * per, hipMemcpyHostToDevice));
    for (int k = 0; k < b->desc.n_kernels; ++k) {
        const KernelState &ks = e.kernels[k];
        HIP_TRY(hipMemcpy(ks.feat_own, features[k], sizeof(float) * n_frames * per * ks.dev.d, hipMemcpyHostToDevice));
    }
    batch_bind_inputs(b, active, unary ? e.unary_own : nullptr, e.label_own, conf, nullptr);
    return LCCRF_OK;
}

static int pipe_refresh_after_rerun(void *ctx);

static int pipe_init(lccrf_batch *b)
{
    HostPipe &p = b->pipe;
    if (p.up) return LCCRF_OK;
    Engine &e = b->eng;
    e.after_rerun = pipe_refresh_after_rerun;
    e.after_rerun_ctx = b;
    HIP_TRY(hipStreamCreateWithFlags(&p.up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&p.down, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_up, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_down, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_q, hipEventDisableTiming));
    return LCCRF_OK;
}

int lccrf_batch_set_inputs_host_async(lccrf_batch_handle b, int n_frames, const int32_t *n_points, const float *unary,
                                      const int16_t *label, const float *conf, const float *const *features, int flags)
{
    CHECK_H(b);
    if (!n_points) return fail(LCCRF_E_INVALID, "n_points is NULL");
    if (b->desc.n_kernels && !features) return fail(LCCRF_E_INVALID, "features is NULL");
    int active = 0;
    int rc = batch_begin_inputs(b, n_frames, n_points, unary != nullptr, label != nullptr, conf, flags, features, "features", &active);
    if (rc) return rc;                                 // (this settled what the previous batch on this handle left pending)
    Engine &e = b->eng;
    HostPipe &p = b->pipe;
    if ((rc = pipe_init(b))) return rc;
    const bool direct = (flags & LCCRF_HOST_PINNED) != 0;
    const size_t per = (size_t)e.maxN, Fz = (size_t)n_frames, Fc = (size_t)e.Fcap;
    if (p.up_pending) {                                // the staging set is still the source of the previous upload (normally long done)
        HIP_TRY(hipEventSynchronize(p.ev_up));
        p.up_pending = false;
    }
    const float *src_un = unary;
    const int16_t *src_lb = label;
    std::vector<const float *> src_ft(features, features + b->desc.n_kernels);
    // (the point counts are always staged: a few bytes per frame, and the caller's array is usually a local one)
    if (!p.npoints && (rc = pinned_plain(e.mem, &p.npoints, Fc))) return rc;
    memcpy(p.npoints, n_points, sizeof(int) * Fz);
    if (!direct) {                                     // copy out of the caller's buffers before returning
        std::vector<CopyPool::Job> jobs;
        if (unary) {
            if (!p.unary && (rc = pinned_plain(e.mem, &p.unary, Fc * per * e.L))) return rc;
            jobs.push_back({(char *)p.unary, (const char *)unary, sizeof(float) * Fz * per * e.L});
            src_un = p.unary;
        } else {
            if (!p.label && (rc = pinned_plain(e.mem, &p.label, Fc * per))) return rc;
            jobs.push_back({(char *)p.label, (const char *)label, sizeof(int16_t) * Fz * per});
            src_lb = p.label;
        }
        p.feat.resize(b->desc.n_kernels, nullptr);
        for (int k = 0; k < b->desc.n_kernels; ++k) {
            const int d = e.kernels[k].dev.d;
            if (!p.feat[k] && (rc = pinned_plain(e.mem, &p.feat[k], Fc * per * d))) return rc;
            jobs.push_back({(char *)p.feat[k], (const char *)features[k], sizeof(float) * Fz * per * d});
            src_ft[k] = p.feat[k];
        }
        const int pool = (e.device >= 0 ? e.device : 0) % kCopyPools;
        std::lock_guard<std::mutex> g(g_copy_pool_user[pool]);
        g_copy_pool[pool].run(jobs, p.copy_threads);
    }
    // the upload waits for everything queued on the batch's stream so far (a kernel of the previous batch may still read the
    // device copies), and whatever is queued from here on waits for the upload
    HIP_TRY(hipEventRecord(p.ev_q, e.stream));
    HIP_TRY(hipStreamWaitEvent(p.up, p.ev_q, 0));
    HIP_TRY(hipMemcpyAsync(e.npoints_own, p.npoints, sizeof(int) * Fz, hipMemcpyHostToDevice, p.up));
    if (unary) HIP_TRY(hipMemcpyAsync(e.unary_own, src_un, sizeof(float) * Fz * per * e.L, hipMemcpyHostToDevice, p.up));
    else HIP_TRY(hipMemcpyAsync(e.label_own, src_lb, sizeof(int16_t) * Fz * per, hipMemcpyHostToDevice, p.up));
    for (int k = 0; k < b->desc.n_kernels; ++k) {
        const KernelState &ks = e.kernels[k];
        HIP_TRY(hipMemcpyAsync(ks.feat_own, src_ft[k], sizeof(float) * Fz * per * ks.dev.d, hipMemcpyHostToDevice, p.up));
    }
    HIP_TRY(hipEventRecord(p.ev_up, p.up));
    HIP_TRY(hipStreamWaitEvent(e.stream, p.ev_up, 0));
    p.up_pending = true;
    batch_bind_inputs(b, active, unary ? e.unary_own : nullptr, e.label_own, conf, nullptr);
    return LCCRF_OK;
}

int lccrf_batch_wait_inputs(lccrf_batch_handle b)
{
    CHECK_H(b);
    if (b->pipe.up_pending) {
        HIP_TRY(hipEventSynchronize(b->pipe.ev_up));
        b->pipe.up_pending = false;
    }
    return LCCRF_OK;
}

static int pipe_queue_download(lccrf_batch *b, hipStream_t on)
{
    Engine &e = b->eng;
    HostPipe &p = b->pipe;
    const size_t Fz = (size_t)p.down_frames, per = (size_t)e.maxN;
    if (p.down_what & LCCRF_DOWNLOAD_LABEL_BITS)
        HIP_TRY(hipMemcpyAsync(p.bits, e.crf.map_bits, sizeof(uint64_t) * Fz * e.crf.bits_stride, hipMemcpyDeviceToHost, on));
    if (p.down_what & LCCRF_DOWNLOAD_MAP)
        HIP_TRY(hipMemcpyAsync(p.map, e.crf.map, sizeof(int16_t) * Fz * per, hipMemcpyDeviceToHost, on));
    if (p.down_what & LCCRF_DOWNLOAD_PROBABILITY)
        HIP_TRY(hipMemcpyAsync(p.prob, e.crf.Q, sizeof(float) * Fz * per * e.L, hipMemcpyDeviceToHost, on));
    return LCCRF_OK;
}

// Engine::after_rerun of a batch with a download pipe: a queued download copied the results BEFORE the flagged frames were re-run
// (whoever settled them -- lccrf_batch_get_fallback_frames, _synchronize, the next batch's inputs, ...): queue the copies again behind
// the re-run on the batch's stream and move the "download landed" event there, so lccrf_batch_wait_download waits for the fresh ones.
static int pipe_refresh_after_rerun(void *ctx)
{
    lccrf_batch *b = static_cast<lccrf_batch *>(ctx);
    HostPipe &p = b->pipe;
    if (!p.down_pending) return LCCRF_OK;
    HIP_TRY(hipEventSynchronize(p.ev_down));           // (the first copies still own the pinned arrays)
    int rc = pipe_queue_download(b, b->eng.stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(p.ev_down, b->eng.stream));
    return LCCRF_OK;
}

int lccrf_batch_download_async(lccrf_batch_handle b, int what)
{
    CHECK_H(b);
    Engine &e = b->eng;
    HostPipe &p = b->pipe;
    if (!what || (what & ~(LCCRF_DOWNLOAD_LABEL_BITS | LCCRF_DOWNLOAD_MAP | LCCRF_DOWNLOAD_PROBABILITY)))
        return fail(LCCRF_E_INVALID, "what = 0x%x: a combination of LCCRF_DOWNLOAD_*", what);
    if ((what & LCCRF_DOWNLOAD_LABEL_BITS) && !e.crf.map_bits) return fail(LCCRF_E_INVALID, "label bits exist for n_labels == 2 only");
    int rc = pipe_init(b);
    if (rc) return rc;
    if (p.down_pending) {                              // (the host copies of the previous download are about to be overwritten)
        HIP_TRY(hipEventSynchronize(p.ev_down));
        p.down_pending = false;
    }
    const size_t Fc = (size_t)e.Fcap, per = (size_t)e.maxN;
    if ((what & LCCRF_DOWNLOAD_LABEL_BITS) && !p.bits && (rc = pinned_plain(e.mem, &p.bits, Fc * std::max(e.crf.bits_stride, 1)))) return rc;
    if ((what & LCCRF_DOWNLOAD_MAP) && !p.map && (rc = pinned_plain(e.mem, &p.map, Fc * per))) return rc;
    if ((what & LCCRF_DOWNLOAD_PROBABILITY) && !p.prob && (rc = pinned_plain(e.mem, &p.prob, Fc * per * e.L))) return rc;
    p.down_what = what;
    p.down_frames = e.F;
    // behind everything queued on the batch's stream (calls on a caller's stream are ordered into it when they return), on the
    // download stream; the batch's stream in turn waits for the copies before anything may overwrite the results
    HIP_TRY(hipEventRecord(p.ev_q, e.stream));
    HIP_TRY(hipStreamWaitEvent(p.down, p.ev_q, 0));
    if ((rc = pipe_queue_download(b, p.down))) return rc;
    HIP_TRY(hipEventRecord(p.ev_down, p.down));
    HIP_TRY(hipStreamWaitEvent(e.stream, p.ev_down, 0));
    p.down_pending = true;
    return LCCRF_OK;
}

int lccrf_batch_wait_download(lccrf_batch_handle b, const uint64_t **label_bits, int *words_per_frame, const int16_t **map,
                              const float **probability)
{
    CHECK_H(b);
    Engine &e = b->eng;
    HostPipe &p = b->pipe;
    if (!p.down_pending) return fail(LCCRF_E_STATE, "no download queued (lccrf_batch_download_async)");
    HIP_TRY(hipEventSynchronize(p.ev_down));
    // a one-launch run may have flagged frames that did not fit: they are re-run at the first synchronisation point behind the launch
    // -- here, or in any call made since lccrf_batch_download_async -- and the re-run queues the copies again (pipe_refresh_after_rerun)
    int rc = e.resolve_late();
    if (rc) { p.down_pending = false; return rc; }
    HIP_TRY(hipEventSynchronize(p.ev_down));           // (re-recorded behind a re-run; otherwise already complete)
    p.down_pending = false;
    if (label_bits) *label_bits = (p.down_what & LCCRF_DOWNLOAD_LABEL_BITS) ? p.bits : nullptr;
    if (words_per_frame) *words_per_frame = e.crf.bits_stride;
    if (map) *map = (p.down_what & LCCRF_DOWNLOAD_MAP) ? p.map : nullptr;
    if (probability) *probability = (p.down_what & LCCRF_DOWNLOAD_PROBABILITY) ? p.prob : nullptr;
    return LCCRF_OK;
}

int lccrf_batch_bind_inputs_device(lccrf_batch_handle b, int n_frames, const int32_t *d_n_points, const float *d_unary,
                                   const int16_t *d_label, const float *conf, const float *const *d_features)
{
    CHECK_H(b);
    if (!d_n_points) return fail(LCCRF_E_INVALID, "d_n_points is NULL");
    if (b->desc.n_kernels && !d_features) return fail(LCCRF_E_INVALID, "d_features is NULL");
    int active = 0;                                   // per-frame sizes live on the device: unknown here
    int rc = batch_begin_inputs(b, n_frames, nullptr, d_unary != nullptr, d_label != nullptr, conf, 0, d_features, "d_features", &active);
    if (rc) return rc;
    Engine &e = b->eng;
    // the kernels index every per-frame array with n_points[f]: work on a validated copy (clamped to
    // [0, max_points]; an out-of-range entry raises LCCRF_E_CAPACITY at the next synchronisation point)
    launch_validate_npoints(d_n_points, e.npoints_own, n_frames, e.maxN, e.npoints_bad, e.stream);
    HIP_TRY(hipGetLastError());
    batch_bind_inputs(b, active, d_unary, d_label, conf, d_features);
    return LCCRF_OK;
}

int lccrf_batch_build(lccrf_batch_handle b, void *stream)
{
    CHECK_H(b);
    if (!b->inputs_set) return fail(LCCRF_E_STATE, "inputs not set");
    Engine &e = b->eng;
    const int rc = timed_batch_call(e, stream, e.ev[0], e.ev[1], e.timed_build, [&] {
        const int rb = e.kernels.empty() ? LCCRF_OK : e.build_kernels(0, (int)e.kernels.size());
        e.built_upto = (int)e.kernels.size();
        return rb;
    });
    e.built = !rc;
    return rc;                                        // (kSized waits on the own stream, which ~StreamScope orders behind this one)
}

int lccrf_batch_inference(lccrf_batch_handle b, int n_iterations, int with_map, float relax, void *stream)
{
    CHECK_H(b);
    Engine &e = b->eng;
    if (!e.built) return fail(LCCRF_E_STATE, "lccrf_batch_build has not run for these inputs");
    int rc = e.make_ready(Engine::kSized);
    if (rc) return rc;
    return timed_batch_call(e, stream, e.ev[2], e.ev[3], e.timed_inf, [&] { return e.inference(n_iterations, with_map, relax); });
}

// section 2e (the argument checks come first: they need no handle and no device)
int lccrf_batch_inference_converged(lccrf_batch_handle b, int max_iterations, int criterion, float tol, int with_map, float relax,
                                    void *stream)
{
    const int ra = Engine::check_converged_args(max_iterations, criterion, tol, relax);
    if (ra) return ra;
    CHECK_H(b);
    Engine &e = b->eng;
    if (!e.built) return fail(LCCRF_E_STATE, "lccrf_batch_build has not run for these inputs");
    int rc = e.make_ready(Engine::kSized);
    if (rc) return rc;
    return timed_batch_call(e, stream, e.ev[2], e.ev[3], e.timed_inf,
                            [&] { return e.inference_converged(converged_run(max_iterations, criterion, tol, with_map, relax)); });
}

int lccrf_batch_get_convergence_host(lccrf_batch_handle b, int32_t *iterations, float *delta, int32_t *changed, int32_t *converged)
{
    CHECK_H(b);
    Engine &e = b->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    const int rc = e.read_convergence();              // waits for this batch's stream (a caller's stream is ordered into it), not the device
    if (rc) return rc;
    void *outs[4] = {iterations, delta, changed, converged};
    for (int a = 0; a < 4; ++a)
        if (outs[a]) memcpy(outs[a], e.conv_host + (size_t)a * e.Fcap, sizeof(int32_t) * (size_t)e.F);
    return LCCRF_OK;
}

int lccrf_batch_device_convergence(lccrf_batch_handle b, const int32_t **d_iterations, const float **d_delta, const int32_t **d_changed,
                                   const int32_t **d_converged)
{
    CHECK_H(b);
    { int rl = b->eng.resolve_late(); if (rl) return rl; }   // (section 2f: a pending one-launch run's flagged frames are re-run first)
    const ConvergeOut o = b->eng.conv_out();
    if (d_iterations) *d_iterations = o.iterations;
    if (d_delta) *d_delta = o.delta;
    if (d_changed) *d_changed = o.changed;
    if (d_converged) *d_converged = o.converged;
    return LCCRF_OK;
}

int lccrf_batch_run(lccrf_batch_handle b, int n_iterations, int with_map, float relax, void *stream)
{
    CHECK_H(b);
    if (!b->inputs_set) return fail(LCCRF_E_STATE, "inputs not set");
    Engine &e = b->eng;
    const int rc = timed_batch_call(e, stream, e.ev[2], e.ev[3], e.timed_inf, [&] { return e.run(n_iterations, with_map, relax); });
    e.built = e.built_upto == (int)e.kernels.size() && !e.kernels.empty();
    return rc;
}

// section 2f (the argument checks come first, as in 2e)
int lccrf_batch_run_converged(lccrf_batch_handle b, int max_iterations, int criterion, float tol, int with_map, float relax, void *stream)
{
    const int ra = Engine::check_converged_args(max_iterations, criterion, tol, relax);
    if (ra) return ra;
    CHECK_H(b);
    if (!b->inputs_set) return fail(LCCRF_E_STATE, "inputs not set");
    Engine &e = b->eng;
    const int rc = timed_batch_call(e, stream, e.ev[2], e.ev[3], e.timed_inf,
                                    [&] { return e.run_converged(converged_run(max_iterations, criterion, tol, with_map, relax)); });
    e.built = e.built_upto == (int)e.kernels.size() && !e.kernels.empty();
    return rc;
}

int lccrf_batch_get_fallback_frames(lccrf_batch_handle b, int *n_frames)
{
    CHECK_H(b);
    if (!n_frames) return fail(LCCRF_E_INVALID, "n_frames is NULL");
    { int rl = b->eng.resolve_late(); if (rl) return rl; }
    *n_frames = b->eng.report.fallback_frames;
    return LCCRF_OK;
}

int lccrf_batch_synchronize(lccrf_batch_handle b)
{
    CHECK_H(b);
    // Scoped to THIS batch: its stream (calls made on a caller's stream are ordered into it before they return) and its two copy
    // streams.  Not hipDeviceSynchronize: a host that keeps several batches in flight (tools/replay_multi.cpp, tools/host_pipeline.cpp)
    // settles one of them while the others' uploads and kernels keep running.
    HIP_TRY(hipStreamSynchronize(b->eng.stream));
    if (b->pipe.up) HIP_TRY(hipStreamSynchronize(b->pipe.up));
    if (b->pipe.down) HIP_TRY(hipStreamSynchronize(b->pipe.down));
    return b->eng.resolve_late();
}

// The batch read-backs: settle a pending one-launch run (its re-run of flagged frames included), then copy `bytes` of a device array
// of the batch to the caller.
static int batch_read_back(lccrf_batch *b, void *out, const void *d_src, size_t bytes)
{
    { int rl = b->eng.resolve_late(); if (rl) return rl; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
    return LCCRF_OK;
}

int lccrf_batch_get_map_host(lccrf_batch_handle b, int16_t *map_out)
{
    CHECK_H(b);
    if (!map_out) return fail(LCCRF_E_INVALID, "map_out is NULL");
    return batch_read_back(b, map_out, b->eng.crf.map, sizeof(int16_t) * (size_t)b->eng.F * b->eng.maxN);
}

int lccrf_batch_get_probability_host(lccrf_batch_handle b, float *prob_out)
{
    CHECK_H(b);
    if (!prob_out) return fail(LCCRF_E_INVALID, "prob_out is NULL");
    return batch_read_back(b, prob_out, b->eng.crf.Q, sizeof(float) * (size_t)b->eng.F * b->eng.maxN * b->eng.L);
}

int lccrf_batch_get_lattice_sizes_host(lccrf_batch_handle b, int kernel, int32_t *n_vertices_out)
{
    CHECK_H(b);
    CHECK_K(b, kernel);
    if (!n_vertices_out) return fail(LCCRF_E_INVALID, "n_vertices_out is NULL");
    return batch_read_back(b, n_vertices_out, b->eng.kernels[kernel].dev.V, sizeof(int) * b->eng.F);
}

// parity probe: the tables of one frame's lattice as they sit in HBM (internal point order, the build's own vertex ids); downloads only
int lccrf_batch_get_built_lattice(lccrf_batch_handle b, int kernel, int frame, int32_t *n_points_padded, int32_t *n_vertices,
                                  int32_t *perm_out, int32_t *offset_out, float *bary_out, int32_t *rowptr_out, int32_t *csr_pt_out,
                                  float *csr_w_out, int32_t *nbr_out, uint8_t *fastn_out, int *has_fastn)
{
    CHECK_H(b);
    CHECK_K(b, kernel);
    Engine &e = b->eng;
    if (frame < 0 || frame >= e.F) return fail(LCCRF_E_INVALID, "frame %d not in [0, %d)", frame, e.F);
    { int rc = e.make_ready(Engine::kSettled | Engine::kSized); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(e.stream));
    const KernelDev &k = e.kernels[kernel].dev;
    const size_t f = (size_t)frame, fe = f * k.Epad, f1 = f * (k.Epad + 1);
    int N = 0, V = 0;
    HIP_TRY(hipMemcpy(&N, e.crf.n_points + f, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&V, k.V + f, sizeof(int), hipMemcpyDeviceToHost));
    N = std::min(std::max(N, 0), e.maxN);
    V = std::min(std::max(V, 0), k.Epad);
    const int Np = (N + 3) & ~3;
    const size_t ne = (size_t)Np * k.D1, nr = (size_t)N * k.D1;
    if (n_points_padded) *n_points_padded = Np;
    if (n_vertices) *n_vertices = V;
    if (perm_out) {
        if (k.perm && Np) HIP_TRY(hipMemcpy(perm_out, k.perm + f * k.maxNpad, (size_t)Np * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; !k.perm && i < Np; ++i) perm_out[i] = i;
    }
    if (offset_out && ne) HIP_TRY(hipMemcpy(offset_out, k.offset + fe, ne * sizeof(int), hipMemcpyDeviceToHost));
    if (bary_out && ne) HIP_TRY(hipMemcpy(bary_out, k.bary + fe, ne * sizeof(float), hipMemcpyDeviceToHost));
    if (rowptr_out) HIP_TRY(hipMemcpy(rowptr_out, k.rowptr + f1, ((size_t)V + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (csr_pt_out && nr) HIP_TRY(hipMemcpy(csr_pt_out, k.csr_pt + fe, nr * sizeof(int), hipMemcpyDeviceToHost));
    if (csr_w_out && nr) HIP_TRY(hipMemcpy(csr_w_out, k.csr_w + fe, nr * sizeof(float), hipMemcpyDeviceToHost));
    for (int j = 0; nbr_out && j < k.D1 && V; ++j)        // device rows are strided by Epad, output by V
        HIP_TRY(hipMemcpy(nbr_out + (size_t)j * V * 2, k.nbr + (f * k.D1 + j) * k.Epad * 2, (size_t)V * 2 * sizeof(int), hipMemcpyDeviceToHost));
    const bool fastn = k.fastn != nullptr && k.vorder;    // (written by the sorted build alone)
    if (has_fastn) *has_fastn = fastn ? 1 : 0;
    if (fastn_out && fastn && V) HIP_TRY(hipMemcpy(fastn_out, k.fastn + fe, (size_t)V, hipMemcpyDeviceToHost));
    return LCCRF_OK;
}

int lccrf_batch_get_norm_host(lccrf_batch_handle b, int kernel, float *norm_out)
{
    CHECK_H(b);
    CHECK_K(b, kernel);
    if (!norm_out) return fail(LCCRF_E_INVALID, "norm_out is NULL");
    Engine &e = b->eng;
    { int rc = e.make_ready(Engine::kSettled | Engine::kBuilt); if (rc) return rc; }   // lccrf_batch_run builds nothing in HBM
    const float *src = e.kernels[kernel].dev.norm;
    if (e.perm_on) {                                  // the lattice's point arrays are in the internal order: undo it for the caller
        int rc = e.need_io();
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(e.io_a, 0, sizeof(float) * (size_t)e.F * e.maxN, e.stream));
        launch_permute_rows(e.crf, e.io_a, src, 1, 0, e.stream);
        HIP_TRY(hipGetLastError());
        src = e.io_a;
    }
    return batch_read_back(b, norm_out, src, sizeof(float) * (size_t)e.F * e.maxN);   // (nothing left to settle)
}

int lccrf_batch_device_buffers(lccrf_batch_handle b, const int16_t **d_map, const float **d_prob)
{
    CHECK_H(b);
    if (d_map) *d_map = b->eng.crf.map;
    if (d_prob) *d_prob = b->eng.crf.Q;
    return LCCRF_OK;
}

int lccrf_batch_device_label_bits(lccrf_batch_handle b, const uint64_t **d_bits, int *words_per_frame)
{
    CHECK_H(b);
    if (!d_bits || !words_per_frame) return fail(LCCRF_E_INVALID, "NULL output");
    if (!b->eng.crf.map_bits) return fail(LCCRF_E_INVALID, "packed labels exist for binary CRFs (n_labels == 2) only");
    *d_bits = reinterpret_cast<const uint64_t *>(b->eng.crf.map_bits);
    *words_per_frame = b->eng.crf.bits_stride;
    return LCCRF_OK;
}

int lccrf_batch_set_engine(lccrf_batch_handle b, int engine)
{
    CHECK_H(b);
    if (engine < 0 || engine > 2) return fail(LCCRF_E_INVALID, "engine must be 0, 1 or 2");
    b->eng.engine_pref = engine;
    b->eng.sizes_known = false;
    return LCCRF_OK;
}

int lccrf_batch_get_engine(lccrf_batch_handle b, int *engine_in_use)
{
    CHECK_H(b);
    if (!engine_in_use) return fail(LCCRF_E_INVALID, "engine_in_use is NULL");
    { int rl = b->eng.resolve_late(); if (rl) return rl; }   // a one-launch run may have fallen back
    return b->eng.engine_in_use(engine_in_use);
}

int lccrf_batch_get_fused_shape(lccrf_batch_handle b, int *lanes_per_frame, int *frames_per_cu)
{
    CHECK_H(b);
    if (!lanes_per_frame || !frames_per_cu) return fail(LCCRF_E_INVALID, "output pointer is NULL");
    *lanes_per_frame = b->eng.report.fused_shape & 0xffff;
    *frames_per_cu = b->eng.report.fused_shape >> 16;
    return LCCRF_OK;
}

int lccrf_batch_get_locality_mode(lccrf_batch_handle b, int *internal_point_order, int *sorted_build)
{
    CHECK_H(b);
    Engine &e = b->eng;
    if (e.built) {                                      // (a build that met an overflowing / wrapping frame is redone with the hash here)
        int rc = e.make_ready(Engine::kSized);
        if (rc) return rc;
    }
    if (internal_point_order) *internal_point_order = e.perm_on ? 1 : 0;
    if (sorted_build) *sorted_build = (e.perm_on && e.vorder_on && !e.vorder_broken) ? 1 : 0;
    return LCCRF_OK;
}

int lccrf_batch_get_stream(lccrf_batch_handle b, void **stream)
{
    CHECK_H(b);
    if (!stream) return fail(LCCRF_E_INVALID, "stream is NULL");
    *stream = static_cast<void *>(b->eng.stream);
    return LCCRF_OK;
}

int lccrf_batch_last_timing(lccrf_batch_handle b, float *inference_ms, float *build_ms)
{
    CHECK_H(b);
    Engine &e = b->eng;
    { int rl = b->eng.resolve_late(); if (rl) return rl; }
    HIP_TRY(hipDeviceSynchronize());
    if (build_ms) {
        *build_ms = 0.0f;
        if (e.timed_build) HIP_TRY(hipEventElapsedTime(build_ms, e.ev[0], e.ev[1]));
    }
    if (inference_ms) {
        *inference_ms = 0.0f;
        if (e.timed_inf) HIP_TRY(hipEventElapsedTime(inference_ms, e.ev[2], e.ev[3]));
    }
    return LCCRF_OK;
}

int lccrf_batch_last_prepare(lccrf_batch_handle b, float *prepare_ms, int *runs)
{
    CHECK_H(b);
    Engine &e = b->eng;
    { int rl = e.resolve_late(); if (rl) return rl; }
    if (prepare_ms) {
        *prepare_ms = 0.0f;
        if (e.lean_prep.timed) {
            HIP_TRY(hipEventSynchronize(e.lean_prep.ev1));
            HIP_TRY(hipEventElapsedTime(prepare_ms, e.lean_prep.ev0, e.lean_prep.ev1));
        }
    }
    if (runs) *runs = (int)e.lean_prep.runs;
    return LCCRF_OK;
}

int lccrf_batch_time_blur_pass(lccrf_batch_handle b, int kernel, int reps, float *ms_per_launch, int64_t *vertices_per_launch)
{
    CHECK_H(b);
    CHECK_K(b, kernel);
    if (reps < 1 || !ms_per_launch) return fail(LCCRF_E_INVALID, "reps < 1 or NULL output");
    Engine &e = b->eng;
    if (!e.built) return fail(LCCRF_E_STATE, "lccrf_batch_build has not run for these inputs");
    int rc = e.make_ready(Engine::kSized);
    if (rc) return rc;
    if (vertices_per_launch) {
        int64_t tot = 0;
        for (int f = 0; f < e.F; ++f) tot += e.V_host[(size_t)kernel * e.Fcap + f];
        *vertices_per_launch = tot;
    }
    hipError_t er = time_blur_pass(e.kdevs[kernel], e.F, e.maxV[kernel], e.L, reps, e.stream, ms_per_launch);
    if (er != hipSuccess) return fail(LCCRF_E_HIP, "time_blur_pass: %s", hipGetErrorString(er));
    return LCCRF_OK;
}

// section 2c: the batch's unaries (its weights are in api_model.hip, the gradients of its inference in api_backward.hip)
int lccrf_batch_set_unary_device(lccrf_batch_handle b, const float *d_unary)
{
    CHECK_H(b);
    Engine &e = b->eng;
    const size_t n = (size_t)e.F * e.maxN * e.L;
    { int rc = check_device_array(e, d_unary, n * sizeof(float), "d_unary"); if (rc) return rc; }
    if (!b->inputs_set) return fail(LCCRF_E_STATE, "inputs not set");
    { int rl = e.resolve_late(); if (rl) return rl; }
    if (n) HIP_TRY(hipMemcpyAsync(e.unary_own, d_unary, n * sizeof(float), hipMemcpyDefault, e.stream));
    e.bind_unary(e.unary_own);                            // (drops label-derived and permuted unary state; lattices and records stay)
    return LCCRF_OK;
}

// --------------------------------------------------------------------------------------
// section 5: pose optimisation on a batch's labels

int lccrf_batch_pose_optimization(lccrf_batch_handle b, const float *d_Xw, const float *d_kp, const float *d_u_right,
                                  const float *d_inv_sigma2, const uint8_t *d_valid, const float *K4, float bf,
                                  const float *d_Tcw_in, float *d_Tcw_out, uint8_t *d_outlier, int32_t *d_n_inliers,
                                  int32_t *d_n_initial, void *stream)
{
    CHECK_H(b);
    if (!d_Xw || !d_kp || !d_u_right || !d_inv_sigma2 || !K4 || !d_Tcw_in || !d_Tcw_out || !d_outlier || !d_n_inliers || !d_n_initial)
        return fail(LCCRF_E_INVALID, "NULL array");
    Engine &e = b->eng;
    if (!e.started) return fail(LCCRF_E_STATE, "no inference has produced labels yet");
    if (!e.last_with_map) return fail(LCCRF_E_STATE, "the last inference ran with with_map = 0: there are no labels to consume");
    if (e.maxN > 16384) return fail(LCCRF_E_CAPACITY, "at most 16384 keypoints per frame");
    // a one-launch run may still owe the labels of frames that did not fit its kernel (they are written by the
    // re-run): settle that first -- one synchronisation, and only when lccrf_batch_run is still pending
    { int rl = e.resolve_late(); if (rl) return rl; }
    StreamScope scope(e, stream);
    int rc = scope.enter();
    if (rc) return rc;
    // the labels are read where the inference kernel wrote them: no host round trip between the CRF and the pose
    hipError_t er = launch_pose_optimization(e.F, e.maxN, b->d_pose_total ? b->d_pose_total : e.crf.n_points, d_Xw, d_kp, d_u_right,
                                             d_inv_sigma2, d_valid, e.crf.map, K4, bf, d_Tcw_in, d_Tcw_out, d_outlier, d_n_inliers,
                                             d_n_initial, e.stream, b->d_pose_total ? e.crf.n_points : nullptr);
    if (er != hipSuccess) return fail(LCCRF_E_HIP, "pose optimisation: %s", hipGetErrorString(er));
    return LCCRF_OK;
}

int lccrf_batch_pose_set_crf_counts(lccrf_batch_handle b, const int32_t *d_n_total)
{
    CHECK_H(b);
    b->d_pose_total = d_n_total;
    return LCCRF_OK;
}

}  // extern "C"

// api_common.h -- what the units of the C-ABI (api_*.hip) share: the handles' definitions, the handle checks, and the few helpers
// more than one unit calls.  fail() and HIP_TRY come with host_engine.h; the error text itself lives in api_tools.hip.
#pragma once

#include "host_engine.h"

#include <vector>

struct lccrf_crf {
    lccrf::Engine eng;
    int N = 0;                      // points of the CRF this handle currently represents
    int cap = 0;                    // capacity it was allocated for (eng.maxN)
    int16_t *stage_i16 = nullptr;   // pinned [cap]
    float *stage_f32 = nullptr;     // pinned [cap*L]
    int *stage_n = nullptr;         // pinned [1]: the point count where the kernels of a SLAM frame read it (no upload command)
    bool label_stage_busy = false;  // a kernel that reads stage_i16 may still be pending
    int16_t *map_pin = nullptr;     // pinned [cap]: the kernels write the MAP labels straight into host memory
    int16_t *map_dev = nullptr;     // device [cap]: where they go instead once lccrf_device_buffers has handed out the labels (section 1b)
};

// The asynchronous host path of a batch (lccrf_batch_set_inputs_host_async / _download_async / _wait_download): pinned staging for
// the inputs and the results, one stream per copy direction (the GPU has DMA engines for both), events instead of host waits.
// One batch is in flight per handle; a caller that wants batch i+1 uploaded under batch i's kernels alternates between handles.
struct HostPipe {
    hipStream_t up = nullptr, down = nullptr;
    hipEvent_t ev_up = nullptr, ev_down = nullptr, ev_q = nullptr;   // upload landed / download landed / "everything queued so far"
    int *npoints = nullptr;                  // pinned staging, sized for the batch's capacities
    int16_t *label = nullptr;
    float *unary = nullptr;
    std::vector<float *> feat;
    uint64_t *bits = nullptr;                // pinned results
    int16_t *map = nullptr;
    float *prob = nullptr;
    bool up_pending = false, down_pending = false;
    int down_what = 0, down_frames = 0;
    int copy_threads = 8;                    // host threads of the staging copy (LCCRF_OPT_COPY_THREADS)
    void destroy()
    {
        if (up) (void)hipStreamDestroy(up);
        if (down) (void)hipStreamDestroy(down);
        for (hipEvent_t ev : {ev_up, ev_down, ev_q})
            if (ev) (void)hipEventDestroy(ev);
        up = down = nullptr;
        ev_up = ev_down = ev_q = nullptr;
    }
};

struct lccrf_batch {
    lccrf::Engine eng;
    lccrf_batch_desc desc{};
    bool inputs_set = false, labels_bound = false;
    const int16_t *d_label = nullptr;
    const int32_t *d_pose_total = nullptr;   // lccrf_batch_pose_set_crf_counts
    HostPipe pipe;
};

#define CHECK_H(h)                                                    \
    do {                                                              \
        if (!(h)) return fail(LCCRF_E_INVALID, "handle is NULL");     \
        HIP_TRY(hipSetDevice((h)->eng.device));                       \
        (h)->eng.touched();                                           \
    } while (0)

#define CHECK_K(h, k)                                                                      \
    do {                                                                                   \
        if ((k) < 0 || (k) >= (int)(h)->eng.kernels.size())                                \
            return fail(LCCRF_E_INVALID, "kernel index %d out of range", (k));             \
    } while (0)

// ... and the same of an index no handle or batch can have: checked before the handle is looked at, so the answer needs no device
#define CHECK_K_ANY(k)                                                                                      \
    do {                                                                                                    \
        if ((k) < 0 || (k) >= LCCRF_MAX_KERNELS) return fail(LCCRF_E_INVALID, "kernel index %d out of range", (k)); \
    } while (0)

namespace lccrf {

int use_device(int device_id);                                  // api_tools.hip
void trim_pose_stages();                                        // frees lccrf_pose_optimization's staging areas (lccrf_trim_cache)
void trim_unary_stage();                                        // unary_builder.hip: frees lccrf_unary_build's staging (lccrf_trim_cache)
void trim_bf_stage();                                           // bf_match.hip: frees lccrf_bf_match's staging (lccrf_trim_cache)
int apply_option(Engine &e, int option, int value);             // api_object.hip: the options a handle and a batch share
// api_object.hip (section 1b): is `p` device memory of the engine's device, or pinned host memory, with `bytes` inside its allocation?
int check_device_array(const Engine &eng, const void *p, size_t bytes, const char *what);

// Runs the body of a batch call on a caller-supplied stream.  The engine's own stream carries the
// zeroing of fresh allocations (Arena::alloc) and the kernels of lccrf_batch_bind_inputs_device, and
// nothing else orders a foreign stream against it: entering makes the caller's stream wait for
// everything queued on the own stream so far, leaving makes the own stream (read-backs, later
// calls) wait for the caller's.  The engine's stream is restored on every exit path.
struct StreamScope {
    Engine &e;
    hipStream_t own, use;
    StreamScope(Engine &eng, void *stream) : e(eng), own(eng.stream), use(stream ? (hipStream_t)stream : eng.stream) {}
    int enter()
    {
        if (use != own) {
            HIP_TRY(hipEventRecord(e.ev_order, own));
            HIP_TRY(hipStreamWaitEvent(use, e.ev_order, 0));
        }
        e.stream = e.mem.stream = use;                    // lazy allocations of this call are zeroed on the stream its kernels run on
        return LCCRF_OK;
    }
    ~StreamScope()
    {
        e.stream = e.mem.stream = own;
        if (use != own) {
            (void)hipEventRecord(e.ev_order, use);
            (void)hipStreamWaitEvent(own, e.ev_order, 0);
        }
    }
};

// The timed batch calls (build, inference, run): `body` runs in a StreamScope on the call's stream, between the events `begin` and
// `end` when event timing is on; `timed` tells lccrf_batch_last_timing whether that pair now holds this call's time.
template <typename Body>
int timed_batch_call(Engine &e, void *stream, hipEvent_t begin, hipEvent_t end, bool &timed, Body body)
{
    StreamScope scope(e, stream);
    int rc = scope.enter();
    if (rc) return rc;
    if (e.opt.event_timing) HIP_TRY(hipEventRecord(begin, e.stream));
    rc = body();
    if (!rc && e.opt.event_timing) {
        hipError_t er = hipEventRecord(end, e.stream);
        if (er != hipSuccess) rc = fail(LCCRF_E_HIP, "hipEventRecord: %s", hipGetErrorString(er));
    }
    timed = !rc && e.opt.event_timing;
    return rc;
}

}  // namespace lccrf

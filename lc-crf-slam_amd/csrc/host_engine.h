// host_engine.h -- the host-side state machine behind the C-ABI: one Engine per handle or batch.
//
// Host code only (no kernel): device memory, lattice builds, locality mode, engine choice, the late-bound one-launch run with its
// per-frame fallback, the done-word protocol, the backward area and the learnt model.  The bodies are in host_engine.hip (lifecycle,
// readiness, builds, run routes), host_late.hip (settling a one-launch run) and host_model.hip (LearntModel); the entry points of
// include/lccrf.h (api_*.hip) read and write the fields below directly -- all but what has one owner: what a call relies on is brought
// up to date by make_ready() alone, what is in flight is `flight`, a user's options are `opt` (reset as a whole), what the last run
// was is `report` (written by its recorders alone) and the terms' matrices and modes are `model` (changed by its methods alone).
// Every run is one Schedule (engine.h) -- a fixed count, or a cap with its criterion and tol -- built by the entry points.  A
// one-launch run is armed by run_frame() alone, which keeps it as `late`, what resolve_late() re-runs flagged frames with; the fused
// engine's kernels on lattices in HBM are launched, and what the engine reports of them recorded, by launch_sized() alone.
#pragma once

#include "engine.h"

#include <vector>

namespace lccrf {

// Sets the calling thread's error text (lccrf_last_error) and returns `code`.  Defined once, in api_tools.hip.
int fail(int code, const char *fmt, ...);
bool default_single_wg(), default_frame_general();   // LCCRF_OPT_SINGLE_WORKGROUP's and LCCRF_OPT_FRAME_GENERAL's process-wide defaults (api_tools.hip)
bool default_fused_multilabel();                      // ... and LCCRF_OPT_FUSED_MULTILABEL's

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? LCCRF_E_NOMEM : LCCRF_E_HIP, "%s: %s",  \
                        #expr, hipGetErrorString(e_));                                       \
    } while (0)

// spin-wait hint of the host polls (the library must build on non-x86 ROCm hosts too)
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}

inline int next_pow2(long v)
{
    long p = 16;
    while (p < v) p <<= 1;
    return (int)p;
}

// Owns every device / pinned allocation of one engine.
struct Arena {
    std::vector<void *> dev, pinned;
    // Allocations are zeroed ON THE STREAM THE OWNER'S WORK IS ISSUED ON (StreamScope retargets this together with
    // Engine::stream while a batch call runs on a caller's stream: a lazily allocated buffer zeroed on the engine's
    // own stream would be unordered with the kernels of that call -- ADVICE r3).  hipMemset on the null stream is
    // asynchronous and the engine streams are non-blocking, i.e. unordered with the null stream: a null-stream
    // memset could land after the first copy into the new buffer (seen as a one-in-hundreds lattice
    // of all-zero features).
    hipStream_t stream = nullptr;
    template <typename T>
    int alloc(T **out, size_t count, bool zero = true)
    {
        void *p = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        HIP_TRY(hipMalloc(&p, bytes));
        dev.push_back(p);
        if (zero) {
            HIP_TRY(hipMemsetAsync(p, 0, bytes, stream));
            if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
        }
        *out = static_cast<T *>(p);
        return LCCRF_OK;
    }
    template <typename T>
    int alloc_pinned(T **out, size_t count)
    {
        void *p = nullptr;
        // fine-grained (coherent) on purpose, not left to HIP_HOST_COHERENT: kernels publish status words, done words and labels
        // here and the host reads them while the kernel is still running
        HIP_TRY(hipHostMalloc(&p, (count ? count : 1) * sizeof(T), hipHostMallocCoherent));
        pinned.push_back(p);
        *out = static_cast<T *>(p);
        return LCCRF_OK;
    }
    void release()
    {
        for (void *p : dev) (void)hipFree(p);
        for (void *p : pinned) (void)hipHostFree(p);
        dev.clear();
        pinned.clear();
    }
};

struct KernelState {
    KernelDev dev{};
    float *feat_own = nullptr;    // device copy of host-provided features
    float *feat_stage = nullptr;  // pinned staging for the object API
    int maxV = 0;                 // max over frames of V once known, else Epad
    int maxRow = 0;               // max over frames of the longest CSR row
    int *bstat = nullptr;         // [Fcap][kBuildStats] device: the streaming build's counters, behind dev.rowmax's Fcap ints (engine.h: BuildStat)
    bool build_counted = false;   // the lattices now in HBM came from the streaming build, whose counters are in Engine::row_host
    float *norm_root = nullptr;   // [F][maxN] sqrtf(norm) of a term normalised SYMMETRICally (section 1g; lazy, kept with the lattice)
    bool root_valid = false;      // ... holds the roots of the norm now in HBM.  Invariant: whatever writes KernelDev::norm in HBM clears
                                  //   this -- today that is Engine::build_kernels alone (the streaming and the one-workgroup build; the
                                  //   one-launch frame kernel keeps its norm in LDS and leaves built_upto as it was)
};

// One CRF problem set: F frames x maxN points x L labels, K kernels.
struct Engine {
    // ---- shape and buffers ----
    int device = 0;
    hipStream_t stream = nullptr;
    Arena mem;
    int Fcap = 0, F = 0, maxN = 0, maxNpad = 0, L = 0;
    int activeN = 0;                   // largest frame of the current inputs if known on the host, else 0
    CrfDev crf{};
    int *npoints_own = nullptr;
    float *unary_own = nullptr;
    int16_t *label_own = nullptr;
    hipEvent_t ev_order = nullptr;     // orders a caller-supplied stream against the engine's own (StreamScope)
    int *npoints_bad = nullptr;        // pinned: set by the validation kernel when a bound n_points[f] is outside [0, maxN]
    float *io_a = nullptr, *io_b = nullptr;   // device [Fcap][maxN][L] each: caller buffers of apply / expAndNormalize / ... (lazy)
    int16_t *io_map = nullptr;
    bool unary_set = false, built = false, sizes_known = false, started = false;

    // ---- lattices and their sizes ----
    int *V_host = nullptr;             // pinned [K][Fcap]
    int *row_host = nullptr;           // pinned [K][row_stride()]: rowmax of every frame, then [Fcap][kBuildStats] the streaming build's counters
    size_t row_stride() const { return (size_t)Fcap * (1 + kBuildStats); }
    int *long_host = nullptr;          // pinned [K][Fcap]: rows beyond kLongRowMin entries per frame (KernelDev::longcnt)
    std::vector<KernelState> kernels;
    std::vector<KernelState> spare;    // allocated lattices of earlier uses of this (recycled) engine
    std::vector<KernelDev> kdevs;      // contiguous copy handed to the launchers
    std::vector<int> maxV, maxRow;
    int built_upto = 0;                // kernels [0, built_upto) have their lattice

    // ---- engine choice ----
    int engine_pref = 0;
    int sized_engine = 1;              // what choose_sized_engine() chose for inference on lattices that sit in HBM (1, 2, 4, 5 or 6)
    int last_with_map = 0;             // did the last inference produce MAP labels?
    size_t fused_lds = 0;
    LeanPrep lean_prep;                // prepared launch records of the two-frames-per-CU inference kernel (engine.h)
    bool fused_fits = false;           // learn_sizes(): the lattices now in HBM fit the fused engine
    bool multi_fits = false;           // ... or, with 3 to 8 labels, the plan of its multi-label kernel (multilabel_supported)
    bool learnt_fits = false;          // ... or that of its kernel for learnt models of 3 to 8 labels (multilabel_general_supported)
    bool batch_owned = false;          // set by lccrf_batch_create: the engine of a batch (whatever its frame count), not of a handle

    // ---- deferred unaries ----
    // setUnaryEnergyFromLabel is deferred: the labels wait in pinned memory and either the late-bound
    // fused kernel derives the energies itself or ensure_unary() launches the small kernel.
    bool unary_deferred = false;
    const int16_t *deferred_label = nullptr;
    UnaryTable deferred_tbl{};
    bool unary_is_label = false;       // the unaries come from labels (re-derivable in any order) rather than from a raw array
    // ... and, for two labels, what ensure_unary() leaves beside the unary array for the lean inference kernel (engine.h: LabelCodes):
    // the library's own, allocated on first use; valid while the unary array is the one that launch wrote
    unsigned char *label_codes = nullptr;
    float *label_pairs = nullptr;
    bool label_codes_valid = false;

    // ---- the late-bound one-launch run, the done word and the label polling ----
    // Late-bound fused inference (object API): queued right behind the build, before the host has seen
    // the lattice sizes; `late_status` (pinned) tells afterwards whether the frame fitted.
    int *late_status = nullptr;
    bool late_ok = false;              // set by the object API: single frame, automatic engine choice
    // the pending run's (run_frame): its flagged frames are re-run with it on the two-kernel path (rerun_on) -- a converged one with
    // inference_converged(), their reports scattered back beside Q and the labels
    Schedule late{0, 0, 1.0f, false, 0, 0.0f};
    // Called by resolve_late() right behind a re-run of flagged frames (before its final synchronisation): the owner of host-side
    // copies of the results (the batch's download pipe) re-queues them, whichever entry point happened to settle the run.
    int (*after_rerun)(void *) = nullptr;
    void *after_rerun_ctx = nullptr;
    static constexpr int kDualMaxFrames = 64;    // (measured, `scripts/small_batch_latency.py`: 4 frames 98 -> 86 us, 32 frames 93 -> 83 us, 128 frames 112 -> 114 us)
    unsigned *dual_area = nullptr;     // hand-off area of the two-workgroup form of the frame kernel (batches of up to kDualMaxFrames frames)
    unsigned dual_epoch = 0;
    // object API: the frame kernel's last act is a store of `done_epoch` into this pinned word, behind its results; the host
    // polls it instead of waiting for the runtime's completion signal (which arrives a few microseconds later)
    unsigned *done_word = nullptr;
    unsigned done_epoch = 0;
    // ... and with_map launches of the object API do not even wait for that word: the host pre-fills the pinned label array
    // with -1 and takes each label as it arrives (the kernel's last stores; no fence, no acknowledgement round trip)
    int16_t *map_host = nullptr;       // the handle's pinned label array (= crf.map), or null
    // What is in flight on the stream, as far as the host knows: moved by run_frame() (arm), take_labels(), resolve_late() (settle),
    // done_seen(), touched(), recycle() (park) and ensure_parked_idle(), and by nothing else.
    enum class Flight {
        kUnknown,          // nothing known to be in flight, nothing known to have ended: whoever must know waits for the stream
        kPending,          // a one-launch run: settled by a stream synchronisation,
        kPendingDone,      //   ... by its done word,
        kPendingLabels,    //   ... or label by label (take_labels), the done word behind them
        kLabelsSeen,       // the last call on the handle was a getMap() that saw every label (the stores right before the done word,
                           //   which is still to come): the run has fitted and is past its last read
        kDoneSeen,         // ... or that saw the done word: nothing is in flight
        kParkedDoneDue,    // parked from kLabelsSeen, the word still unseen: ensure_parked_idle() settles it for the next user
    } flight = Flight::kUnknown;
    bool run_pending() const { return flight == Flight::kPending || flight == Flight::kPendingDone || flight == Flight::kPendingLabels; }
    // another call has touched the handle: whatever the last getMap() saw says nothing about what that call enqueues
    void touched() { if (flight == Flight::kLabelsSeen || flight == Flight::kDoneSeen) flight = Flight::kUnknown; }
    void done_seen() { flight = Flight::kDoneSeen; }   // (getMap(): resolve_late() saw the done word and nothing was enqueued since)
    bool take_labels(int16_t *out, int n);

    // ---- per-frame fallback ----
    // Per-frame fallback of the one-launch kernel: k_frame leaves 1 in frame_status[f] for a frame whose lattices do not
    // fit its LDS plan; resolve_late() gathers exactly those frames into the sub-engine `fb`, runs the two-kernel path
    // there and scatters Q / labels / V back.
    int *frame_status = nullptr;       // device [Fcap]
    int *frame_status_host = nullptr;  // pinned [Fcap]
    int *fb_list = nullptr;            // device [Fcap]: frames being re-run
    int *fb_list_host = nullptr;       // pinned [Fcap]
    Engine *fb = nullptr;
    bool frame_small_ok = true;        // small frames may run as 512-lane workgroups (two per CU); turned off for this engine when
    bool frame_small_used = false;     //   more than 1/8 of a batch's frames did not fit that plan
    bool frame_lean_ok = true;         // ... and so may batches of full-size frames (frame_lean.hip), under the same rule
    bool frame_lean_used = false;
    unsigned char *lean_rec = nullptr; //   [lean_rec_frames][kLeanRecBytes] per-point records of that kernel (lazy, sized for the frames bound)
    int lean_rec_frames = 0;

    // ---- locality mode and the sorted build ----
    // Locality mode (batch engines, frames of >= kPermMinPoints points on the streaming engine): the lattices are built
    // with the points in an internal Z-order of their lattice cells (stream_build.hip: launch_sort_points); Q, next and
    // the unaries of the iteration live in that order (Qp, unary_p / unary_own) and Q is un-permuted on the way out.
    static constexpr int kPermMinPointsDefault = 8192;
    bool allow_perm = false;           // set by lccrf_batch_create, and by lccrf_create for handles of >= kPermMinPoints points ...
    bool perm_scoped = false;          // ... where it only applies to lattices that are first asked for by inference() (kMayReorder): every
                                       //   other entry point of the object API (stepwise inference, PairwisePotential::apply, the lattice
    bool perm_banned = false;          //   probes) works on the caller's point order -- such a handle is built, or re-built once, the plain way
    bool perm_on = false;              // the lattices now in HBM were built in locality mode
    bool unary_p_valid = false;        // unary_p holds the raw unaries in the current internal order
    SortScratch sort{};
    float *Qp = nullptr, *unary_p = nullptr;   // [Fcap][maxN][L]
    bool sort_scratch_complete = false;
    bool vorder_on = false;            // the sorted build (Options::vertex_order), as decided by the last build of every kernel
    bool vorder_broken = false;        // a frame's code space overflowed (*sort.vbad): this engine keeps to the hash build
    int *ndist_host = nullptr;         // pinned [K][kNdistAxes]: the sorted build's largest neighbour distances (KernelDev::ndist)
    int *tbl_bad = nullptr;            // pinned [2]: what the sorted build found wrong with its tables (KernelDev::tbl_bad)

    // ---- backward area ----
    // the area of lccrf_inference_backward / lccrf_batch_inference_backward (engine.h: BackwardArea): its own allocation, grown on
    // demand and freed with the handle's use (recycle) -- a parked handle does not keep it -- or with the batch
    unsigned char *bwd_area = nullptr;
    size_t bwd_area_bytes = 0;

    // ---- a user's options ----
    // lccrf_set_option / lccrf_batch_set_option write here and nowhere else; lccrf_create (new and recycled handles alike) and
    // lccrf_batch_create assign fresh(), so a recycled handle inherits none of its last user's.
    struct Options {
        bool single_wg = false;        // LCCRF_OPT_SINGLE_WORKGROUP: never the two-workgroup form of the frame kernel
        bool frame_general = false;    // LCCRF_OPT_FRAME_GENERAL: terms with a matrix or a mode may take the one-launch route (frame_general.hip)
        bool fused_backward = false;   // LCCRF_OPT_FUSED_BACKWARD: dL/dU and dL/dw of frames the fused plan takes run in one launch (fused_backward.hip)
        bool fused_backward_learnt = false;   // LCCRF_OPT_FUSED_BACKWARD_LEARNT: the same for learnt models and dL/dmu (fused_backward_general.hip)
        bool fused_backward_features = false; // LCCRF_OPT_FUSED_BACKWARD_FEATURES: the same with feature gradients (fused_backward_features.hip)
        bool fused_multilabel = false; // LCCRF_OPT_FUSED_MULTILABEL: frames of 3 to 8 labels the fused plan takes run in one launch (fused_multilabel.hip)
        bool fused_multilabel_learnt = false;   // LCCRF_MULTILABEL_LEARNT (lccrf_set_multilabel_routes; no option number, no process-wide default):
                                       //   the same for terms with a matrix or a mode (fused_multilabel_general.hip)
        int vertex_order = 0;          // LCCRF_OPT_VERTEX_ORDER: 0 automatic (= on), 1 on, 2 off -- locality mode's sorted build
        bool event_timing = true;      // LCCRF_OPT_EVENT_TIMING: HIP events around every build / inference / run of the batch API
        static Options fresh() { Options o; o.single_wg = default_single_wg(); o.frame_general = default_frame_general(); o.fused_multilabel = default_fused_multilabel(); return o; }
    } opt;

    // ---- what the last run was ----
    // Report only (lccrf_get_engine, lccrf_batch_get_engine / _fused_shape / _fallback_frames, lccrf_get_backward_route): nothing
    // decides on it.  Written by the recorders below, one per route, and reset as a whole (recycle, lccrf_create).
    struct RunReport {
        int engine = 1;                // 1 streaming, 2 fused, 3 one launch per frame, 4 the fused engine's kernels with matrices and factors,
                                       //   5 its kernel for 3 to 8 labels, 6 that kernel's form for learnt models (matrices and modes)
        int shape = 0;                 // fused_report() of the last inference on engine 2, 4, 5 or 6, else 0
        int fused_shape = 0;           // what the last one-workgroup inference launched: lanes per frame | frames per CU << 16 (engines 5 and 6: | points per lane << 16)
        int conv_engine = 0;           // 4 / 3 / 2 / 1 when the last inference was a converged one, else 0
        int fallback_frames = 0;       // frames the last one-launch run had to re-run
        int backward_route = 0;        // LCCRF_BACKWARD_* of the last successful backward call
        void ran_on(int e, bool until_converged) { engine = e; shape = 0; conv_engine = until_converged ? e : 0; }
        void frame_run(int launch_shape, bool until_converged)   // run_frame: launch_frame()'s 0, 1 (small) or 2 (lean)
        {
            ran_on(3, until_converged);
            fallback_frames = 0;
            fused_shape = launch_shape == 0 ? (1024 | 1 << 16) : (512 | 2 << 16);
        }
        void sized_run(int e, const SizedLaunch &r, bool until_converged, bool general)   // launch_sized (k_converge leaves fused_shape)
        {
            ran_on(e, until_converged);
            shape = r.report;
            if (!until_converged || general) fused_shape = r.shape;
        }
        void settled(int flagged, bool partial) { fallback_frames = flagged; if (partial) engine = 3; }   // resolve_late
        void backward(int route) { backward_route = route; }
        void new_inputs() { conv_engine = 0; }
        // lccrf_batch_get_engine's answer, kept: `sized` (or 0) is what lattices in HBM run on now; a converged run overrides it
        int in_use(int sized) { if (sized) engine = sized; if (conv_engine) engine = conv_engine; return engine; }
    } report;
    int engine_in_use(int *out);

    // ---- the learnt model ----
    // Sections 1e / 1g (a handle) and 2g (a batch: one matrix and one mode per term, shared by every frame).  The matrices live in one
    // device array, allocated by the first setter and kept with the handle or batch; compat_ptr[k] is term k's [L][L] slice of it, or
    // null (Potts).  The modes say where each term applies its norm: after the filter (the reference's form and the default), before
    // it, half on either side, or not at all.  While general() the one-launch frame kernel (but for its general form under
    // LCCRF_OPT_FRAME_GENERAL: frame_ok) and the fused engine, which hard-wire Potts terms normalised AFTER, are not taken (nor their
    // prepared launch records touched): the frames choose_sized_engine() names run on the fused engine's general kernels, the rest on
    // the streaming engine's general branch -- with modes, on kdevs_post, the copy of kdevs whose `norm` points at each term's factor
    // BEHIND the filter, with pre_ptr[k] the factor of its input (kStepViews, behind kSized).  Bodies in host_model.hip; the counters,
    // compat_ptr and factors_dirty are written there alone.  No setter touches a lattice, a norm or a prepared record.
    struct LearntModel {
        float *compat_dev = nullptr;       // [LCCRF_MAX_KERNELS][L][L]
        float *compat_host = nullptr;      // pinned, the same shape: the matrices as set (the getter's answer and the uploads' source)
        hipEvent_t compat_ev = nullptr;    // behind the last upload: a setter waits for it before it rewrites a source that may be in flight
        const float *compat_ptr[LCCRF_MAX_KERNELS] = {};
        size_t ll = 0;                     // L * L (known once a matrix is set)
        int n_compat = 0;
        int norm_mode[LCCRF_MAX_KERNELS] = {};   // lccrf_normalization of every term
        int n_modes = 0;                   // terms that are not LCCRF_NORMALIZE_AFTER
        float *ones = nullptr;             // [Fcap][maxN] of 1.0f: the factor behind the filter of a BEFORE or NONE term (lazy)
        std::vector<KernelDev> kdevs_post;
        const float *pre_ptr[LCCRF_MAX_KERNELS] = {};
        const float *host_mats[LCCRF_MAX_KERNELS] = {};
        bool factors_dirty = true;         // kdevs_post / pre_ptr are behind kdevs or the modes (raised by views_changed and set_mode)

        bool general() const { return n_compat || n_modes; }
        bool has_matrix(int k) const { return compat_ptr[k] != nullptr; }
        const float *matrix(int k) const { return compat_host + k * ll; }      // (the pinned copy; valid while has_matrix(k))
        int mode(int k) const { return norm_mode[k]; }
        const float *const *compat_arg() const { return n_compat ? compat_ptr : nullptr; }
        const float *const *pre_arg() const { return n_modes ? pre_ptr : nullptr; }   // (valid behind kStepViews)
        // the terms as the one-workgroup engines' launch requests take them (engine.h: TermModel; all null without a matrix or a mode):
        TermModel terms(size_t K)
        {
            for (size_t k = 0; k < K; ++k) host_mats[k] = compat_ptr[k] ? matrix((int)k) : nullptr;
            return TermModel{n_compat ? host_mats : nullptr, pre_arg(), n_modes ? norm_mode : nullptr, n_compat ? compat_ptr : nullptr};
        }
        void views_changed();                            // (sync_views: the views derived from kdevs are rebuilt by ensure_factors())
        // `e` is the engine this model is the `model` of: its arena, stream, kernels and engine choice
        void clear(Engine &e);                           // every term a Potts term normalised AFTER the filter
        int set_matrix(Engine &e, int k, const float *m);
        void set_mode(Engine &e, int k, int mode);
        int ensure_factors(Engine &e);
        int put_on(Engine &g, int K) const;              // g's model becomes this one (the sub-engine of rerun_frames)
        void release() { if (compat_ev) (void)hipEventDestroy(compat_ev); compat_ev = nullptr; compat_dev = compat_host = nullptr; }   // (destroy)
    } model;

    // ---- convergence-driven inference ----
    // sections 1h and 2e: what the last converged run reported per frame -- four [Fcap] arrays in HBM, written by the kernel of
    // fused_converge.hip or by the bookkeeping of converge_track.hip -- with the pinned mirror the host getters copy into, the
    // streaming path's accumulators / finished flags and its pinned "frames still running" word.  All allocated by init(): a
    // converged call allocates nothing on the one-launch path (the streaming path's kept copy of Q is io_a, need_io()).
    int *conv_dev = nullptr;           // device [7][Fcap]: iterations, delta (float), changed, converged, acc [Fcap][2], done
    int *conv_host = nullptr;          // pinned [4][Fcap]
    int *conv_running = nullptr;       // pinned [1]
    bool conv_valid = false;           // a converged run has reported on the current inputs
    ConvergeOut conv_out() const
    {
        return ConvergeOut{conv_dev, reinterpret_cast<float *>(conv_dev + Fcap), conv_dev + 2 * (size_t)Fcap, conv_dev + 3 * (size_t)Fcap};
    }

    // ---- timing ----
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // build begin/end, inference begin/end
    bool timed_build = false, timed_inf = false;

    // ---- methods (host_engine.hip, in this order, but for the late-run ones -- host_late.hip; the short ones here) ----
    int init(int device_id, int frames, int max_points, int n_labels);
    void destroy();
    int add_kernel(int d, float w, bool own_features, bool stage);
    void ensure_parked_idle();
    void recycle();
    void sync_views();
    int need_io();
    // every lattice is re-built (and its sizes learnt) by the next call that needs it; the prepared launch records are rewritten
    void invalidate_lattices() { built_upto = 0; sizes_known = false; }
    void invalidate_lean_prep() { lean_prep.valid = false; lean_prep.seen_key = 0; }
    // new inputs (a batch's next frames, a parked handle's next user): nothing set, built or started, every lattice stale
    void forget_inputs() { unary_set = built = started = conv_valid = false; report.new_inputs(); invalidate_lattices(); }
    // term k gets the weight w (settle a pending inference first): whatever was prepared for the old weights is rewritten
    void set_weight(int k, float w) { kernels[k].dev.w = w; sync_views(); invalidate_lean_prep(); }

    static int perm_min_points();
    int ensure_sort_scratch();
    int build_kernels(int k0, int n, bool may_reorder = false);

    // What a caller is about to rely on.  make_ready() satisfies the needs asked for in the order of the bits: a step may undo what a
    // later one provides (a re-build leaves label-derived unaries and the step views stale), never what an earlier one did.
    enum Need : unsigned {
        kSettled = 1,        // a pending one-launch run has finished, its flagged frames re-run (resolve_late)
        kCallerOrder = 2,    // no lattice in locality mode's internal point order (re-built the plain way if one is): for good on a
                             //   handle of large frames; on a batch for this call only, the next build decides afresh
        kBuilt = 4,          // every term has its lattice in HBM (the object API only stages features)
        kSized = 8,          // ... and the host knows their sizes: implies kBuilt and a stream synchronisation
        kUnaries = 16,       // label-derived unaries are written, in the lattices' point order
        kStepViews = 32,     // step_kdevs() / pre_arg() are valid (section 1g's factors)
        kMayReorder = 64,    // modifier: lattices built by this call may use locality mode (inference() on a handle of large frames)
    };
    int make_ready(unsigned needs);

    UnaryTable label_table(const float *conf) const;
    void defer_unary_from_label(const int16_t *label, const float *conf);
    void bind_unary(const float *p);

    int start();
    int step(float relax);
    bool frame_ok() const;
    int run_frame(const Schedule &run);
    int inference(int n_iter, int with_map, float relax);
    int run(int n_iter, int with_map, float relax);
    int inference_sized(const Schedule &run, unsigned more_needs = 0);   // (a fixed count; more_needs: 0 or kMayReorder)
    static int check_converged_args(int max_iter, int criterion, float tol, float relax);
    int inference_converged(const Schedule &run);
    int run_converged(const Schedule &run);
    int rerun_on(Engine &e);
    int converge_stream(const Schedule &run);
    int read_convergence();
    int resolve_late(bool *seen_done = nullptr);
    int rerun_frames(int n);

    // Lattices that fit the fused plan: Potts terms normalised AFTER run on the fused engine; frames -- a handle's one or a batch's
    // F -- of up to kGeneralMaxPoints active points with a matrix or another mode on the general kernel; anything else streams.
    // Under LCCRF_OPT_FUSED_MULTILABEL, Potts terms normalised AFTER over 3 to 8 labels on lattices that fit the multi-label kernel's
    // plan (multi_fits; never together with fused_fits, which wants two labels) run on that kernel: engine 5.  Under
    // LCCRF_MULTILABEL_LEARNT, terms with a matrix or a mode over 3 to 8 labels on lattices that fit the plan of
    // k_multilabel_general (learnt_fits) run on that kernel: engine 6.  The two bits are independent: each moves its own frames only.
    static constexpr int kGeneralMaxPoints = 2048;
    void choose_sized_engine()
    {
        sized_engine = !fused_fits ? 1 : !model.general() ? 2 : active_points(crf) <= kGeneralMaxPoints ? 4 : 1;
        if (opt.fused_multilabel && multi_fits && !model.general()) sized_engine = 5;
        if (opt.fused_multilabel_learnt && learnt_fits && model.general()) sized_engine = 6;
    }
    // what the streaming step, the plug-in filter and the backward sweep are handed (valid behind kStepViews)
    const KernelDev *step_kdevs() const { return model.n_modes ? model.kdevs_post.data() : kdevs.data(); }

    void free_backward_area();
    int ensure_backward_area(size_t need);
    size_t backward_need(const BackwardRequest &rq, size_t slice, int rows) const;
    int backward(const BackwardRequest &rq, size_t slice, int rows);

private:
    // the steps of make_ready(), and the view a streaming iteration runs on
    int flush_builds(bool may_reorder = false);
    int learn_sizes(bool may_reorder = false);
    int ensure_unary();
    CrfDev begin_iteration();
    void end_iteration(int with_map);
    bool launch_sized(const Schedule &run, LeanPrep *prep);
};

}  // namespace lccrf

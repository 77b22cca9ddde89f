/*
 * lccrf.h -- C-ABI of the MI355X-native dense-CRF mean-field path.
 *
 * Drop-in boundary for ONE hot path of LC-CRF-SLAM: the per-frame dense-CRF inference
 * that labels ORB keypoints static / dynamic inside Tracking::DynamicDetectionWithCRF
 * (reference src/Tracking.cc:1919-1930).  The entry points are exactly what a binding
 * of the reference's own operator interface for this path needs -- the two abstract
 * classes of Thirdparty/DenseCRF/include/densecrf_base.h:
 *
 *      class PairwisePotential   (densecrf_base.h:12-19)
 *      class DenseCRF            (densecrf_base.h:22-92)
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns
 * LCCRF_OK (0) or a negative lccrf_status; lccrf_last_error() gives the detail for
 * the calling thread.  There is NO CPU fallback behind this ABI: without a usable
 * gfx950 device every call that needs one fails with LCCRF_E_NO_DEVICE.
 *
 * Threading: handles are thread-compatible (one handle per thread at a time), like
 * the reference's stack-local per-frame objects.
 *
 * Layouts (all little-endian, densely packed):
 *   unary / probability : float32 [N][L]   "x0l0 x0l1 .. x1l0 .." (densecrf_base.h:56)
 *   label / map         : int16   [N]      -1 = unknown (densecrf3d.h:119)
 *   features            : float32 [N][d]   already divided by the kernel's stdev
 *                                          (pairwise3d.h:41-44,64-66 do that division)
 */
#ifndef LCCRF_H
#define LCCRF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCCRF_ABI_VERSION 3   /* 3: lccrf_batch_last_prepare, lccrf_batch_get_stream, LCCRF_OPT_EVENT_TIMING, lccrf_batch_synchronize scoped to the batch's streams; 2: lccrf_batch_get_fused_shape, the asynchronous host path of the batch API, lccrf_set_option's option 3 (LCCRF_OPT_COPY_THREADS) */
#define LCCRF_MAX_KERNELS 8      /* pairwise terms per CRF                        */
#define LCCRF_MAX_DIMS    8      /* feature dimensions per kernel (reference uses <= 6) */
#define LCCRF_MAX_LABELS  64

typedef enum lccrf_status {
    LCCRF_OK            =  0,
    LCCRF_E_INVALID     = -1,    /* bad argument (NULL, negative size, d/L out of range) */
    LCCRF_E_NO_DEVICE   = -2,    /* no gfx950 device / HIP runtime unusable              */
    LCCRF_E_HIP         = -3,    /* a HIP call failed; see lccrf_last_error()            */
    LCCRF_E_NOMEM       = -4,
    LCCRF_E_STATE       = -5,    /* call order violated (e.g. inference before unary)    */
    LCCRF_E_CAPACITY    = -6     /* more kernels / frames / points than created for      */
} lccrf_status;

int          lccrf_abi_version(void);
const char  *lccrf_last_error(void);
int          lccrf_device_count(int *count);

/* ======================================================================================
 * 1. Object API -- one CRF, host buffers in / host buffers out.
 *    Mirrors DenseCRF3D<M> + PottsPotential3D<M,F> as used at src/Tracking.cc:1920-1930.
 * ==================================================================================== */
typedef struct lccrf_crf *lccrf_handle;

/* DenseCRF3D<M>::DenseCRF3D(int N)              densecrf3d.h:23-28   (M = n_labels)   */
int  lccrf_create(lccrf_handle *out, int device_id, int n_points, int n_labels);
/* ~DenseCRF3D / ~DenseCRF (owns its pairwise terms)  densecrf3d.h:30-36, base.h:41-45.
 * The reference constructs and destroys one CRF per frame (src/Tracking.cc:1920); to keep that
 * pattern cheap a destroyed handle's device memory, stream and pinned staging are parked and
 * reused by the next lccrf_create of a compatible size.  lccrf_trim_cache() frees the parked
 * handles (returns how many), and with them the staging areas (pinned host and device memory,
 * stream) that lccrf_pose_optimization, lccrf_unary_build and lccrf_bf_match keep between calls
 * and only ever grow; the next call of each tool allocates what it needs afresh.            */
void lccrf_destroy(lccrf_handle h);
int  lccrf_trim_cache(void);

/* Options (no reference counterpart; none can change a result).
 *   LCCRF_OPT_SINGLE_WORKGROUP   value != 0: a frame is never given two workgroups.  By default a single two-kernel frame (and a
 *       batch of up to 64) runs as TWO workgroups on two CUs, one per lattice build, handing tables over through device memory
 *       (-8 us at 2000 keypoints).  The main workgroup waits for its helper with a bounded poll: if the helper is not
 *       co-scheduled -- a GPU shared with other processes or streams whose kernels hold every CU -- the frame stalls for up to
 *       ~0.05-0.1 s (three frames of a 30 fps tracker) before it falls back to the ordinary path, with the same labels.  A tracker
 *       that shares its GPU sets this option and pays the 8 us instead.
 *   LCCRF_OPT_VERTEX_ORDER   (batches; 0 automatic = on, 1 on, 2 off; from the next lccrf_batch_build on) large frames (>= 8192 points,
 *       streaming engine) are built by SORTING the (point, corner) entries on the row-major code of their vertex in the basis of the
 *       lattice's own axes -- no hash table -- with the points processed in the same order: the vertices are numbered along those axes
 *       and a blur pass (permutohedral_cpu.h:663-679) touches half as many cache lines per gather (23 -> 19.5 us per pass over 8 frames of
 *       100 000 points, 0.61 -> 0.72 of the HBM peak).  2 selects round 3's build (hash table, vertices by first occurrence along a
 *       Z-order curve of the points).  Results never depend on how vertices are found or numbered.
 *   LCCRF_OPT_COPY_THREADS   (batches; 1 .. 64, default 8) host threads that copy the caller's arrays into the batch's pinned
 *       staging in lccrf_batch_set_inputs_host_async (one core copies ~10 GB/s, the PCIe link takes ~50).
 *   LCCRF_OPT_EVENT_TIMING   (batches; default 1) value 0: lccrf_batch_build / _inference / _run record no HIP events around their
 *       work and lccrf_batch_last_timing reads 0.  An event record is a packet of its own between two launches: ~20 us per call on a
 *       stream that is kept busy, 1-2 % of a 1.7 ms batch -- a replay loop that does not read the timings turns them off.
 *   LCCRF_OPT_FRAME_GENERAL   (default 0) value != 0: a handle or batch whose terms carry a label-compatibility matrix (sections 1e /
 *       2g) or a normalisation mode other than AFTER (sections 1g / 2g) may take the ONE-launch route of a fresh frame: lattice build,
 *       normalisation and inference in one kernel launch (csrc/frame_general.hip), the lattices never in HBM.  The four calls that
 *       take that route are affected -- lccrf_inference on a fresh handle, lccrf_run_converged, lccrf_batch_run and
 *       lccrf_batch_run_converged -- for two labels, one or two 2-D terms and frames of up to 2048 points (the largest n_points the
 *       host knows, else max_points): always one 1024-lane workgroup per frame, lccrf_get_engine / lccrf_batch_get_engine report 3,
 *       lccrf_batch_get_fused_shape 1024 / 1.  Q, the labels, the label bits and the convergence report are bit for bit those of the
 *       option off; a frame whose lattices do not fit the kernel's LDS is re-run with the same model on the route of the option off
 *       (lccrf_batch_get_fallback_frames counts it).  Every other call, shape and model -- Potts terms normalised AFTER above all --
 *       takes exactly the route it takes with the option off.  Off by default: what the route saves for a learnt model is measured in
 *       notes/frame_general.md, not yet across deployments.
 *   LCCRF_OPT_FUSED_BACKWARD   (default 0) value != 0: a backward call that asks for dL/dU and / or dL/dw alone (sections 1c and 2c,
 *       and the calls of sections 1d - 1f, 2d and 2h when nothing else is asked for) on two-label frames of up to 2048 points with one
 *       or two 2-D Potts terms normalised AFTER runs the replay and the sweep in ONE kernel launch (section 1j; csrc/fused_backward.hip).
 *       The gradients and the Q left behind are bit for bit those of the option off; everything else takes the route it takes today.
 *   LCCRF_OPT_FUSED_BACKWARD_LEARNT   (default 0) value != 0: the same for the requests LCCRF_OPT_FUSED_BACKWARD leaves out, feature
 *       gradients apart: a backward call on a handle or batch whose terms carry a label-compatibility matrix or a normalisation mode
 *       other than AFTER, and every call that asks for d_grad_compat or d_grad_model (Potts terms included) -- dL/dU, dL/dw and dL/dmu
 *       of two-label frames of up to 2048 points with one or two 2-D terms in ONE kernel launch (section 1k;
 *       csrc/fused_backward_general.hip), plus the two launches of d_grad_model's sums.  Bit for bit the results of the option off.  A
 *       Potts / AFTER request for dL/dU and / or dL/dw alone is LCCRF_OPT_FUSED_BACKWARD's and is not affected.
 *   LCCRF_OPT_FUSED_BACKWARD_FEATURES   (default 0) value != 0: the same for a backward call WITH feature gradients (sections 1d and 2d,
 *       and the calls of sections 1f and 2h that reduce to them: at least one non-NULL entry of d_grad_features, neither d_grad_compat
 *       nor d_grad_model, no matrix) on Potts terms normalised AFTER, n_iterations >= 1 -- dL/dU, dL/dw and every dL/df_k asked for of
 *       two-label frames of up to 2048 points with one or two 2-D terms in ONE kernel launch (section 1l;
 *       csrc/fused_backward_features.hip).  Bit for bit the results of the option off.  A request without a feature array is never
 *       this option's: options 6 and 7 select exactly what they selected.
 *   LCCRF_OPT_FUSED_MULTILABEL   (default 0) value != 0: a fixed count of iterations on lattices in HBM -- lccrf_inference on a handle
 *       whose lattices are built, lccrf_batch_inference, and lccrf_batch_run where it builds into HBM -- of frames with THREE TO EIGHT
 *       labels runs in ONE kernel launch, one 1024-lane workgroup per frame (csrc/fused_multilabel.hip; notes/fused_multilabel.md),
 *       instead of the streaming engine's launch per phase: one or two 2-D Potts terms normalised AFTER (no matrix, no mode), 3 or 4
 *       labels on frames of up to 2048 points, 5 to 8 labels on frames of up to 1024 (the largest n_points the host knows, else the
 *       capacity), lattices that fit the fused engine's plan, no locality mode.  A batch decides once, over its largest frame and
 *       lattices.  Q and the labels are bit for bit those of the option off; lccrf_get_engine / lccrf_batch_get_engine report 5 with
 *       engine 2's shape word, lccrf_batch_get_fused_shape 1024 and the points per lane (1 or 2), and lccrf_batch_set_engine(b, 2) is
 *       honoured for such a batch.  Everything else -- the converged calls, the gradients (whose replay streams), the stepwise calls,
 *       two labels, nine and more, matrices, modes, a 3-D term, larger frames -- takes exactly the route it takes with the option
 *       off.  Label bits exist for two labels only.  Takes effect with the next inference.  The same switch as bit
 *       LCCRF_MULTILABEL_POTTS of lccrf_set_multilabel_routes, whose other bit, LCCRF_MULTILABEL_LEARNT, moves the frames with
 *       matrices and modes (engine 6).
 * lccrf_set_option applies to one handle (set it after lccrf_create: a handle taken from the cache starts from the defaults) and is
 * per handle (or batch) only for LCCRF_OPT_VERTEX_ORDER, LCCRF_OPT_COPY_THREADS, LCCRF_OPT_EVENT_TIMING, LCCRF_OPT_FUSED_BACKWARD,
 * LCCRF_OPT_FUSED_BACKWARD_LEARNT and LCCRF_OPT_FUSED_BACKWARD_FEATURES;
 * lccrf_set_default_option applies LCCRF_OPT_SINGLE_WORKGROUP, LCCRF_OPT_FRAME_GENERAL or LCCRF_OPT_FUSED_MULTILABEL to every handle and batch created afterwards
 * in this process.                                                                                                             */
typedef enum lccrf_option {
    LCCRF_OPT_SINGLE_WORKGROUP = 1,
    LCCRF_OPT_VERTEX_ORDER     = 2,
    LCCRF_OPT_COPY_THREADS     = 3,
    LCCRF_OPT_EVENT_TIMING     = 4,
    LCCRF_OPT_FRAME_GENERAL    = 5,
    LCCRF_OPT_FUSED_BACKWARD  = 6,
    LCCRF_OPT_FUSED_BACKWARD_LEARNT = 7,
    LCCRF_OPT_FUSED_BACKWARD_FEATURES = 8,
    LCCRF_OPT_FUSED_MULTILABEL = 9
} lccrf_option;
int  lccrf_set_option(lccrf_handle h, int option, int value);
int  lccrf_set_default_option(int option, int value);

/* Which ONE-launch kernels a fixed count of iterations on frames of THREE TO EIGHT labels may take (lattices in HBM: lccrf_inference on
 * a handle whose lattices are built, lccrf_batch_inference, lccrf_batch_run where it builds into HBM).  A mask of routes, not an option
 * number: added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3), probe for the calls by symbol.  The follow-ups of these kernels --
 * the convergence form, the fresh-frame kernels -- get further BITS here, not option numbers.
 *   LCCRF_MULTILABEL_POTTS    IS LCCRF_OPT_FUSED_MULTILABEL: setting either is visible through the other; lccrf_set_option(h, 9, v) and
 *       the process-wide default touch this bit alone.  Potts terms normalised AFTER on k_multilabel, engine 5.
 *   LCCRF_MULTILABEL_LEARNT   (off by default; no process-wide default, and a handle taken from the cache starts without it) frames
 *       of which at least one term carries a label-compatibility matrix (sections 1e / 2g) or a normalisation mode other than AFTER
 *       (sections 1g / 2g) run on k_multilabel_general (csrc/fused_multilabel_general.hip; notes/fused_multilabel.md section 6), one
 *       1024-lane workgroup per frame: one or two 2-D terms, 3 or 4 labels on frames of up to 2048 points, 5 to 8 labels on frames of
 *       up to 1024 (the largest n_points the host knows, else the capacity), lattices that fit the fused engine's plan, no locality
 *       mode; a batch decides once, over its largest frame and lattices.  Q and the labels are bit for bit those of the bit off (the
 *       streaming engine's general step); lccrf_get_engine / lccrf_batch_get_engine report 6 with engine 5's shape word,
 *       lccrf_batch_get_fused_shape 1024 and the points per lane, and lccrf_batch_set_engine(b, 2) is honoured for such a batch.
 * The two bits are independent: each moves its own frames and no others.  Everything else -- the converged and the stepwise calls, the
 * gradients (whose replay streams), two labels, nine and more, a 3-D term, locality mode, an engine preference of 1, frames beyond the
 * plan -- keeps its route, bit for bit.  Takes effect with the next inference.
 * LCCRF_E_INVALID, with nothing written, for a NULL handle, a NULL `routes` or bits beyond the two.                                 */
enum { LCCRF_MULTILABEL_POTTS = 1, LCCRF_MULTILABEL_LEARNT = 2 };
int  lccrf_set_multilabel_routes(lccrf_handle h, unsigned routes);
int  lccrf_get_multilabel_routes(lccrf_handle h, unsigned *routes);

/* DenseCRF::setUnaryEnergy(const float*)        densecrf3d.h:41-43                    */
int  lccrf_set_unary(lccrf_handle h, const float *unary);
/* DenseCRF::setUnaryEnergyFromLabel(const short*, float*)   densecrf3d.h:107-130;
 * conf has n_labels entries.  The scalar overload (densecrf3d.h:100-105) is the same
 * call with every entry equal.                                                         */
int  lccrf_set_unary_from_label(lccrf_handle h, const int16_t *label, const float *conf);

/* new PottsPotential3D<M,F>(features, N, w) + DenseCRF::addPairwiseEnergy(p)
 * pairwise3d.h:20-28 (lattice init + normalisation), densecrf_base.h:54.
 * The CRF owns the term.  d = F.  Kernels are applied in the order added.              */
int  lccrf_add_pairwise(lccrf_handle h, const float *features, int d, float w);

/* PottsPotential3D<M,2>::appearanceKernel(N, w, vobserv, verror, sd1, sd2)
 * pairwise3d.h:37-48 : features (vobserv/sd1, verror/sd2), then the ctor above.        */
int  lccrf_add_appearance_kernel(lccrf_handle h, float w, const float *vobserv,
                                 const float *verror, float sd_observ, float sd_error);
/* PottsPotential3D<M,2>::smoothKernel(N, w, points3d, points2d, sd3d, sd2d)
 * pairwise3d.h:51-71 : only the 2-D branch is live -> features (u/sd2d, v/sd2d).
 * xy is [N][2] (cv::Point2f layout).                                                   */
int  lccrf_add_smooth_kernel(lccrf_handle h, float w, const float *xy, float sd2d);

/* DenseCRF::startInference()                    densecrf_base.h:78-80                 */
int  lccrf_start_inference(lccrf_handle h);
/* DenseCRF::stepInference(float relax)          densecrf_base.h:82-91                 */
int  lccrf_step_inference(lccrf_handle h, float relax);
/* DenseCRF3D<M>::buildMap()                     densecrf3d.h:136-151                  */
int  lccrf_build_map(lccrf_handle h);
/* DenseCRF::inference(n_iterations, with_map, relax)   densecrf_base.h:65-73
 * Frames of >= 8192 points (far beyond a SLAM frame: BASELINE config 5) run it in the streaming engine's LOCALITY MODE -- the points
 * in an internal order, the lattice built by sorting, the first blur passes inside the splat -- when the
 * lattices are first needed by this call.  Results are the same bits in the caller's order.  The entry points that expose or
 * continue from per-point lattice state (lccrf_start_inference / lccrf_step_inference, lccrf_pairwise_apply, lccrf_step_init,
 * lccrf_get_norm / _lattice / _unary) work on the plain build: used first, the handle is built that way and stays so; used after an
 * inference() in locality mode, the lattices are re-built once (same results, one extra build).                       */
int  lccrf_inference(lccrf_handle h, int n_iterations, int with_map, float relax);

/* DenseCRF::getMap() / getProbability()         densecrf_base.h:74-75
 * (copies out; the reference returns pointers into object-owned buffers)
 * lccrf_get_map right behind lccrf_inference(h, n, 1, ...) is the tracker's sequence and the fast one: the frame kernel's
 * last stores are the labels, into pinned host memory, and the call takes them as they arrive instead of waiting for the
 * stream.  Same results as any other order of calls.                                    */
int  lccrf_get_map(lccrf_handle h, int16_t *map_out);
int  lccrf_get_probability(lccrf_handle h, float *prob_out);

/* Which engine the last lccrf_inference on the handle ran on (no reference counterpart; as lccrf_batch_get_engine for batches).
 * Added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.
 *   *engine   1 the streaming engine (one launch per phase); 2 the fused engine (lattices in HBM, inference in one launch);
 *             3 one launch per frame (lattice build + inference); 4 the fused engine's kernel for terms with a label-compatibility
 *             matrix (section 1e) or a normalisation mode other than AFTER (section 1g); 5 its kernel for frames of three to eight
 *             labels (LCCRF_OPT_FUSED_MULTILABEL); 6 that kernel's form for terms with a matrix or a mode
 *             (LCCRF_MULTILABEL_LEARNT).  For 3 it is the value after a late-bound
 *             run has settled: a frame that did not fit the one-launch kernel's plan reports what it was re-run on.  A handle
 *             that has not run lccrf_inference reports 1.
 *   *shape    (may be NULL) for engines 2, 4, 5 and 6: lanes per workgroup in bits 0-15, points per lane in bits 16-19, and 1 in bit 20
 *             when the first term's splat rows took the chain path; otherwise 0.
 * Report only: nothing depends on the value, and the call does no device work beyond settling a pending one-launch run.
 * LCCRF_E_INVALID for a NULL handle or a NULL `engine`.                                                                          */
int  lccrf_get_engine(lccrf_handle h, int *engine, int *shape);

/* ---- the reference's two plug-in points, on HOST arrays (device in, device out behind the call) ------------------
 * PairwisePotential::apply(out_values, in_values, tmp)        densecrf_base.h:18, pairwise3d.h:73-78
 *   out_values[i][k] += w * norm[i] * compute(in_values)[i][k] for pairwise term `kernel` of this CRF (both
 *   [N][n_labels]; the reference's `tmp` scratch lives on the device).  This is the one pure virtual of the
 *   reference's plug-in class: a caller that mixes its own PairwisePotential subclasses with ours drives the
 *   mean-field step itself (densecrf_base.h:82-91) and calls this for our terms.                               */
int  lccrf_pairwise_apply(lccrf_handle h, int kernel, float *out_values, const float *in_values);
/* DenseCRF's protected virtuals (densecrf_base.h:34-36), for exactly that kind of caller:
 *   expAndNormalize(out, in, scale, relax)    densecrf3d.h:70-98   (out is read too when relax != 1)
 *   stepInit(): next = -unary                 densecrf3d.h:154-158
 *   buildMap() on a given probability array   densecrf3d.h:136-151                                            */
int  lccrf_exp_and_normalize(lccrf_handle h, float *out, const float *in, float scale, float relax);
int  lccrf_step_init(lccrf_handle h, float *next_out);
int  lccrf_map_of(lccrf_handle h, const float *prob, int16_t *map_out);
/* PermutohedralLatticeCPU::init(features, d, N) + compute(out, in, value_size)   permutohedral_cpu.h:241-424,634-699
 * the bare lattice filter (splat, d+1 blurs, slice; no normalisation, no weight) with any value_size in
 * [1, LCCRF_MAX_LABELS]; n_vertices (may be NULL) receives the lattice size M_.                                */
int  lccrf_lattice_filter(int device_id, const float *features, int n_points, int d, const float *in,
                          int value_size, float *out, int *n_vertices);

/* Parity probes (no reference API; the reference keeps these protected):
 * lattice size M_ (permutohedral_cpu.h:398) and PottsPotential3D::norm_ (pairwise3d.h:18).
 * offset/bary are [N][d+1], nbr is [d+1][V][2]; any output pointer may be NULL.         */
int  lccrf_get_lattice_size(lccrf_handle h, int kernel, int *n_vertices);
int  lccrf_get_norm(lccrf_handle h, int kernel, float *norm_out);
int  lccrf_get_lattice(lccrf_handle h, int kernel, int32_t *offset_out, float *bary_out,
                       int32_t *nbr_out);
int  lccrf_get_unary(lccrf_handle h, float *unary_out);

/* ======================================================================================
 * 1b. Object API on DEVICE arrays -- the reference's GPU interface (Thirdparty/DenseCRF/README.md "GPU Version": DenseCRFGPU<M>,
 *     PottsPotentialGPU<M,F>::FromImage, "all pointers should be device pointers") on the same handles as section 1.
 *
 * Contract of every _device entry point (and of lccrf_add_image_kernel's image):
 *   - device arrays are read and written in order on the handle's own stream (lccrf_get_stream); a call returns without waiting
 *     for that work (a call behind an inference that has not been settled yet settles it first, as every entry point of section 1
 *     does; the first use of new terms' lattices waits once for their sizes);
 *   - inputs are consumed by work the call enqueues: the caller may overwrite or free them once the handle's stream has passed that
 *     work (lccrf_synchronize, or an event recorded on lccrf_get_stream's stream).  Nothing keeps a pointer to a caller's array;
 *   - the library does not synchronise with other streams: a producer on another stream must have finished, or the caller makes
 *     the handle's stream wait for it (an event);
 *   - every pointer is checked with hipPointerGetAttributes before anything is enqueued: device memory of the handle's device, or
 *     host memory registered as pinned (hipHostMalloc / hipHostRegister) whose device address is the pointer itself.  Anything
 *     else -- plain pageable host memory above all, which a kernel cannot read with XNACK off -- is refused with LCCRF_E_INVALID,
 *     and so is an array the runtime knows to be shorter than what the call reads or writes.  NULL is accepted for n_points == 0.
 * Results: after lccrf_inference the device results are complete behind lccrf_synchronize (which also settles the one-launch
 * kernel's per-frame fallback, see lccrf_batch_run) or any call of section 1 that reads results.
 *
 * The reference's GPU example, its type names patched (include/lccrf_densecrf_gpu.hpp):
 *      DenseCRFGPU<M> crf(W * H);                                              lccrf_create + lccrf_device_buffers
 *      crf.setUnaryEnergyFromLabel(labelGPU, 0.5);                             lccrf_set_unary_from_label_device
 *      crf.addPairwiseEnergy(PottsPotentialGPU<M, 2>::FromImage<>(W, H, 3, 3));                        lccrf_add_image_kernel, NONE
 *      crf.addPairwiseEnergy(PottsPotentialGPU<M, 5>::FromImage<float>(W, H, 10, 60, rgbFeatGPU, 20)); lccrf_add_image_kernel, F32
 *      crf.inference(10, true);                                                lccrf_inference (+ lccrf_synchronize)
 *      short *mapGPU = crf.getMap();                                           lccrf_device_buffers' d_map
 * ==================================================================================== */
/* The handle's stream (a hipStream_t), as lccrf_batch_get_stream; lccrf_synchronize waits for that stream only.             */
int  lccrf_get_stream(lccrf_handle h, void **stream);
int  lccrf_synchronize(lccrf_handle h);

/* DenseCRF::setUnaryEnergy on a device array [N][L] (copied into the handle on its stream).                                  */
int  lccrf_set_unary_device(lccrf_handle h, const float *d_unary);
/* setUnaryEnergyFromLabel on a device label array [N]: the unary kernel is enqueued at once (labels outside [0, L) count as
 * unknown, as in the host path).  conf: n_labels values in host memory, or in device memory (read before the call returns).  */
int  lccrf_set_unary_from_label_device(lccrf_handle h, const int16_t *d_label, const float *conf);
/* new PottsPotential3D<M,F>(d_features, N, w) + addPairwiseEnergy: d_features [N][d] on the device, copied into the handle.   */
int  lccrf_add_pairwise_device(lccrf_handle h, const float *d_features, int d, float w);
/* PottsPotentialCPU<M,F>::FromImage(width, height, w, posdev, image, featuredev)   pairwise_cpu.h:33-51, the image on the device.
 * Point i = y * width + x; width * height must equal n_points.
 *   LCCRF_IMAGE_NONE : d = 2, features (x, y) / posdev; d_image must be NULL
 *   LCCRF_IMAGE_U8   : d = 5, features (x, y) / posdev, (r, g, b) / featuredev from uint8 RGB [N][3] (HWC)
 *   LCCRF_IMAGE_F32  : the same from float RGB [N][3]
 * posdev (and featuredev with an image) must be positive and finite, else LCCRF_E_INVALID.                                    */
#define LCCRF_IMAGE_NONE 0
#define LCCRF_IMAGE_U8   1
#define LCCRF_IMAGE_F32  2
int  lccrf_add_image_kernel(lccrf_handle h, int width, int height, float w, float posdev, const void *d_image, int image_format,
                            float featuredev);
/* The handle-owned HBM arrays behind the reference's members unary_, current_, next_, tmp_, map_ (densecrf_base.h:27-28); any
 * argument may be NULL.  The first call moves the handle's labels from pinned host memory to HBM (d_map, allocated with the
 * handle): from then on inference(with_map), lccrf_build_map and the steps write them there, and lccrf_get_map copies them out.
 * d_current is Q, d_next the engine's own next array (overwritten by every step, as next_ is), d_tmp a scratch array that the
 * host-array plug-ins of section 1 use too.  The pointers stay valid until lccrf_destroy; a handle taken from the cache by
 * lccrf_create starts with its labels in host memory again.                                                                   */
int  lccrf_device_buffers(lccrf_handle h, const float **d_unary, float **d_current, float **d_next, float **d_tmp, int16_t **d_map);
/* The plug-in points of section 1 (lccrf_pairwise_apply, lccrf_exp_and_normalize, lccrf_step_init, lccrf_map_of) on device
 * arrays: the same kernels on the caller's pointers, no copy and no synchronisation.                                          */
int  lccrf_pairwise_apply_device(lccrf_handle h, int kernel, float *d_out_values, const float *d_in_values);
int  lccrf_exp_and_normalize_device(lccrf_handle h, float *d_out, const float *d_in, float scale, float relax);
int  lccrf_step_init_device(lccrf_handle h, float *d_next_out);
int  lccrf_map_of_device(lccrf_handle h, const float *d_prob, int16_t *d_map_out);

/* ======================================================================================
 * 1c. Gradients of inference() -- reverse mode through DenseCRF::inference (densecrf_base.h:65-91) with respect to the unary
 *     energies and the weight of every pairwise term (the reference's README: "does not support gradient computation").
 *
 * The forward, for unary U [N][L], T = n_iterations, r = relax, term k with norm n_k, weight w_k and lattice filter
 * Phi_k = alpha S^T B_d .. B_1 B_0 S (S the splat, B_j the Jacobi blur pass along axis j, alpha = 1/(1+2^-d)):
 *      Q_0 = softmax(-U)
 *      x_t = -U + sum_k w_k n_k . Phi_k(Q_{t-1})                        t = 1 .. T
 *      P_t = softmax(x_t),   Q_t = P_t (r == 1)   or   (1-r) Q_{t-1} + r P_t
 * Given G_T = dL/dQ_T, with <.,.> the per-point sum over labels and P_0 = Q_0:
 *      for t = T .. 1:
 *          gamma_t   = r P_t . (G_t - <G_t, P_t>)
 *          dL/dU    -= gamma_t
 *          dL/dw_k  += sum_{i,l} gamma_t . n_k . Phi_k(Q_{t-1})
 *          G_{t-1}   = (1-r) G_t + sum_k w_k Phi_k^T(n_k . gamma_t)
 *      dL/dU -= P_0 . (G_0 - <G_0, P_0>)
 * Phi_k^T = alpha S^T B_0 .. B_d S: the same splat and slice, the blur passes in REVERSE axis order (every pass is symmetric -- n1(v)
 * = u exactly when n2(u) = v -- but the passes do not commute on a sparse lattice, so Phi_k is not).  The derivative treats the
 * reference's polynomial fast_exp (densecrf3d.h:51-67) as exp: the softmax Jacobian is formed from the forward's own P_t, computed
 * with the forward's arithmetic.  Not differentiated: the MAP labels, and the label-and-confidence form of the unary (take dL/dU
 * and chain through that formula yourself).  The features (kernel bandwidths, positions, embeddings): section 1d.                 */

/* PottsPotential3D::w_ of term `kernel` (set after construction).  The lattice and norm stay; the next inference equals, bit for
 * bit, that of a handle built with weight w.  Anything derived from w (the fused engines' w*norm products, prepared launch records)
 * is invalidated.                                                                                                              */
int  lccrf_set_pairwise_weight(lccrf_handle h, int kernel, float w);
/* Gradients of lccrf_inference(h, n_iterations, -, relax) on the handle's current unary and terms.
 * d_grad_prob [N][L] = dL/dQ_T, d_grad_unary [N][L] (overwritten), d_grad_weights [K] (overwritten; may be NULL).  Device arrays,
 * checked as in section 1b, on the handle's stream, no host synchronisation (but the first use of new terms' lattices, which waits
 * once for their sizes, as every entry point does).
 *   - Self-contained: the forward is replayed on the step path (lccrf_start_inference + n_iterations x lccrf_step_inference; frames
 *     of >= 8192 points use the plain build, re-built once after a locality-mode inference()), keeping Q_0 .. Q_{T-1}; Phi_k(Q_{t-1})
 *     and P_t are recomputed in the sweep.  No earlier lccrf_inference is needed.
 *   - Afterwards Q (lccrf_device_buffers' d_current, lccrf_get_probability) holds exactly what lccrf_inference(h, n_iterations, 0,
 *     relax) would have left, bit for bit.
 *   - Deterministic: no float atomics; the weight gradient is a sum of per-workgroup partials in a fixed order -- the same bits
 *     from run to run.
 *   - Memory: a handle-owned HBM area of 4 * (N4*L*(T + K + 1) + max(T,1) * K * B) bytes, N4 = N rounded up to a multiple of 4
 *     (the phantom points' rows, kept zero), B = ceil(N / R) workgroups of
 *     R = 256, 128, 64, 32, 16 points for L <= 4, 8, 16, 32, 64 (N = 2000, L = 2, K = 2, T = 5: 128 KB; 320 x 240, L = 21, K = 2,
 *     T = 10: 84 MB).  Allocated by the first call that needs more, freed by lccrf_destroy (and lccrf_trim_cache); a failed
 *     allocation returns LCCRF_E_NOMEM and leaves the handle as it was.  lccrf_inference never allocates it.
 *   - Errors: LCCRF_E_INVALID for n_iterations < 0, a relax that is not finite, or a device array that section 1b refuses;
 *     LCCRF_E_STATE without unary energies.  K = 0 is legal (d_grad_weights then receives nothing).                             */
int  lccrf_inference_backward(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                              float *d_grad_weights);

/* ======================================================================================
 * 1d. Gradients of inference() with respect to the FEATURES of the pairwise terms: one [N][d_k] array per term.  Everything a caller
 *     derives features from -- the kernel standard deviations (feature = raw / stdev), an embedding network -- is a chain rule on
 *     top of it (lc-crf-slam_amd/autograd.py: mean_field_features, LearnedKernelCRF).
 *     Sections 1d and 2d were added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for them by symbol.
 *
 * What is differentiated.  The lattice filter is continuous in the features and piecewise smooth: while no point leaves its simplex
 * the vertices, the neighbour tables and every rank are constant, and the barycentric weight b_ic of point i at corner c (vertex
 * v_ic) is LINEAR in the point's features (permutohedral_cpu.h:304-366).  The gradient is that derivative -- one-sided where a point
 * sits exactly on a simplex face or a rounding tie -- i.e. the exact derivative of what the library computes, not that of the
 * Gaussian the lattice approximates.  With section 1c's notation, V = S x the splat, B = B_d .. B_0, B^T = B_0 .. B_d:
 *      d<y, Phi_k(x)> / d b_ic = alpha_k (<y_i, (B S x)[v_ic]> + <x_i, (B^T S y)[v_ic]>)              <.,.> over the labels
 *      for t = T .. 1:   g_b[k][i][c] += alpha_k w_k (<y_i, (B S Q_{t-1})[v_ic]> + <Q_{t-1},i, (B^T S y)[v_ic]>),   y = n_k . gamma_t
 *                        g_n[k][i]    += w_k <gamma_t,i, Phi_k(Q_{t-1})_i>
 *      the norm n_k = 1 / (Phi_k(1) + 1e-20), with a_k = -n_k^2 . g_n[k]:
 *                        g_b[k][i][c] += alpha_k (a_k,i (B S 1)[v_ic] + (B^T S a_k)[v_ic])
 *      dL/df_im = sum_q g_b[k][i][q] . scale_m / (d+1) . (E[e(q)][m] - E[e(q-1)][m]),   E[j][m] = [m >= j] - j [m == j-1], E[0][m] = 1,
 *      e(q) the coordinate of the elevated point whose rank is d - q (indices mod d+1), scale_m as permutohedral_cpu.h:282-285.
 * At n_iterations = 0 nothing depends on the features: the gradient is exactly 0.
 *
 * d_grad_features: HOST array of K device pointers; d_grad_features[k] is [N][d_k], overwritten.  An entry may be NULL: that term's
 * feature gradient (and its extra launches) is skipped, the other terms' bits do not change.  d_grad_features == NULL makes the
 * call lccrf_inference_backward.  d_grad_unary and d_grad_weights receive the bits lccrf_inference_backward gives; either may be
 * NULL here.  Everything else is section 1c's contract: self-contained (the forward is replayed), device arrays checked as in
 * section 1b, on the handle's stream, no host synchronisation beyond the one-time learning of new lattices' sizes, frames in
 * locality mode re-built the plain way with results in the caller's point order, Q afterwards as lccrf_inference(h, T, 0, relax)
 * leaves it, the same errors, and a rejected call leaves the handle as it was.
 *   - Deterministic: no float atomics.  Every g_b[k][i][c] has one owner and is accumulated in the order t = T .. 1, slice-side
 *     part before splat-side part, the norm part last, labels 0 .. L-1 inside a dot product: the same bits from run to run.
 *   - Launches: per iteration and term two corner-dot kernels more than section 1c; per term, after the loop, two filters of value
 *     width 1 (splat + d+1 blur passes each), two corner-dot kernels, and two small per-point kernels.
 *   - Memory: section 1c's area grows by 4 * sum over the terms asked for of N4 * (d_k + 2) bytes (g_b and g_n), and by 4 * N4 * L
 *     when d_grad_unary is NULL: 4 * (N4*L*(T + K + 1) + max(T,1)*K*B + sum_k N4*(d_k + 2)) bytes in all (N = 2000, L = 2, K = 2
 *     of d = 2, T = 5: 128 KB + 64 KB).  Allocated as section 1c's: by the first call that needs more, never by lccrf_inference.
 *   - In ONE launch under LCCRF_OPT_FUSED_BACKWARD_FEATURES (section 1l): the same bits, the same area, one kernel.                  */
int  lccrf_inference_backward_features(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                       float *d_grad_weights, float *const *d_grad_features);

/* ======================================================================================
 * 1e. Label-compatibility matrices -- a per-term matrix mu_k [L][L] in place of the Potts term's identity: the semimetric / matrix
 *     compatibilities of the dense-CRF formulation, the learnt compatibility transform of CRF-as-RNN
 *     (lc-crf-slam_amd/autograd.py: mean_field_compat, CompatMeanFieldCRF).  Added WITHOUT a step of LCCRF_ABI_VERSION (it stays
 *     3): probe for these three by symbol.
 *
 * Meaning.  Term k with matrix mu_k contributes
 *      next[i][l] += w_k . n_k[i] . sum_{l'} mu_k[l][l'] . Phi_k(Q)[i][l']
 * where a Potts term adds w_k . n_k[i] . Phi_k(Q)[i][l] (PairwisePotential::apply, pairwise3d.h:73-78).  Lattice, norm and weight
 * are those of the Potts term.  Arithmetic, per point and label, in fp32 with every product and every sum rounded on its own (no
 * FMA):   s = 0;  for l' = 0 .. L-1:  s = s + mu[l][l'] * t[l'];   next = base + w * norm * s,   t[l'] the sliced value the Potts
 * term forms.  A term whose matrix is the identity therefore gives, bit for bit, what the term gives without a matrix.
 *
 * Honoured by lccrf_inference (locality mode at >= 8192 points included), lccrf_start_inference / lccrf_step_inference,
 * lccrf_pairwise_apply / _device (the `apply` of that term), lccrf_inference_backward (dL/dU and dL/dw are then those of the forward
 * with the matrices) and lccrf_inference_backward_compat.  While any term of a handle has a matrix, the one-launch frame kernel and
 * the fused engine, which hard-wire Potts, are not taken (LCCRF_OPT_FRAME_GENERAL: a fresh two-label frame of up to 2048 points takes
 * the one-launch route's kernel for such terms, engine 3, same bits).  lccrf_inference on the shape the project exists for -- L = 2, one or two
 * 2-D terms, a frame of up to 2048 points whose lattices fit the fused engine's plan -- then runs in ONE launch on the fused
 * engine's kernel for such terms (lccrf_get_engine reports 4), with the same bits.  Everything else -- other L, d or K, 2049 points
 * and more, locality mode, lccrf_start_inference / lccrf_step_inference, the plug-in entry points, every backward call's replay (but under
 * LCCRF_OPT_FUSED_BACKWARD_LEARNT, section 1k: the replay and the sweep of such a frame in one launch) --
 * runs on the streaming engine with the matrix applied inside the slice kernel, which takes the Potts slice kernel's place: the
 * step issues no launch more than the streaming engine's general, L-label step (at L = 2 that is more than the two-label
 * specialisation issues).  The C++ mirror lccrf_densecrf.hpp sets a matrix per potential (PottsPotentialHIP::setCompatibility).
 * The batch API has the same setter, one matrix per term shared by every frame (section 2g); the gradients of such a batch are
 * section 2h's (sections 2c and 2d refuse it), and lccrf_densecrf_gpu.hpp is unchanged.  lccrf_inference_backward_features itself still returns
 * LCCRF_E_STATE on a handle with any matrix and leaves the handle as it was: the feature gradients of such a handle are
 * lccrf_inference_backward_all's (section 1f).                                                                                 */

/* compat: HOST [L][L], row-major (row = the label that receives, column = the label of the filtered distribution), copied during
 * the call and uploaded on the handle's stream; NULL removes the matrix (the term is Potts again).  Entries must be finite and
 * `kernel` a term of the handle, else LCCRF_E_INVALID.  May be called before or after the lattices are built and between
 * inferences: no lattice, norm or prepared launch record changes, and once the last matrix is removed the handle takes the fast
 * engines again and returns the bits it returned before.  A handle from lccrf_create -- a recycled one too -- has no matrices.  */
int  lccrf_set_pairwise_compatibility(lccrf_handle h, int kernel, const float *compat);
/* *is_set = 1 if term `kernel` has a matrix, else 0; compat_out (HOST [L][L], may be NULL) receives it -- the identity for a Potts
 * term.  No device work.                                                                                                        */
int  lccrf_get_pairwise_compatibility(lccrf_handle h, int kernel, float *compat_out, int *is_set);
/* lccrf_inference_backward plus d_grad_compat, DEVICE [K][L][L] (overwritten) = dL/dmu_k.  With section 1c's notation and
 * Phi~_k = Phi_k(Q_{t-1}):
 *      x_t               = -U + sum_k w_k n_k . (Phi~_k mu_k^T)
 *      dL/dw_k          += sum_{i,l} gamma_t[i][l] . n_k[i] . sum_{l'} mu_k[l][l'] Phi~_k[i][l']
 *      dL/dmu_k[l][l']  += sum_i w_k . gamma_t[i][l] . n_k[i] . Phi~_k[i][l']
 *      G_{t-1}           = (1-r) G_t + sum_k w_k Phi_k^T( n_k . (mu_k^T gamma_t) )
 * For a term without a matrix d_grad_compat[k] is the derivative at mu_k = I (where learning starts from a Potts model).  At
 * n_iterations = 0 it is exactly 0.  d_grad_compat == NULL makes the call lccrf_inference_backward; d_grad_unary and d_grad_weights
 * may be NULL otherwise; they receive the bits lccrf_inference_backward gives on the same handle.  Everything else is section 1c's
 * contract: self-contained, device arrays checked as in section 1b, on the handle's stream, Q afterwards as
 * lccrf_inference(h, T, 0, relax) leaves it, the same errors.
 *   - Deterministic: no float atomics.  A frame's points are cut into C = min(ceil(N / 256), 128) contiguous chunks, one workgroup
 *     each; an entry of a chunk's partial has one owner and is added to in the order of the points, t = T .. 1, and the C partials
 *     are summed in order: the same bits from run to run.
 *   - Launches: per iteration and term one kernel more than section 1c (mu^T gamma and the partials of dL/dmu), one reduction at
 *     the end.
 *   - Memory: section 1c's area grows by 4 * (N4*L + K*C*L*L) bytes (gamma_t and the partials), plus 4 * N4*L when d_grad_unary
 *     is NULL: 4 * (N4*L*(T + K + 2) + max(T,1)*K*B + K*C*L*L) bytes in all (320 x 240, L = 21, K = 2, T = 10: 90 MB + 0.5 MB).
 *     lccrf_inference_backward on a handle with a matrix takes the same area.  Allocated as section 1c's.                      */
int  lccrf_inference_backward_compat(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                     float *d_grad_weights, float *d_grad_compat);

/* ======================================================================================
 * 1f. Everything at once: the gradients of inference() with respect to the unary, the weights, the FEATURES and the MATRICES of a
 *     handle whose terms may carry label-compatibility matrices, from one replay and one sweep -- what a CRF-as-RNN layer with
 *     learnt kernel bandwidths AND a learnt compatibility transform needs (lc-crf-slam_amd/autograd.py: mean_field_learned,
 *     LearnedCRF).  Added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.
 *
 * The gradients of lccrf_inference(h, n_iterations, -, relax) on the handle's current unary, terms and matrices.  With the notation
 * of sections 1c - 1e, Phi~_k = Phi_k(Q_{t-1}) and mu_k the term's matrix (I for a Potts term), dL/dU, dL/dw_k, dL/dmu_k and G_{t-1}
 * are section 1e's, and section 1d's formulas hold with two replacements:
 *      upstream row of the corner dots:   y = n_k . (mu_k^T gamma_t)                        in place of n_k . gamma_t
 *          g_b[k][i][c] += alpha_k w_k (<y_i, (B S Q_{t-1})[v_ic]> + <Q_{t-1},i, (B^T S y)[v_ic]>)
 *      norm adjoint:                      g_n[k][i] += w_k <gamma_t,i, (mu_k Phi~_k)_i>     in place of w_k <gamma_t,i, Phi~_k,i>
 * where (mu_k Phi~_k)_i[l] is the forward's own per-label sum, s = 0; s = s + mu[l][l'] * t[l'], l' = 0 .. L-1 (section 1e), and the
 * dot over l adds the labels in order 0 .. L-1.  The norm part after the loop (a_k = -n_k^2 . g_n[k]) and the map from dL/db to dL/df
 * are section 1d's, unchanged.  At n_iterations = 0 dL/df and dL/dmu are exactly 0.
 *
 * d_grad_features: HOST array of K device pointers, [N][d_k] each, overwritten; entries, or the array itself, may be NULL (that
 * term's feature gradient and its extra launches are skipped; the other outputs' bits do not change).  d_grad_compat: DEVICE
 * [K][L][L], overwritten, or NULL; for a term without a matrix it is the derivative at mu_k = I.  d_grad_unary and d_grad_weights
 * may be NULL.  On a handle with a matrix dL/dU, dL/dw and dL/dmu are, bit for bit, lccrf_inference_backward_compat's, and with
 * d_grad_features == NULL the call is that call.  On a handle without matrices and with d_grad_compat == NULL every output is, bit
 * for bit, lccrf_inference_backward_features's.  (Explicit identity matrices take the compatibility form: dL/df then agrees with the
 * Potts handle's to rounding, not by contract to the bit.)  Everything else is the contract of sections 1c - 1e: self-contained (the
 * forward is replayed), device arrays checked as in section 1b before anything is enqueued, on the handle's stream, no float atomics
 * and the same bits from run to run (every g_b, g_n and partial of dL/dmu keeps its one owner and its order of additions), Q
 * afterwards as lccrf_inference(h, T, 0, relax) leaves it, the same errors, a rejected call leaves the handle as it was, frames in
 * locality mode are re-built the plain way and return results in the caller's point order.  K = 0 is legal.
 *   - Launches: per iteration and term, the one kernel section 1e adds to section 1c and the two corner-dot kernels section 1d
 *     adds -- the slice-side one between that kernel (which leaves n_k . (mu_k^T gamma_t) where Phi~_k was) and the transposed
 *     filter; after the loop section 1d's norm part per term and section 1e's one reduction.
 *   - Memory: the union of the areas of sections 1d and 1e,
 *     4 * (N4*L*(T + K + 2) + max(T,1)*K*B + K*C*L*L + sum over the terms asked for of N4*(d_k + 2)) bytes, plus 4 * N4*L when
 *     d_grad_unary is NULL (N = 2000, L = 2, K = 2 of d = 2, T = 5: 144 KB + 0.3 KB + 64 KB = 209 KB).  Allocated as section 1c's. */
int  lccrf_inference_backward_all(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                  float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat);

/* ======================================================================================
 * 1g. Normalisation modes -- where a pairwise term applies its norm n_k = 1 / (Phi_k(1) + 1e-20): AFTER the filter (the reference's
 *     PottsPotential3D, pairwise3d.h:73-78, and the default), BEFORE it, SYMMETRICally (n^1/2 on either side: the form that keeps the
 *     effective kernel symmetric, and the default of the dense-CRF formulation this code descends from), or not at all
 *     (lc-crf-slam_amd/autograd.py: MeanFieldCRF / CompatMeanFieldCRF take `normalization`).  Added WITHOUT a step of
 *     LCCRF_ABI_VERSION (it stays 3): probe for these two by symbol.
 *
 * Meaning.  n is the term's norm exactly as before (lccrf_get_norm is the same in every mode), s[i] = sqrtf(n[i]) correctly rounded:
 *      mode         pre[i]    post[i]
 *      AFTER        -         n[i]
 *      BEFORE       n[i]      -
 *      SYMMETRIC    s[i]      s[i]
 *      NONE         -         -
 * Arithmetic, in fp32 with every product and every sum rounded on its own (no FMA): the filter's input is x[i][l] = pre[i] * Q[i][l],
 * rounded once (Q itself without a pre); t = Phi(x) is the unchanged splat, blur and slice; a term with a label-compatibility matrix
 * turns t into section 1e's sum s = s + mu[l][l'] * t[l']; then next = base + (w * post[i]) * t with a post, next = base + w * t
 * without one.  A term explicitly set to AFTER gives, bit for bit, what it gave before the call existed.
 *
 * Honoured by lccrf_inference (locality mode at >= 8192 points included: the factors follow the internal point order the norm
 * has), lccrf_start_inference / lccrf_step_inference, lccrf_pairwise_apply / _device (the `apply` of that term is
 * out += (w * post) * Phi(pre * in)), lccrf_inference_backward and lccrf_inference_backward_compat.  While any term of a handle is not
 * AFTER, the one-launch frame kernel and the fused engine are not taken -- exactly what a matrix of section 1e does, LCCRF_OPT_FRAME_GENERAL
 * included (that kernel forms the factors itself, from the norm it holds in a register).  lccrf_inference
 * on L = 2, one or two 2-D terms and a frame of up to 2048 points whose lattices fit the fused engine's plan runs in ONE launch on
 * the fused engine's kernel for such terms (lccrf_get_engine reports 4): the pre factors sit in registers beside w * post.
 * Everything else (section 1e lists it; a backward call's replay under LCCRF_OPT_FUSED_BACKWARD_LEARNT is section 1k's) runs on the
 * streaming engine's general L-label step, at L = 2 too: the pre factor is applied
 * inside the splat where it loads its input (no launch more, no scaled copy of Q), the post factor is the array the slice reads in
 * the norm's place.  Both give the same bits.  Once every term is AFTER again the handle takes the fast engines and returns the
 * bits it returned before.
 *
 * Gradients.  With a_k the term's post and b_k its pre, each 1 where the mode has none, and section 1e's notation:
 *      x_t        = -U + sum_k w_k . a_k . (mu_k applied to Phi_k(b_k . Q_{t-1}))
 *      dL/dw_k   += sum_{i,l} gamma_t . a_k . (mu_k Phi_k(b_k . Q_{t-1}))
 *      dL/dmu_k  += sum_i w_k . gamma_t[i][l] . a_k[i] . Phi_k(b_k . Q_{t-1})[i][l']
 *      G_{t-1}    = (1-r) G_t + sum_k w_k . b_k . Phi_k^T( a_k . (mu_k^T gamma_t) )
 * Determinism, memory and the contracts "self-contained" and "Q afterwards as lccrf_inference leaves it" are those of sections 1c
 * and 1e.  NOT differentiated: s and n with respect to the features -- lccrf_inference_backward_features, and
 * lccrf_inference_backward_all with a non-NULL d_grad_features, return LCCRF_E_STATE on a handle with any term that is not AFTER and
 * leave the handle as it was.  Section 1m's lccrf_inference_backward_modes differentiates them (section 2i for a batch).
 *
 * The C++ mirror lccrf_densecrf.hpp sets a mode per potential (PottsPotentialHIP::setNormalization).  The batch API has the same
 * setter, one mode per term shared by every frame (section 2g); the gradients of such a batch are section 2h's (sections 2c and 2d
 * refuse a batch with a term that is not AFTER), and lccrf_densecrf_gpu.hpp is unchanged.
 *   - Memory: one [N] float array per SYMMETRIC term (s, formed from n on the handle's stream when first needed after a build or a
 *     mode change) and one [N] array of 1.0f per handle with a BEFORE or NONE term (what the slice reads where such a term has no
 *     post: w * 1.0f is exact); both stay with the handle.  Nothing is allocated for a handle that never calls the setter.      */
typedef enum lccrf_normalization {
    LCCRF_NORMALIZE_AFTER     = 0,   /* default: the reference, pairwise3d.h:73-78 */
    LCCRF_NORMALIZE_BEFORE    = 1,
    LCCRF_NORMALIZE_SYMMETRIC = 2,
    LCCRF_NORMALIZE_NONE      = 3
} lccrf_normalization;
/* mode: an lccrf_normalization; LCCRF_E_INVALID for a NULL handle, a `kernel` that is not a term of the handle, or a mode outside
 * 0 .. 3.  May be called before or after the lattices are built and between inferences: no lattice, norm or prepared launch record
 * changes.  A handle from lccrf_create -- a recycled one too -- has every term at LCCRF_NORMALIZE_AFTER.                          */
int  lccrf_set_pairwise_normalization(lccrf_handle h, int kernel, int mode);
/* *mode = the lccrf_normalization of term `kernel`.  No device work.                                                             */
int  lccrf_get_pairwise_normalization(lccrf_handle h, int kernel, int *mode);

/* ======================================================================================
 * 1h. Convergence-driven inference -- "run until converged, at most max_iterations" in place of a fixed iteration count.
 *
 * Definitions.  Q_0 is what lccrf_start_inference leaves, Q_t is one lccrf_step_inference(relax) applied to Q_{t-1}, and
 *     d_t = max over i < N and l < L of fabsf(Q_t[i][l] - Q_{t-1}[i][l])      (fp32: one subtraction, one abs; a maximum of
 *                                                                              non-negative floats does not depend on the order
 *                                                                              it is taken in, so d_t is a defined bit pattern)
 *     c_t = the number of points whose MAP label differs between Q_t and Q_{t-1} (buildMap's rule, densecrf3d.h:136-151: the
 *           first maximum wins).
 * `criterion` is a mask of the bits below; with both set, both conditions must hold.  The run stops behind the first t in
 * 1 .. max_iterations at which every selected condition holds, else at t = max_iterations.  Per frame:
 *     Q, the labels and label bits (with_map)   those of Q_t -- bit for bit what lccrf_inference(h, t, with_map, relax) leaves
 *     iterations = t, delta = d_t, changed = c_t, converged = 1 when the criterion was met at t (at the cap too), 0 when the cap
 *     ended the run.
 * max_iterations == 0, or a frame of 0 points, gives Q_0 (nothing for the empty frame) and reports 0 / 0.0f / 0 / 0.
 * LCCRF_E_INVALID for a criterion outside 1 .. 3, max_iterations < 0, a tol that is negative or not finite, or a relax that is not
 * finite -- checked before the handle is looked at.  With non-finite Q the only promise is that the run ends no later than the cap.
 *
 * Engines.  A two-label handle with one or two 2-D Potts terms normalised AFTER, up to 4096 points and lattices that fit one
 * workgroup's LDS runs the whole call in ONE launch (csrc/fused_converge.hip): the stop decision falls inside the kernel, and
 * lccrf_get_engine reports 2 with the shape word.  Everything else -- other label counts or dimensions, more terms or points, a
 * term with a matrix (1e) or a normalisation mode (1g), locality mode, lattices beyond LDS -- runs the streaming engine's step
 * unchanged with a small comparison kernel behind each step; the host then reads ONE word per iteration (the number of frames still
 * running) behind a synchronisation of the call's stream.  lccrf_get_engine reports 1.  A HANDLE with a matrix or a mode takes this
 * streaming step even where lccrf_inference runs it in one launch (engine 4): the one-launch kernel for such terms run until
 * converged (csrc/fused_general_converge.hip) is taken by batches only (section 2g; a batch of max_frames = 1 included), and moving
 * the handle's converged call onto it is the follow-up.  The lattices are built and sized exactly as
 * by lccrf_inference on built lattices; THIS call never takes the one-launch build + inference kernel (section 1i's
 * lccrf_run_converged does) and neither reads, writes nor invalidates prepared launch records.
 *
 * Behind the call the handle is as after lccrf_inference(h, t, ...): lccrf_step_inference continues from Q_t, the getters return
 * Q_t and its labels, and lccrf_inference_backward(h, t, relax, ...) with the reported `iterations` is the gradient of the
 * converged result (the stop decision itself is piecewise constant and contributes nothing).
 * Added WITHOUT a step of LCCRF_ABI_VERSION: probe for the entry points by symbol.
 * ==================================================================================== */
#define LCCRF_STOP_DELTA  1   /* d_t <= tol  */
#define LCCRF_STOP_LABELS 2   /* c_t == 0    */
int  lccrf_inference_converged(lccrf_handle h, int max_iterations, int criterion, float tol, int with_map, float relax);
/* What the last lccrf_inference_converged on the handle reported; any pointer may be NULL.  Waits for the handle's stream.
 * LCCRF_E_STATE when no converged inference has run on the handle's current inputs.                                               */
int  lccrf_get_convergence(lccrf_handle h, int *iterations, float *delta, int *changed, int *converged);

/* ======================================================================================
 * 1i. Convergence-driven inference on a fresh frame in ONE launch -- section 1h's call for the tracker's sequence "build both
 * lattices, infer once, read the labels" (src/Tracking.cc:1920-1929).  Needs inputs only (unaries and every term's features).  A
 * handle lccrf_inference would run in one launch -- two labels, one or two 2-D Potts terms normalised AFTER, up to 4096 points,
 * automatic engine choice -- builds both lattices in LDS, normalises, and infers until converged in ONE kernel launch
 * (csrc/frame_converge.hip: one 1024-lane workgroup, as with LCCRF_OPT_SINGLE_WORKGROUP); the lattices never reach HBM, with_map
 * labels arrive in the handle's pinned array (lccrf_get_map right behind the call takes them as they land) and
 * lccrf_get_convergence returns the report.  lccrf_get_engine reports 3.
 *     Q, labels, label bits, report   bit for bit what lccrf_inference_converged leaves, i.e. what lccrf_inference(h, t, ...)
 *                                     leaves at the reported t; max_iterations == 0 and the empty frame as in section 1h
 * A frame the kernel cannot take -- lattices beyond one workgroup's LDS -- is found at the next synchronisation point and re-run
 * there with lccrf_inference_converged's engines; lccrf_get_engine then reports what it was re-run on (2 or 1).  A handle whose
 * lattices are already built and sized, or that lccrf_inference would not run in one launch, takes lccrf_inference_converged at
 * once -- a handle with a matrix (section 1e) or a mode (section 1g) among them, unless LCCRF_OPT_FRAME_GENERAL is set: then a frame
 * of up to 2048 points runs in one launch here too (csrc/frame_general.hip, engine 3), re-run on section 1h's engines if it does not
 * fit.  Errors and the state behind the call: section 1h's.  Added WITHOUT a step of LCCRF_ABI_VERSION: probe by symbol.
 * ==================================================================================== */
int  lccrf_run_converged(lccrf_handle h, int max_iterations, int criterion, float tol, int with_map, float relax);

/* ======================================================================================
 * 1j. The gradients of a tracker-sized frame in ONE launch -- LCCRF_OPT_FUSED_BACKWARD (off by default; per handle or batch).
 *
 * Section 1c's sweep is a launch per phase: about 150 launches of a few microseconds each for two 2-D terms and T = 5, which a frame
 * of 2000 keypoints cannot fill.  With the option set, a backward call runs the replay of the forward AND the reverse sweep in one
 * kernel launch, one 1024-lane workgroup per frame with the lattices' values in LDS (csrc/fused_backward.hip), when
 *   - the call asks for dL/dU and / or dL/dw only: lccrf_inference_backward and lccrf_batch_inference_backward, and the calls of
 *     sections 1d - 1f, 2d and 2h with neither feature gradients, nor d_grad_compat, nor d_grad_model, on a handle or batch without
 *     a label-compatibility matrix;
 *   - every term is a Potts term normalised AFTER the filter;
 *   - the frames are ones the fused engine's plan takes: two labels, one or two 2-D terms, at most 2048 active points (the largest
 *     n_points the host knows, else max_points), lattices inside one workgroup's LDS.  A batch decides once for all its frames, over
 *     its largest frame and lattices: one frame that does not fit, and the whole batch takes section 1c's sweep.
 * Everything else -- other label counts, dimensions and sizes, matrices, modes, feature and model gradients -- takes section 1c's
 * sweep as with the option off.  n_iterations = 0 may take either route.
 *   - Bit for bit: d_grad_unary (the zero rows beyond a frame's points included), d_grad_weights and the Q left behind are exactly
 *     those of the option off -- every product and sum of sections 1c / 2c is formed in the same order, the weight gradient's
 *     partials over the same 256-point blocks, reduced by the same walk and tree.  The option changes speed only.
 *   - Memory: section 1c's (2c's) area, nothing more; the per-term arrays of it are not touched on this route.
 *   - Argument checks, LCCRF_E_STATE, LCCRF_E_NOMEM and "a rejected call leaves the handle as it was" are section 1c's: the route is
 *     chosen behind them.  The lattices are built in HBM as section 1c needs them (a pending one-launch run is settled, a
 *     locality-mode build made plain).
 * lccrf_get_backward_route / lccrf_batch_get_backward_route (section 2c) report which route the last successful backward call of any
 * section took; NULL arguments return LCCRF_E_INVALID and write nothing.  Added WITHOUT a step of LCCRF_ABI_VERSION: probe by symbol.
 * Not covered by this option (notes/fused_backward.md): matrices, normalisation modes, d_grad_compat and d_grad_model -- section 1k's
 * LCCRF_OPT_FUSED_BACKWARD_LEARNT --, feature gradients -- section 1l's LCCRF_OPT_FUSED_BACKWARD_FEATURES --, frames of 2049 points
 * and more, the half-CU shapes; the route is not the default.
 *
 * 1k. ... and of a LEARNT model -- LCCRF_OPT_FUSED_BACKWARD_LEARNT (off by default; per handle or batch).
 *
 * The layers that learn the model (sections 1e, 1g, 2g, 2h) call the backward on handles and batches whose terms carry a matrix or a
 * normalisation mode, and ask for dL/dmu.  With this option set such a call runs the replay and the sweep in one kernel launch too
 * (csrc/fused_backward_general.hip: one 1024-lane workgroup per frame), when
 *   - no entry of d_grad_features is non-NULL;
 *   - some term has a matrix or a mode other than AFTER, or the call is in section 1e's form: d_grad_compat or d_grad_model is asked
 *     for, also on Potts terms (the derivative at mu = I).  A Potts / AFTER request for dL/dU and / or dL/dw alone is section 1j's and
 *     is governed by LCCRF_OPT_FUSED_BACKWARD only; LCCRF_OPT_FUSED_BACKWARD selects exactly what it selected before this option;
 *   - the frames are ones the plan takes, as in section 1j (two labels, one or two 2-D terms, at most 2048 active points, lattices
 *     inside one workgroup's LDS); when dL/dmu is asked for, also every term with a product buffer of its own in that plan (frames
 *     whose lattices are so large that the plan shares one buffer take the sweep).  A batch decides once, over its largest frame.
 * Everything else takes the route it takes with the option off.  n_iterations = 0 may take either route.
 *   - Bit for bit: d_grad_unary (zero rows included), d_grad_weights, d_grad_compat (exactly +0 for a frame of 0 points and at
 *     n_iterations = 0) and the Q left behind are those of the option off: the replay forms Q_t as the general step does; the sweep
 *     forms every product and sum of sections 1e / 1g in their order; dL/dmu's partials are added over the same chunks of
 *     ceil(n / chunks) rows in ascending row order, accumulated over the iterations and added over the chunks in order.
 *   - d_grad_model (section 2h): the same two launches of the sums over the frames behind the kernel -- three launches in all.
 *   - Memory: the area of sections 1e / 2h, nothing more.
 *   - Argument checks, LCCRF_E_STATE, LCCRF_E_NOMEM and "a rejected call leaves the object as it was": the route is chosen where
 *     section 1j's is.  lccrf_get_backward_route / lccrf_batch_get_backward_route report LCCRF_BACKWARD_FUSED.
 * Not covered: feature gradients (on Potts terms normalised AFTER they are section 1l's; with a matrix or dL/dmu, sections 1f / 2h,
 * they take the sweep), frames of 2049 points and more, the half-CU shapes, other label counts and dimensions, K > 2.
 *
 * 1l. ... and WITH feature gradients -- LCCRF_OPT_FUSED_BACKWARD_FEATURES (off by default; per handle or batch).
 *
 * The layers that learn the kernel bandwidths call lccrf_inference_backward_all with feature arrays on a Potts model; sections 1d / 2d
 * add two corner-dot launches per iteration and term and two width-1 filters per term to section 1c's sweep (203 launches at T = 5
 * with two 2-D terms).  With this option set such a call runs the replay and the sweep in one kernel launch
 * (csrc/fused_backward_features.hip: one 1024-lane workgroup per frame), when
 *   - at least one entry of d_grad_features is non-NULL (a NULL entry's term does no feature work, the other terms' bits do not
 *     change; a request without a feature array is section 1j's or 1k's and never this option's);
 *   - the call is not in section 1e's form: neither d_grad_compat nor d_grad_model, no matrix on the handle or batch --
 *     lccrf_inference_backward_features, lccrf_batch_inference_backward_features, and lccrf_inference_backward_all /
 *     lccrf_batch_inference_backward_all when they reduce to those, and section 2l's
 *     lccrf_batch_inference_backward_modes_converged on such a batch: every frame's workgroup then runs its own t_f iterations;
 *   - every term is a Potts term normalised AFTER the filter, and n_iterations >= 1 (at 0 the call takes the sweep's memset to +0);
 *   - the frames are ones the plan takes, as in section 1j.  A batch decides once, over its largest frame and lattices.
 * Everything else takes the route it takes with the option off; options 6 and 7 select exactly what they selected.
 *   - Bit for bit: d_grad_unary, d_grad_weights and the Q left behind are section 1j's; every d_grad_features[k] (rows at or beyond a
 *     frame's n_points written +0, a frame of 0 points all zeros) is that of the option off -- g_b and g_n keep one owner, the lane
 *     that owns the point, and section 1d's order of additions (t = T .. 1, slice side then splat side, the norm part last).
 *   - Memory: the area of sections 1d / 2d, nothing more.  The kernel initialises g_b and g_n itself.
 *   - Argument checks, LCCRF_E_STATE, LCCRF_E_NOMEM and "a rejected call leaves the object as it was": the route is chosen where
 *     section 1j's is.  lccrf_get_backward_route / lccrf_batch_get_backward_route report LCCRF_BACKWARD_FUSED.
 * Added WITHOUT a step of LCCRF_ABI_VERSION.  Not covered: feature gradients in the compat form, normalisation modes (the API refuses
 * feature gradients there), frames of 2049 points and more, the half-CU shapes.
 * ==================================================================================== */
typedef enum lccrf_backward_route {
    LCCRF_BACKWARD_NONE   = 0,   /* no backward call yet */
    LCCRF_BACKWARD_STREAM = 1,   /* section 1c's sweep on the streaming engine */
    LCCRF_BACKWARD_FUSED  = 2    /* one launch */
} lccrf_backward_route;
int  lccrf_get_backward_route(lccrf_handle h, int *route);

/* ======================================================================================
 * 1m. Feature gradients under EVERY normalisation mode -- section 1f's call without section 1g's refusal: the factors a mode puts
 *     in front of and behind the filter are functions of the norm, and the norm of the features; here they are differentiated too
 *     (lc-crf-slam_amd/autograd.py: mean_field_features, mean_field_learned, LearnedKernelCRF and LearnedCRF take `normalization`).
 *     Added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.  lccrf_inference_backward_features and
 *     lccrf_inference_backward_all are unchanged and keep refusing a handle with a term that is not AFTER.
 *
 * The gradients of lccrf_inference(h, n_iterations, -, relax) on the handle's current unary, terms, matrices and modes.  With section
 * 1g's a_k (the factor behind the filter) and b_k (the factor in front of it), each 1 where the mode has none, s = sqrtf(n) as the
 * handle stores it, and per iteration t = T .. 1 and term k
 *      x = b_k . Q_{t-1}                  rounded once: the forward's own splat input (Q_{t-1} itself without a pre factor)
 *      y = a_k . (mu_k^T gamma_t)         (a_k . gamma_t for a Potts term)
 *      z = Phi_k^T(y)                     the sliced result of the transposed filter, before it is multiplied by b_k
 * dL/dU, dL/dw_k, dL/dmu_k and G_{t-1} are section 1g's, and for every term with a feature array:
 *      filter part    g_b[k][i][c] += alpha_k w_k (<y_i, (B S x)[v_ic]> + <x_i, (B^T S y)[v_ic]>)
 *      post adjoint   g_post[k][i] += w_k <gamma_t,i, (mu_k Phi_k(x))_i>         = dL/da_k[i]; terms with a post factor only
 *      pre adjoint    g_pre[k][i]  += w_k <Q_{t-1},i, z_i>                       = dL/db_k[i]; terms with a pre factor only
 * every dot over the labels added in the order 0 .. L-1; within an iteration the post part is added before the pre part.  Then
 *      AFTER       g_n = g_post                               (a = n)
 *      BEFORE      g_n = g_pre                                (b = n)
 *      SYMMETRIC   g_n = (g_post + g_pre) * (0.5f / s[i])     (a = b = s, ds/dn = 1 / (2 s); both adjoints in ONE accumulator)
 *      NONE        no norm part: the filter part alone
 * and a_n = -n_k^2 . g_n (n_k the true norm, lccrf_get_norm's), g_b[k][i][c] += alpha_k (a_n,i (B S 1)[v_ic] + (B^T S a_n)[v_ic]) and the
 * map from dL/db to dL/df are section 1d's, unchanged.  At n_iterations = 0 dL/df is exactly 0.
 *
 * Arguments, checks (before anything is enqueued), errors (LCCRF_E_INVALID; LCCRF_E_STATE without unary energies; LCCRF_E_NOMEM),
 * stream and memory rules are lccrf_inference_backward_all's; a rejected call leaves the handle as it was.
 *   - Every term AFTER, or d_grad_features == NULL: the call IS lccrf_inference_backward_all -- the same bits in every output and
 *     the same route, the one-launch routes of sections 1j - 1l included.
 *   - A term that is not AFTER and at least one non-NULL entry of d_grad_features: the streaming sweep, whatever
 *     LCCRF_OPT_FUSED_BACKWARD* options are set (lccrf_get_backward_route: LCCRF_BACKWARD_STREAM).  d_grad_unary, d_grad_weights and
 *     d_grad_compat receive, bit for bit, what lccrf_inference_backward_all gives on the same handle with d_grad_features == NULL.
 *     A NULL entry of d_grad_features skips that term's feature work; the other outputs keep their bits.
 *   - Deterministic: no float atomics.  g_b keeps section 1d's owner and order (t = T .. 1, slice side, splat side, the norm part
 *     last); the one accumulator of g_post and g_pre is owned by its point: the same bits from run to run.
 *   - Handles in locality mode (8192 points and more) are re-built the plain way, as in section 1c; results in the caller's order.
 *   - Launches: those of section 1f.  The pre adjoint rides in the kernel that forms G_{t-1} (a row-wise form of it: not a launch
 *     more); the splat-side corner dot multiplies its row by b_k as it loads it; a NONE term saves the norm part's two width-1
 *     filters, two corner dots and one per-point kernel.
 *   - Memory: section 1f's area, not a byte more (g_n is the one accumulator), plus section 1g's factor arrays.                  */
int  lccrf_inference_backward_modes(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                    float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat);

/* ======================================================================================
 * 2. Batch API -- many independent frames in flight on one GPU.
 *    Every frame is one CRF of the object API; frames never interact.  Inputs may be
 *    handed over as host buffers (uploaded) or bound as DEVICE pointers (zero copy), so
 *    a caller that already holds the arrays in HBM pays no PCIe traffic.
 * ==================================================================================== */
typedef struct lccrf_batch *lccrf_batch_handle;

typedef struct lccrf_batch_desc {
    int   max_frames;                       /* frames per batch                          */
    int   max_points;                       /* per-frame stride of every array           */
    int   n_labels;
    int   n_kernels;
    int   feat_dims[LCCRF_MAX_KERNELS];
    float weights[LCCRF_MAX_KERNELS];
} lccrf_batch_desc;

int  lccrf_batch_create(lccrf_batch_handle *out, int device_id, const lccrf_batch_desc *desc);
void lccrf_batch_destroy(lccrf_batch_handle b);
/* lccrf_set_option for a batch (LCCRF_OPT_SINGLE_WORKGROUP: batches of up to 64 two-kernel frames take two workgroups per frame) */
int  lccrf_batch_set_option(lccrf_batch_handle b, int option, int value);
/* lccrf_set_multilabel_routes / lccrf_get_multilabel_routes for a batch (section 1: LCCRF_MULTILABEL_POTTS | LCCRF_MULTILABEL_LEARNT) */
int  lccrf_batch_set_multilabel_routes(lccrf_batch_handle b, unsigned routes);
int  lccrf_batch_get_multilabel_routes(lccrf_batch_handle b, unsigned *routes);

/* Host inputs (copied to the device).  n_points[f] <= max_points; arrays are strided by
 * max_points per frame.  Exactly one of unary / label must be non-NULL.                 */
int  lccrf_batch_set_inputs_host(lccrf_batch_handle b, int n_frames, const int32_t *n_points,
                                 const float *unary, const int16_t *label, const float *conf,
                                 const float *const *features /* [n_kernels] */);
/* Host inputs, nothing waits (round 5; the reference's per-frame cost at src/Tracking.cc:1919-1930 is host to host, so a replay
 * that wants the GPU's rate has to keep the link busy under the kernels).  Same arrays as lccrf_batch_set_inputs_host.  They are
 * copied into pinned staging owned by the batch before the call returns -- the caller's buffers may be reused at once -- and
 * uploaded on the batch's copy stream; whatever is queued on the batch afterwards (lccrf_batch_run / _build / ..., on its own or a
 * caller's stream) waits for the upload on the device, and the upload itself waits for the kernels queued before it.  With
 * LCCRF_HOST_PINNED the caller vouches that the label / unary and feature arrays are pinned (hipHostMalloc / hipHostRegister) and stay untouched until
 * lccrf_batch_wait_inputs returns (or any later result of this batch has been seen): no staging copy, the DMA reads the caller's
 * memory.  One batch is in flight per handle: to upload batch i+1 under batch i's kernels alternate between two or three handles
 * (tools/replay_multi.cpp does).                                                                       */
#define LCCRF_HOST_PINNED 1
int  lccrf_batch_set_inputs_host_async(lccrf_batch_handle b, int n_frames, const int32_t *n_points,
                                       const float *unary, const int16_t *label, const float *conf,
                                       const float *const *features /* [n_kernels] */, int flags);
int  lccrf_batch_wait_inputs(lccrf_batch_handle b);
/* Results to the host, nothing waits: queues, behind everything queued on the batch so far, copies of the chosen results into
 * pinned memory owned by the batch (label bits: 256 bytes per 2000-keypoint frame -- the layout of lccrf_batch_device_label_bits;
 * int16 labels and probabilities: the layouts of lccrf_batch_get_map_host / _get_probability_host) on the batch's download
 * stream.  lccrf_batch_wait_download waits for them -- and settles the per-frame fallback of a one-launch run first, refreshing
 * the copies if a frame had to be re-run -- and hands out the host pointers (NULL for what was not asked for), valid until the
 * next lccrf_batch_download_async on this handle.                                                                              */
#define LCCRF_DOWNLOAD_LABEL_BITS  1
#define LCCRF_DOWNLOAD_MAP         2
#define LCCRF_DOWNLOAD_PROBABILITY 4
int  lccrf_batch_download_async(lccrf_batch_handle b, int what);
int  lccrf_batch_wait_download(lccrf_batch_handle b, const uint64_t **label_bits, int *words_per_frame,
                               const int16_t **map, const float **probability);
/* Device inputs (bound, not copied; must stay valid until the batch finished).  d_n_points must be COMPLETE when
 * this is called (it is validated and clamped into a private copy on the batch's own stream right here, unordered
 * with any other stream); an entry outside [0, max_points] raises LCCRF_E_CAPACITY at the next synchronisation point. */
int  lccrf_batch_bind_inputs_device(lccrf_batch_handle b, int n_frames, const int32_t *d_n_points,
                                    const float *d_unary, const int16_t *d_label, const float *conf,
                                    const float *const *d_features /* host array of device ptrs */);

/* Per frame: every PottsPotential3D ctor (lattice + norm), pairwise3d.h:20-28.
 * Asynchronous on `stream` (a hipStream_t, or NULL for the batch's own stream).         */
int  lccrf_batch_build(lccrf_batch_handle b, void *stream);
/* Per frame: DenseCRF::inference(n_iterations, with_map, relax), densecrf_base.h:65-73. */
int  lccrf_batch_inference(lccrf_batch_handle b, int n_iterations, int with_map, float relax,
                           void *stream);
/* Per frame, in ONE kernel launch: every PottsPotential3D ctor (lattice + norm, pairwise3d.h:20-28) followed by
 * DenseCRF::inference(n_iterations, with_map, relax) (densecrf_base.h:65-73) -- the reference's whole per-frame
 * sequence src/Tracking.cc:1920-1929.  Needs inputs only (no lccrf_batch_build); the lattices never reach
 * HBM, so the parity probes (norm, lattice arrays) rebuild them on demand.  Frames the one-launch kernel
 * cannot take (n_labels != 2, a kernel with d != 2, more than two kernels, > 4096 points, or lattices too
 * large for one workgroup's LDS) run on the build + inference kernels instead: same results either way.  The
 * decision is PER FRAME: the kernel flags the frames whose lattices did not fit and, at the next synchronisation
 * point (lccrf_batch_synchronize, any getter, the next call that continues from the results), exactly those frames
 * are gathered, re-run on the two-kernel path and scattered back -- a batch with one outlier pays for one frame.
 * The device buffers of lccrf_batch_device_buffers / _label_bits are complete behind that synchronisation point.
 * Memory: the first lccrf_batch_run of a handle whose frames qualify for the two-frames-per-CU kernel (>= 256 frames, two 2-D kernels,
 * <= 2048 points) allocates that kernel's per-point record area ON THAT CALL (a synchronous hipMalloc): 96 KB per frame BOUND at that
 * moment (1.6 GB for 16384 frames, 400 MB for 4096), kept until lccrf_batch_destroy; a later run with more frames allocates a larger
 * area (the smaller one stays with the handle).  Expect the first run of a handle to be slower than the following ones.  */
int  lccrf_batch_run(lccrf_batch_handle b, int n_iterations, int with_map, float relax, void *stream);
/* How many frames of the last lccrf_batch_run had to be re-run on the two-kernel path (0 = every frame fitted). */
int  lccrf_batch_get_fallback_frames(lccrf_batch_handle b, int *n_frames);
int  lccrf_batch_synchronize(lccrf_batch_handle b);

/* Results: copy to host, or borrow the device buffers ([n_frames][max_points](xL)).     */
int  lccrf_batch_get_map_host(lccrf_batch_handle b, int16_t *map_out);
int  lccrf_batch_get_probability_host(lccrf_batch_handle b, float *prob_out);
int  lccrf_batch_get_lattice_sizes_host(lccrf_batch_handle b, int kernel, int32_t *n_vertices_out);
int  lccrf_batch_get_norm_host(lccrf_batch_handle b, int kernel, float *norm_out);
int  lccrf_batch_device_buffers(lccrf_batch_handle b, const int16_t **d_map, const float **d_prob);
/* Binary CRFs (n_labels == 2, the SLAM configuration src/Tracking.cc:1919): the MAP labels of the last
 * inference with_map as one BIT per point -- uint64 [n_frames][words_per_frame], point i = bit i%64 of
 * word i/64, bits beyond a frame's n_points are 0.  Written by the same kernel that writes the int16
 * labels; this is the payload of the multi-GPU label gather (250 bytes per
 * 2000-keypoint frame instead of 4000; RCCL has no 16-bit integer type).                          */
int  lccrf_batch_device_label_bits(lccrf_batch_handle b, const uint64_t **d_bits, int *words_per_frame);

/* Engine selection for the inference loop (all give bit-identical results):
 *   0 = automatic, 1 = streaming kernels over HBM (any size), 2 = fused one-workgroup-
 *   per-frame kernel with the lattice values in LDS (SLAM sizes only).  lccrf_batch_get_engine
 *   also reports 3 = the one-launch-per-frame kernel of lccrf_batch_run, and 4 = the fused
 *   engine's kernels for terms with a label-compatibility matrix or a normalisation mode
 *   (section 2g: one 1024-lane workgroup per frame, fixed count or until converged), and
 *   5 = its kernel for frames of three to eight labels (LCCRF_OPT_FUSED_MULTILABEL), which
 *   engine 2 ("fused or fail") accepts for such a batch when the option is on and the plan fits,
 *   and 6 = that kernel's form for terms with a matrix or a mode (LCCRF_MULTILABEL_LEARNT), under
 *   the same rule.                                                                              */
int  lccrf_batch_set_engine(lccrf_batch_handle b, int engine);
int  lccrf_batch_get_engine(lccrf_batch_handle b, int *engine_in_use);
/* Report only: the workgroup shape of the last one-workgroup-per-frame launch -- lccrf_batch_inference on the fused engine (engine 2),
 * lccrf_batch_run's one-launch kernel (engine 3) or section 2g's kernels (engine 4: always 1024 and 1), whichever ran last -- as
 * lanes per frame (1024 or 512) and how many frames share a CU (1; 2 for the half-LDS plans: batches of at least 256 frames of up to
 * 2048 points, csrc/fused_lean.h and csrc/frame_lean.hip).  LCCRF_OPT_FUSED_MULTILABEL's and LCCRF_MULTILABEL_LEARNT's kernels (engines 5 and 6) report 1024 and, in the second
 * value, their POINTS PER LANE (1 or 2; a frame per CU always).  0 / 0 if no such launch happened yet.  Same results in every shape (the order of every row sum is the
 * reference's, permutohedral_cpu.h:653-661).                                                                                   */
int  lccrf_batch_get_fused_shape(lccrf_batch_handle b, int *lanes_per_frame, int *frames_per_cu);
/* Report only: how the lattices now in HBM were built (after lccrf_batch_build) -- whether the points of a frame are processed in
 * an internal order (locality mode: frames of >= 8192 points) and whether the vertices were found by the SORTED build
 * (LCCRF_OPT_VERTEX_ORDER) or, 0, by the hash table: also what an engine falls back to for good when a frame's vertex codes overflow
 * 62 bits or a feature is wide enough to wrap the reference's int16 keys.  Either pointer may be NULL.                           */
int  lccrf_batch_get_locality_mode(lccrf_batch_handle b, int *internal_point_order, int *sorted_build);
/* Report only: how the two-label mean-field step splats term `kernel` for the lattices now in HBM and the frames now bound (after
 * lccrf_batch_build; on a handle, after lccrf_inference or whatever else built its lattices).  With the sorted build the splat takes
 * the first blur passes along: `passes` of them (0: none), and from two passes on it works on an overlapped window of `window`
 * vertices in LDS (256, 512 or 1024) of which `halo` on either side are recomputed by the neighbouring workgroups, launched as
 * workgroups of `lanes` lanes with `vertices_per_lane` vertices each (window = lanes * vertices_per_lane; all three 0 without a
 * window).  long_mode: 0, or 1 / 2 for a coarse kernel, whose long rows get the row-walking splat and no pass.  Same results in
 * every plan.                                                                                                                    */
typedef struct lccrf_splat_plan {
    int32_t passes, halo, window, lanes, vertices_per_lane, long_mode;
} lccrf_splat_plan;
int  lccrf_batch_get_splat_plan(lccrf_batch_handle b, int kernel, lccrf_splat_plan *out);
int  lccrf_get_splat_plan(lccrf_handle h, int kernel, lccrf_splat_plan *out);
/* Report only, under the same conditions: which way each of the d + 1 blur passes of term `kernel` goes in the two-label mean-field
 * step (Potts terms normalised after the filter), as counts of passes per route -- in_splat (taken along by the splat, = the splat
 * plan's `passes`), paired_table / paired_plain (two passes per launch, off the two-hop neighbour table or without one; always
 * even), alone_32bit / alone_compact (a launch per pass, on the 32-bit neighbour ids or the compact 16-bit table of the sorted
 * build) and in_slice (the last pass, inside the slice: 0 or 1).  The six add up to d + 1.  nontemporal: the alone_32bit passes
 * load their table non-temporally (0 when there is none).  first_table_pair: index in the two-hop table of the first pair read
 * from it, -1 when no pass is.  Same results on every route.                                                                  */
typedef struct lccrf_blur_plan {
    int32_t in_splat, paired_table, paired_plain, alone_32bit, alone_compact, in_slice, nontemporal, first_table_pair;
} lccrf_blur_plan;
int  lccrf_batch_get_blur_plan(lccrf_batch_handle b, int kernel, lccrf_blur_plan *out);
int  lccrf_get_blur_plan(lccrf_handle h, int kernel, lccrf_blur_plan *out);
/* Report only, under the same conditions: what the build kernels themselves counted while they built the lattice of term `kernel`,
 * frame `frame`, now in HBM (csrc/stream_build.hip; tests/sorted_build_cases.py places a frame on either side of every rule).  All 0
 * for lattices of the one-workgroup build.  sorted_build: built by sorting the entries on their vertex's row-major code (else by the
 * hash table, and the next nine fields are 0).  direct_codes: the code is its own sort bucket (the box of the vertices is no larger
 * than the histogram).  long_buckets: sort buckets of more than 512 entries, each ordered by a workgroup of its own -- by the LDS
 * bitmap over the original ids (long_by_bitmap: one code, >= 1024 entries, ids spanning at most 15872 words), or by the bitonic
 * network because it holds one code but fewer than 1024 entries (long_by_network_uniform), several codes (long_by_network_mixed) or
 * one code whose ids span more than the bitmap (long_by_network_wide); the four add up to long_buckets.  max_buckets_per_workgroup:
 * the most long buckets one workgroup ordered (more than 1 beyond 64 long buckets).  phantom_entries: entries of the points that pad
 * the frame to a multiple of four; empty_row_vertices: vertices only they touch.  long_rows: hash build only, rows of more than 128
 * entries (ordered by a workgroup each).  Per frame rather than per term, locality mode only: point_buckets_over_64, the buckets of
 * the point sort that kept their arrival order, and largest_point_bucket.  The handle's form reports its one frame.  Added WITHOUT a
 * step of LCCRF_ABI_VERSION: probe by symbol.                                                                                     */
typedef struct lccrf_build_report {
    int32_t sorted_build, direct_codes, long_buckets, long_by_bitmap, long_by_network_uniform, long_by_network_mixed,
            long_by_network_wide, max_buckets_per_workgroup, phantom_entries, empty_row_vertices, long_rows,
            point_buckets_over_64, largest_point_bucket;
} lccrf_build_report;
int  lccrf_batch_get_build_report(lccrf_batch_handle b, int kernel, int frame, lccrf_build_report *out);
int  lccrf_get_build_report(lccrf_handle h, int kernel, lccrf_build_report *out);
/* Parity probe (as lccrf_get_lattice, which re-builds a lattice of locality mode the plain way before it answers): the tables of term
 * `kernel`, frame `frame` AS BUILT, in the internal order the engine iterates in, copied out without a rebuild.  With Np = the
 * frame's points rounded up to a multiple of four, N its real points and V its vertices: n_points_padded = Np, n_vertices = V,
 * perm [Np] (position -> original point; the identity outside locality mode), offset / bary [Np][d+1] by POSITION, rowptr [V+1],
 * csr_pt (positions) / csr_w [N (d+1)], nbr [d+1][V][2], fastn [V] (1: vertex v + 1 is v's axis-0 neighbour) with *has_fastn = 0 and
 * fastn untouched where the build keeps no such table.  Any output pointer may be NULL: ask for the two sizes first.  Added WITHOUT
 * a step of LCCRF_ABI_VERSION: probe by symbol.                                                                                    */
int  lccrf_batch_get_built_lattice(lccrf_batch_handle b, int kernel, int frame, int32_t *n_points_padded, int32_t *n_vertices,
                                   int32_t *perm_out, int32_t *offset_out, float *bary_out, int32_t *rowptr_out, int32_t *csr_pt_out,
                                   float *csr_w_out, int32_t *nbr_out, uint8_t *fastn_out, int *has_fastn);

/* Measurement support for bench.py: HIP-event time of the last lccrf_batch_inference()
 * on its stream, the number of launches of the dominant kernel and their summed
 * duration as seen by events around them (0 if not instrumented).                       */
/* The batch's own stream (a hipStream_t; what `stream = NULL` means in the calls above), for a caller that orders its own work -- a
 * collective on the label bits, a copy -- behind the batch's kernels.  Several batches kept in flight overlap best on their OWN
 * streams: each was created with its handle, one after the other, and HIP spreads streams over its (four) hardware queues in that
 * order, whereas two caller-made streams may share a queue and then run their kernels one after the other (measured: bench.py with two
 * handles, 5.04e7 iterations/s on the handles' streams, 4.7-5.0e7 on two torch streams depending on what else the process created). */
int  lccrf_batch_get_stream(lccrf_batch_handle b, void **stream);
int  lccrf_batch_last_timing(lccrf_batch_handle b, float *inference_ms, float *build_ms);
/* Batches of >= 256 two-kernel frames of 513 .. 2048 points run their inference two frames per CU from PREPARED launch records: what
 * the kernel's prologue would derive from the lattices in every launch (the ranking and placement of the appearance kernel's rows,
 * every point's vertex addresses and product slots, the row and neighbour tables in their on-chip form) is written once, by the
 * FIRST lccrf_batch_inference behind a build, into one block per frame (<= 64 KB; allocated on that call, kept with the handle), and
 * every later inference on those lattices starts from it.  It is part of the lattice construction (the PottsPotential3D ctor,
 * pairwise3d.h:20-28), not of inference(): prepare_ms = HIP-event time of the last such launch (0 if none), runs = how many there
 * were on this handle.  Results are identical with and without the records.
 * When the batch's unaries come from labels (label + conf), those later inferences also read the points' labels as one byte per point
 * (0, 1, or 2 for unknown / out of range) instead of the unary array: the library's own copy, max_frames x max_points bytes, written
 * with the unary array and allocated by the first inference on labels.  The caller's label array is not read again for it.       */
int  lccrf_batch_last_prepare(lccrf_batch_handle b, float *prepare_ms, int *runs);
/* Measurement support: average HIP-event duration of `reps` launches of the streaming engine's dominant kernel (one
 * Jacobi blur pass of `kernel` over every frame of the batch, permutohedral_cpu.h:663-679) and the number of lattice
 * vertices one launch processes.  Needs lccrf_batch_build; leaves the CRF state (Q, labels) untouched.            */
int  lccrf_batch_time_blur_pass(lccrf_batch_handle b, int kernel, int reps, float *ms_per_launch,
                                int64_t *vertices_per_launch);

/* ======================================================================================
 * 2c. Gradients of a batch's inference -- section 1c for every frame of a batch at once: one reverse sweep over the F frames, in
 *     the number of launches section 1c takes for one frame.  The formulas are section 1c's, per frame; the weights w_k are the
 *     batch's (lccrf_batch_desc.weights, shared by every frame), and so are the parameters fitted.
 * ==================================================================================== */
/* lccrf_set_pairwise_weight for a batch: the weight of term `kernel` in every frame.  The lattices, norms and prepared launch records'
 * lattice part stay; everything derived from w (the fused engines' w*norm products, the prepared launch records) is invalidated, and
 * the next lccrf_batch_inference / _run equals, bit for bit, that of a batch created with weight w.  A pending one-launch run is
 * settled first (its fallback frames re-run with the old weight).                                                               */
int  lccrf_batch_set_pairwise_weight(lccrf_batch_handle b, int kernel, float w);
/* Replaces the unary energies of the n_frames frames now bound: d_unary [n_frames][max_points][L], device memory (checked as in
 * section 1b), COPIED into the batch's own array on the batch's stream -- the caller's array may be freed behind that copy.  Labels
 * the inputs came from are forgotten; lattices, norms and prepared launch records stay.  LCCRF_E_STATE before inputs are set.      */
int  lccrf_batch_set_unary_device(lccrf_batch_handle b, const float *d_unary);
/* Gradients of lccrf_batch_inference(b, n_iterations, -, relax, -) on the batch's current inputs and weights, per frame:
 * d_grad_prob [n_frames][max_points][L] = dL/dQ_T, d_grad_unary [n_frames][max_points][L] (overwritten), d_grad_weights
 * [n_frames][n_kernels] (overwritten; may be NULL).  Device arrays, checked as in section 1b against n_frames * max_points * L
 * (n_frames * n_kernels) floats.
 *   - Per frame, the bits of section 1c: d_grad_unary[f] and d_grad_weights[f][:] are exactly what lccrf_inference_backward returns
 *     for a handle holding frame f's n_points[f] points, unary and features and the batch's weights (the weight gradient is reduced
 *     over the same T x B partials in the same order, B = backward_blocks of n_points[f] as section 1c counts them).  Rows at or
 *     beyond n_points[f] of d_grad_unary are written 0; a frame of 0 points gets zero gradients.
 *   - Self-contained, as section 1c: the forward is replayed on the step path, keeping Q_0 .. Q_{T-1} of every frame (one copy of
 *     the whole [n_frames][max_points][L] array per iteration).  Afterwards the batch's Q (lccrf_batch_device_buffers,
 *     lccrf_batch_get_probability_host) holds exactly what lccrf_batch_inference(b, n_iterations, 0, relax, stream) would have left;
 *     the labels are untouched.
 *   - Needs lccrf_batch_build or lccrf_batch_run on the current inputs (LCCRF_E_STATE otherwise); a pending one-launch run is
 *     settled first (its fallback frames included), and lattices the one-launch kernel kept on chip are built in HBM.  Frames in
 *     locality mode (>= 8192 points) are handled as section 1c handles them: the lattices are re-built the plain way for this call
 *     (the next lccrf_batch_build / _run decides afresh); results are in the caller's point order.
 *   - Deterministic: no float atomics; the same bits from run to run.
 *   - Streams: `stream` is a hipStream_t or NULL, as for lccrf_batch_inference; no host synchronisation beyond the one-time learning
 *     of new lattices' sizes every entry point does.  lccrf_batch_last_timing's inference_ms then times this call.
 *   - Memory: a batch-owned HBM area of 4 * (F*S*(T + K + 1) + max(T,1)*K*F*B) bytes, F = n_frames, S = max_points * L,
 *     B = backward_blocks(max_points, L) as section 1c counts them (16384 frames of max_points = 2000, L = 2, K = 2, T = 5: 2.1 GB).
 *     Zeroed when allocated, grown by the first call that needs more, freed by lccrf_batch_destroy; a failed allocation returns
 *     LCCRF_E_NOMEM and leaves the batch usable.  lccrf_batch_inference / _run never allocate it.
 *   - Errors: LCCRF_E_INVALID for n_iterations < 0, a relax that is not finite, or a device array section 1b refuses; a rejected
 *     call leaves the batch's inputs, lattices and Q as they were.  K = 0 is legal (d_grad_weights then receives nothing).
 *   - Potts terms normalised AFTER only: on a batch with a label-compatibility matrix or a mode other than AFTER (section 2g) this call
 *     and section 2d's return LCCRF_E_STATE and leave the batch as it was.  The gradients of such a batch -- of a learnt model, every
 *     frame with the bits of a handle's section 1e and 1g gradients -- are lccrf_batch_inference_backward_all's (section 2h).       */
int  lccrf_batch_inference_backward(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                    float *d_grad_weights, void *stream);
/* Section 1j's report for a batch: the route of its last successful backward call (an lccrf_backward_route). */
int  lccrf_batch_get_backward_route(lccrf_batch_handle b, int *route);

/* ======================================================================================
 * 2d. Section 1d for every frame of a batch at once, in the launches section 1d takes for one frame.  d_grad_features: host array of
 *     n_kernels device pointers, d_grad_features[k] [n_frames][max_points][d_k], overwritten (rows at or beyond a frame's n_points
 *     are written 0; a frame of 0 points gets zeros); entries, or the array, may be NULL as in section 1d, and so may d_grad_unary
 *     and d_grad_weights.  Per frame, the bits of section 1d for a handle holding that frame -- for dL/df as for dL/dU and dL/dw --
 *     and everything else is section 2c's contract (streams, state, errors, what is needed beforehand).  The feature arrays the
 *     batch was given (lccrf_batch_bind_inputs_device: the caller's own) are read again by this call.
 *     Memory: section 2c's area plus 4 * F * sum over the terms asked for of P4 * (d_k + 2) bytes, P4 = max_points rounded up to
 *     a multiple of 4 (plus 4 * F * max_points * L when d_grad_unary is NULL).  Added without a step of LCCRF_ABI_VERSION.
 *     In ONE launch under LCCRF_OPT_FUSED_BACKWARD_FEATURES (section 1l): the same bits, decided once for the batch.               */
int  lccrf_batch_inference_backward_features(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob,
                                             float *d_grad_unary, float *d_grad_weights, float *const *d_grad_features, void *stream);

/* ======================================================================================
 * 2e. Section 1h for every frame of a batch: each frame stops on its own.  On built lattices (behind lccrf_batch_build),
 * asynchronous on `stream` (NULL: the batch's own) like lccrf_batch_inference.  Batches the fused plan takes (two labels, one or
 * two 2-D terms, up to 4096 points per frame, lattices that fit one workgroup's LDS) run in ONE launch, one frame per workgroup: a
 * workgroup whose frame has converged stores its results and leaves its CU to the next frame; lccrf_batch_get_engine reports 2.
 * Every other batch runs the streaming step for all frames until the last frame has finished (one word read by the host and one
 * synchronisation of the call's stream per iteration): a finished frame's Q is kept aside at the iteration it finished and put
 * back before the labels are formed -- stepping it further is wasted work, not a different result.  lccrf_batch_get_engine
 * reports 1.  A batch whose terms carry a matrix or a mode (section 2g) runs in ONE launch as well where lccrf_batch_inference does
 * (engine 4: up to 2048 points per frame), on csrc/fused_general_converge.hip; lccrf_batch_get_engine reports 4.
 * LCCRF_E_STATE before lccrf_batch_build; the argument checks of section 1h.
 * ==================================================================================== */
int  lccrf_batch_inference_converged(lccrf_batch_handle b, int max_iterations, int criterion, float tol, int with_map, float relax,
                                     void *stream);
/* Per frame of the batch, [n_frames] each, any pointer may be NULL: t, d_t, c_t and whether the criterion was met (a FOURTH array
 * rather than a bit: 1 also when the criterion was met exactly at the cap, which `iterations < max_iterations` cannot tell).
 * Waits for THIS batch's stream only (as lccrf_batch_synchronize), not for the device.  LCCRF_E_STATE when no converged inference
 * has run on the current inputs.                                                                                                  */
int  lccrf_batch_get_convergence_host(lccrf_batch_handle b, int32_t *iterations, float *delta, int32_t *changed, int32_t *converged);
/* The same four arrays in the batch's HBM ([max_frames] each, owned by the batch, allocated when it is created), for a caller that
 * stays on the device: valid behind the converged call in stream order.  Any pointer may be NULL.                                 */
int  lccrf_batch_device_convergence(lccrf_batch_handle b, const int32_t **d_iterations, const float **d_delta,
                                    const int32_t **d_changed, const int32_t **d_converged);

/* ======================================================================================
 * 2f. Section 1i for every frame of a batch: lccrf_batch_run with section 2e's stop rule.  Needs inputs only; asynchronous on
 * `stream` (NULL: the batch's own).  Per frame Q, labels, label bits and the report are bit for bit what lccrf_batch_build followed
 * by lccrf_batch_inference_converged leaves; every frame stops on its own.  Batches lccrf_batch_run takes in one launch run one
 * 1024-lane workgroup per frame (csrc/frame_converge.hip), lccrf_batch_get_engine reports 3; frames the kernel cannot take are
 * decided per frame at the next synchronisation point, re-run there with lccrf_batch_inference_converged's engines and counted by
 * lccrf_batch_get_fallback_frames, as for lccrf_batch_run.  The getters of section 2e settle a pending run first
 * (lccrf_batch_device_convergence: the arrays are complete behind lccrf_batch_synchronize).  Every other batch builds its lattices
 * and takes lccrf_batch_inference_converged (a batch with a matrix or a mode: section 2g, LCCRF_OPT_FRAME_GENERAL).  The argument checks of section 1h.  Added without a step of LCCRF_ABI_VERSION.
 * ==================================================================================== */
int  lccrf_batch_run_converged(lccrf_batch_handle b, int max_iterations, int criterion, float tol, int with_map, float relax,
                               void *stream);

/* ======================================================================================
 * 2g. Label-compatibility matrices and normalisation modes of a batch -- sections 1e and 1g for every frame at once.  A learnt model
 * (lc-crf-slam_amd/autograd.py: CompatMeanFieldCRF, LearnedCRF) is term weights, a matrix per term and a mode per term; it is global,
 * so a batch holds ONE matrix and ONE mode per term, shared by every frame.  Meaning, arithmetic, argument checks and error codes are
 * those of the handle's setters: finite entries, `kernel` a term of the batch, a mode in 0 .. 3, else LCCRF_E_INVALID (a mode outside
 * 0 .. 3, a kernel index outside 0 .. LCCRF_MAX_KERNELS - 1 and a NULL `mode` are refused before the batch is looked at).  Added
 * WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for these four by symbol.
 *
 * A setter changes no lattice and no norm; it may be called before or after lccrf_batch_build and between inferences, and a pending
 * one-launch run is settled before it takes effect (as lccrf_batch_set_pairwise_weight does).  It does not touch the prepared
 * launch records (lccrf_batch_last_prepare): those belong to the Potts, normalised-AFTER path, and a batch with a matrix or a mode
 * neither reads, writes nor invalidates them.  Taking the last matrix and mode back returns the batch to the fast engines and to the
 * bits it returned before.  A batch from lccrf_batch_create has no matrix and every term AFTER.
 *
 * Engines.  Per frame, Q, the labels and the label bits are bit for bit those of a handle holding that frame with the same settings.
 *   - lccrf_batch_inference: two labels, one or two 2-D terms, up to 2048 points per frame (the largest n_points the host knows,
 *     else max_points) and lattices that fit the fused engine's plan run in ONE launch, one 1024-lane workgroup per frame, on the
 *     kernel a handle takes (csrc/fused_general.hip).  lccrf_batch_get_engine reports 4, lccrf_batch_get_fused_shape 1024 / 1.
 *   - lccrf_batch_inference_converged (section 2e's contract, unchanged: every frame stops on its own): the same batches in ONE launch
 *     on csrc/fused_general_converge.hip -- that kernel's loop with the stop decision inside; engine 4.  A batch created with
 *     max_frames = 1 takes it too; a handle does not (section 1h).
 *   - Every other batch -- 2049 points and more, other label counts or dimensions, three terms and more, lattices beyond one
 *     workgroup's LDS, lccrf_batch_set_engine(1) -- runs the streaming engine's general L-label step for all frames (engine 1), the
 *     converged call with section 2e's bookkeeping behind each step.
 *   - lccrf_batch_run and lccrf_batch_run_converged on such a batch are lccrf_batch_build followed by the inference call: the
 *     one-launch build + inference kernels hard-wire Potts.  lccrf_batch_get_fallback_frames reads 0.  With LCCRF_OPT_FRAME_GENERAL
 *     set, batches of frames of up to 2048 points take the one-launch kernels for such terms instead (csrc/frame_general.hip): engine
 *     3, shape 1024 / 1, the same bits; frames that do not fit are re-run with the same model and counted.
 * Gradients: lccrf_batch_inference_backward_all (section 2h; one launch under LCCRF_OPT_FUSED_BACKWARD_LEARNT, section 1k), behind
 * the batched torch layer BatchCompatMeanFieldCRF;
 * lccrf_batch_inference_backward and lccrf_batch_inference_backward_features still return LCCRF_E_STATE on such a batch and leave it
 * as it was (section 2c).  Not covered: the half-CU shapes (512 lanes, two frames per CU) and 3 - 4 points per lane; prepared launch
 * records for such batches; the handle's converged call.
 * ==================================================================================== */
/* compat: HOST [L][L], row-major as in section 1e, copied during the call and uploaded on the batch's stream; NULL removes the matrix. */
int  lccrf_batch_set_pairwise_compatibility(lccrf_batch_handle b, int kernel, const float *compat);
/* *is_set = 1 if term `kernel` has a matrix, else 0; compat_out (HOST [L][L], may be NULL) receives it -- the identity for a Potts
 * term.  No device work.                                                                                                        */
int  lccrf_batch_get_pairwise_compatibility(lccrf_batch_handle b, int kernel, float *compat_out, int *is_set);
/* mode: an lccrf_normalization (section 1g).                                                                                     */
int  lccrf_batch_set_pairwise_normalization(lccrf_batch_handle b, int kernel, int mode);
/* *mode = the lccrf_normalization of term `kernel`.  No device work.                                                             */
int  lccrf_batch_get_pairwise_normalization(lccrf_batch_handle b, int kernel, int *mode);

/* ======================================================================================
 * 2h. Gradients of a batch's inference for learnt models -- section 1f for every frame of a batch at once, Potts or with matrices
 *     (section 2g), under any normalisation mode, and the sums over the frames a trainer of the (global) model wants
 *     (lc-crf-slam_amd/autograd.py: mean_field_batch_compat, BatchCompatMeanFieldCRF).  Added WITHOUT a step of LCCRF_ABI_VERSION
 *     (it stays 3): probe for it by symbol.  Sections 2c and 2d are unchanged and keep refusing a batch with a matrix or a mode.
 *
 * The gradients of lccrf_batch_inference(b, n_iterations, -, relax, -) on the batch's current inputs, weights, matrices and modes.
 * d_grad_prob [n_frames][max_points][L] = dL/dQ_T.  Outputs, device arrays, each overwritten, each may be NULL:
 *      d_grad_unary     [n_frames][max_points][L]
 *      d_grad_weights   [n_frames][n_kernels]
 *      d_grad_features  HOST array of n_kernels device pointers, [n_frames][max_points][d_k] each; entries may be NULL (section 2d)
 *      d_grad_compat    [n_frames][n_kernels][L][L]      dL/dmu_k of every frame; for a term without a matrix the derivative at mu_k = I
 *      d_grad_model     [n_kernels + n_kernels*L*L]      sum over the frames of dL/dw, then of dL/dmu
 *   - Per frame, the bits of section 1f: d_grad_unary[f], d_grad_weights[f], d_grad_features[k][f] and d_grad_compat[f] are exactly
 *     what lccrf_inference_backward_all returns for a handle holding frame f's n_points[f] points, unary and features with the batch's
 *     weights, matrices and modes -- dL/dmu included: a frame's points are cut into C_f = min(max(ceil(n_points[f] / 256), 1), 128)
 *     chunks, the count section 1e gives a handle of that many points, whatever max_points is, and the C_f partials are summed in
 *     order.  Rows at or beyond n_points[f] are written 0; a frame of 0 points gets zeros.  At n_iterations = 0 dL/dmu and dL/df are
 *     exactly 0.  On a batch without matrices or modes and with d_grad_compat == d_grad_model == NULL every output is, bit for bit,
 *     lccrf_batch_inference_backward_features's.
 *   - d_grad_model[j] = ((x[0][j] + x[1][j]) + ...) + x[n_frames-1][j] in fp32, the frames in ascending order, x the per-frame values
 *     of this call: the caller's d_grad_weights / d_grad_compat, or the batch's area where the caller passed NULL.  One owner per
 *     entry, no float atomics; frames beyond n_frames are never read.  The order is part of the contract: a host loop of fp32 adds
 *     over the per-frame arrays gives the same bits.
 *   - With d_grad_features non-NULL and a term that is not normalised AFTER the call returns LCCRF_E_STATE and leaves the batch as it
 *     was, as section 1f's handle call does (section 1g: the norm's factors are not differentiated in the features).
 *   - Everything else is section 2c's contract: self-contained (the forward is replayed on the step path), LCCRF_E_STATE before
 *     lccrf_batch_build or lccrf_batch_run on the current inputs, a pending one-launch run settled first, frames in locality mode
 *     re-built the plain way, the stream rules, argument checks (LCCRF_E_INVALID) before anything is enqueued, Q afterwards exactly
 *     what lccrf_batch_inference(b, n_iterations, 0, relax, stream) leaves, the labels untouched, lccrf_batch_last_timing's
 *     inference_ms timing the call, deterministic.
 *   - Launches: those of section 1f for one frame (per iteration and term one kernel more than section 2c with matrices in play or
 *     d_grad_compat / d_grad_model asked for, one reduction at the end), plus two for d_grad_model (K > 0).
 *     Under LCCRF_OPT_FUSED_BACKWARD_LEARNT (section 1k), without feature arrays and on two-label frames of up to 2048 points: ONE
 *     launch for all frames, plus the two for d_grad_model, the same bits.
 *   - Memory: section 2c's area (with section 2d's part for the terms asked for) grows, with a matrix set or d_grad_compat /
 *     d_grad_model given, by 4 * (F*S + K*F*C*L*L) bytes -- gamma_t and the partials of dL/dmu, F = n_frames, S = max_points * L,
 *     C = min(max(ceil(max_points / 256), 1), 128) -- plus 4 * F*S when d_grad_unary is NULL, and with d_grad_model by 4 * F*K bytes
 *     when d_grad_weights is NULL and 4 * F*K*L*L bytes when d_grad_compat is NULL:
 *         4 * (F*S*(T + K + 2) + max(T,1)*K*F*B + K*F*C*L*L) bytes  [+ 4 * F*S] [+ 4 * F*K] [+ 4 * F*K*L*L]
 *     (16384 frames of max_points = 2000, L = 2, K = 2, T = 5: 2.4 GB, 4.2 MB of it the partials of dL/dmu).  Allocated as section 2c's; a failed
 *     allocation returns LCCRF_E_NOMEM and leaves the batch usable.
 * ==================================================================================== */
int  lccrf_batch_inference_backward_all(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob,
                                        float *d_grad_unary, float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat,
                                        float *d_grad_model, void *stream);

/* ======================================================================================
 * 2i. Section 1m for every frame of a batch at once: section 2h's call without its refusal of feature gradients on a batch with a
 *     term that is not normalised AFTER.  Added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.
 *     lccrf_batch_inference_backward_features and lccrf_batch_inference_backward_all are unchanged and keep refusing.
 *
 * Arguments, outputs, checks, errors, stream rules, timing and memory are lccrf_batch_inference_backward_all's.
 *   - Every term AFTER, or d_grad_features == NULL: the call IS lccrf_batch_inference_backward_all (same bits, same route).
 *   - Otherwise the streaming sweep of section 1m over all frames (lccrf_batch_get_backward_route: LCCRF_BACKWARD_STREAM under every
 *     option): every frame's d_grad_unary[f], d_grad_weights[f], d_grad_features[k][f] and d_grad_compat[f] are, bit for bit, what
 *     lccrf_inference_backward_modes returns for a handle holding frame f; rows at or beyond n_points[f] are written 0, a frame of 0
 *     points gets zeros; d_grad_model is section 2h's sum, with section 2h's bits.
 *   - Launches and memory: those of section 2h with feature arrays, as section 1m's are those of section 1f.
 * ==================================================================================== */
int  lccrf_batch_inference_backward_modes(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob,
                                          float *d_grad_unary, float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat,
                                          float *d_grad_model, void *stream);

/* ======================================================================================
 * 2j. Gradients of a batch's CONVERGED inference -- section 2c with one iteration count per frame: what section 1h's recipe
 *     ("lccrf_inference_backward(h, t, relax, ...) with the reported `iterations` is the gradient of the converged result") is for a
 *     handle, for every frame of a batch at once, each frame at its own count.  Added WITHOUT a step of LCCRF_ABI_VERSION (it stays
 *     3): probe for it by symbol.
 *
 * d_iterations: device array of [n_frames] int32 (checked as section 1b checks device arrays; NULL: LCCRF_E_INVALID), read in stream
 * order and never by the host: the array lccrf_batch_device_convergence hands out can be passed straight in, behind a converged call
 * queued on the same stream, with no host synchronisation in between.  Frame f is differentiated at
 *     t_f = min(max(d_iterations[f], 0), max_iterations)            (the kernels clamp)
 * iterations.  d_grad_prob [n_frames][max_points][L] = dL/dQ_{t_f} of every frame; d_grad_unary, d_grad_weights as in section 2c.
 *   - Per frame, the bits of section 1c at t_f: d_grad_unary[f] and d_grad_weights[f][:] are exactly what
 *     lccrf_inference_backward(h, t_f, relax, ...) returns for a handle holding frame f under the batch's weights -- the weight
 *     gradient's reduction over that frame's t_f x B partials included, in the handle's order and tree.  Rows at or beyond
 *     n_points[f] are written +0; a frame of 0 points gets zeros.  A frame with t_f = 0 gets section 2c's T = 0 results.
 *   - Afterwards frame f of the batch's Q holds Q_{t_f}: bit for bit what lccrf_batch_inference_converged left when the counts are
 *     its report.  Labels, label bits and the stored convergence report are not changed.
 *   - Every count equal to max_iterations: all outputs and the Q left behind are lccrf_batch_inference_backward(b, max_iterations,
 *     ...)'s, bit for bit.
 *   - The streaming route replays max_iterations steps for every frame (stepping a finished frame is wasted work, not a different
 *     result; its Q_{t_f} is put back from the history by one small kernel) and leaves frame f idle in the sweep while t > t_f.  Under
 *     LCCRF_OPT_FUSED_BACKWARD (section 1j), on the batches the one-launch backward takes, frame f's workgroup loads t_f once, runs t_f
 *     replays and t_f sweep steps and leaves its CU, the workgroups taking the frames by descending t_f (ranked on the device): the
 *     same bits.  lccrf_batch_get_backward_route reports the route of this call.
 *   - Everything else is section 2c's contract: it needs lccrf_batch_build or _run first (LCCRF_E_STATE otherwise); a pending
 *     one-launch run is settled first; deterministic, no float atomics; the batch-owned area is section 2c's with T = max_iterations
 *     and is never allocated by inference calls; LCCRF_E_INVALID for max_iterations < 0 or a relax that is not finite (these two and
 *     the NULL d_iterations are answered before the batch is looked at); a rejected call leaves the batch as it was; d_grad_weights
 *     may be NULL, K = 0 is legal.
 *   - Potts terms normalised AFTER only, as section 2c: on a batch with a matrix or a mode other than AFTER the call returns
 *     LCCRF_E_STATE and leaves the batch as it was: learnt models in section 2h's form are section 2k's.  Feature gradients at
 *     per-frame counts, the one-launch kernel of section 1l included, are section 2l's.
 * ==================================================================================== */
int  lccrf_batch_inference_backward_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                              const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights, void *stream);

/* ======================================================================================
 * 2k. Gradients of a batch's CONVERGED inference under a LEARNT model -- section 2h without d_grad_features, with section 2j's
 *     d_iterations: every frame of a batch with matrices (section 2g) or normalisation modes differentiated at its own iteration
 *     count, and the sums over the frames (lc-crf-slam_amd/autograd.py: mean_field_batch_compat_converged,
 *     BatchCompatConvergedMeanFieldCRF).  Added WITHOUT a step of LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.  Sections
 *     2c, 2d and 2j are unchanged and keep refusing what they refuse.
 *
 * The contract is the conjunction of sections 2h and 2j.  d_iterations: section 2j's device array of [n_frames] int32, read in stream
 * order and never by the host -- lccrf_batch_device_convergence's array goes straight in behind lccrf_batch_inference_converged on
 * the same stream.  Frame f is differentiated at t_f = min(max(d_iterations[f], 0), max_iterations).  Outputs as section 2h's, each
 * overwritten, each may be NULL: d_grad_unary, d_grad_weights, d_grad_compat, d_grad_model.
 *   - Per frame, the bits of section 1f at t_f: d_grad_unary[f], d_grad_weights[f] and d_grad_compat[f] are exactly what
 *     lccrf_inference_backward_all(h, t_f, relax, ..., NULL, d_grad_compat) returns for a handle holding frame f with the batch's
 *     weights, matrices and modes -- the chunk count C_f and the chunk order of dL/dmu and the t_f x B walk and tree of dL/dw included;
 *     a term without a matrix gets the derivative at mu = I.  Rows at or beyond n_points[f] of d_grad_unary are written +0; a frame of
 *     0 points gets zeros.
 *   - A frame with t_f = 0: d_grad_compat[f] and d_grad_weights[f] are exactly 0 -- whatever an earlier call left in the batch's
 *     area -- and dL/dU is section 2c's T = 0 result.
 *   - d_grad_model is section 2h's ascending-frame fp32 sum of this call's per-frame values (the caller's arrays, or the batch's area
 *     where the caller passed NULL): the same order, part of the contract; no float atomics.
 *   - Afterwards frame f of the batch's Q holds Q_{t_f}, bit for bit what lccrf_batch_inference_converged left when the counts are
 *     its report.  Labels, label bits and the stored convergence report are not changed.
 *   - Every count equal to max_iterations: every output and the Q left behind are lccrf_batch_inference_backward_all(b,
 *     max_iterations, relax, ..., NULL, d_grad_compat, d_grad_model, stream)'s, bit for bit.
 *   - On a batch without matrices or modes, with d_grad_compat == d_grad_model == NULL, the call is section 2j's: same bits, same route.
 *   - Routes: the streaming sweep leaves frame f idle while t > t_f (section 2j), the kernels of dL/dmu included.  Under
 *     LCCRF_OPT_FUSED_BACKWARD_LEARNT (section 1k), on the batches its one-launch kernel takes, frame f's workgroup loads t_f once and
 *     runs t_f replays and t_f sweep steps, the workgroups taking the frames by descending t_f; plus the two launches of
 *     d_grad_model.  The same bits: which workgroup runs a frame changes none.  lccrf_batch_get_backward_route reports the route.
 *   - Errors: max_iterations < 0, a relax that is not finite and a NULL d_iterations give LCCRF_E_INVALID before the batch is looked
 *     at; a device array that section 1b refuses gives LCCRF_E_INVALID; a call before lccrf_batch_build / _run gives LCCRF_E_STATE.
 *     A rejected call leaves the batch as it was.  K = 0 is legal.
 *   - Memory: section 2h's area at T = max_iterations.
 *   - Feature gradients at per-frame counts (sections 2d / 2i) are section 2l's.  Not covered (notes/convergence.md section 7):
 *     handle-level entry points (a handle's recipe stays lccrf_inference_backward_all at the reported count), the half-CU shapes.
 * ==================================================================================== */
int  lccrf_batch_inference_backward_all_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                                  const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights,
                                                  float *d_grad_compat, float *d_grad_model, void *stream);

/* ======================================================================================
 * 2l. FEATURE gradients of a batch's CONVERGED inference -- section 2i's call with section 2j's d_iterations: dL/d features of every
 *     term asked for, under any model (Potts or learnt, any normalisation mode), every frame differentiated at its own iteration
 *     count (lc-crf-slam_amd/autograd.py: mean_field_batch_features_converged, BatchLearnedKernelCRF).  Added WITHOUT a step of
 *     LCCRF_ABI_VERSION (it stays 3): probe for it by symbol.  Every other entry point is unchanged and keeps refusing what it refuses.
 *
 * The contract is the conjunction of sections 2i and 2j.  d_iterations: section 2j's device array of [n_frames] int32, read in stream
 * order and never by the host -- lccrf_batch_device_convergence's array goes straight in behind lccrf_batch_inference_converged on
 * the same stream.  Frame f is differentiated at t_f = min(max(d_iterations[f], 0), max_iterations) (the kernels clamp).  Outputs as
 * section 2i's, each overwritten, each may be NULL: d_grad_unary, d_grad_weights, d_grad_features (the array, or any entry),
 * d_grad_compat, d_grad_model.
 *   - Per frame, the bits of section 1m at t_f: d_grad_unary[f], d_grad_weights[f], d_grad_features[k][f] and d_grad_compat[f] are
 *     exactly what lccrf_inference_backward_modes(h, t_f, relax, ...) returns for a handle holding frame f with the batch's weights,
 *     matrices and modes -- the order of the additions into dL/d(corner weight) and the norm's accumulator included: t = t_f .. 1,
 *     slice side then splat side, post adjoint before pre adjoint, the norm part last.  Rows at or beyond n_points[f] of d_grad_unary
 *     and of every d_grad_features[k] are written +0; a frame of 0 points gets zeros.
 *   - A frame with t_f = 0: d_grad_features[k][f] is exactly +0 in every row -- the bits of the handle's memset at n_iterations = 0,
 *     whatever an earlier call left in the batch's area --, d_grad_weights[f] and d_grad_compat[f] are exactly 0 as in section 2k, and
 *     dL/dU is section 2c's T = 0 result.
 *   - d_grad_model is section 2h's ascending-frame fp32 sum of this call's per-frame values, with its bits.
 *   - Afterwards frame f of the batch's Q holds Q_{t_f}.  Labels, label bits and the stored convergence report are not changed.
 *   - d_grad_features == NULL, or every entry NULL: the call IS lccrf_batch_inference_backward_all_converged (section 2k): same bits,
 *     same route.
 *   - Every count equal to max_iterations: every output and the Q left behind are lccrf_batch_inference_backward_modes(b,
 *     max_iterations, relax, ...)'s, bit for bit.
 *   - Routes: the streaming sweep leaves frame f idle while t > t_f, the corner dots and the pre adjoint included -- nothing is added
 *     to an idle frame's accumulators, its dL/dQ stays the caller's; the norm part behind the sweep runs for every frame (at t_f = 0
 *     on zeroed accumulators: +0 out).  Under LCCRF_OPT_FUSED_BACKWARD_FEATURES, on the requests section 1l takes (Potts terms
 *     normalised AFTER, no d_grad_compat / d_grad_model, two labels, one or two 2-D terms, at most 2048 points), frame f's workgroup
 *     loads t_f once and runs t_f replays and t_f sweep steps, the workgroups taking the frames by descending t_f (ranked on the
 *     device); a frame with t_f = 0 skips the norm part and writes its dL/df as +0.  The same bits: which workgroup runs a frame
 *     changes none.  A learnt model with feature arrays streams.  lccrf_batch_get_backward_route reports the route.
 *   - Errors: max_iterations < 0, a relax that is not finite and a NULL d_iterations give LCCRF_E_INVALID before the batch is looked
 *     at; a device array that section 1b refuses gives LCCRF_E_INVALID; a call before lccrf_batch_build / _run gives LCCRF_E_STATE.
 *     A rejected call leaves the batch as it was.  K = 0 is legal.
 *   - Memory: section 2i's area at T = max_iterations.
 *   - Not covered (notes/convergence.md section 8): handle-level entry points (a handle's recipe stays
 *     lccrf_inference_backward_modes at the reported count), feature gradients of learnt models in one launch, the half-CU shapes, a
 *     streaming replay that stops stepping finished frames.
 * ==================================================================================== */
int  lccrf_batch_inference_backward_modes_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                                    const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights,
                                                    float *const *d_grad_features, float *d_grad_compat, float *d_grad_model,
                                                    void *stream);

/* ======================================================================================
 * 3. Unary builder -- the step right before the CRF (first "next" row):
 *    Tracking::ComputeMapPointErrAndObserv (src/Tracking.cc:1803-1839) for every candidate map
 *    point, then Tracking::RroughClassify (src/Tracking.cc:1961-2013).  The caller flattens the
 *    MapPoint -> observations -> KeyFrame graph of the frame into a CSR.  PARITY UNPINNED: the
 *    reference holds no test or fixture for these two functions.
 * ==================================================================================== */
typedef struct lccrf_crf_params {           /* Tracking.cc:151-171, Examples/RGB-D/TUM3.yaml:78-101 */
    float w1, w2;
    float u_alpha, stdev_alpha;             /* reprojection error mean / stdev            */
    float u_beta, stdev_beta;               /* observation count mean / stdev             */
    float u_gamma, stdev_gamma;             /* epipolar prior (read by the reference, unused here) */
    float point3d_stdev, point2d_stdev;
    float u_depth, pth, confidence;
} lccrf_crf_params;

void lccrf_default_params(lccrf_crf_params *p);       /* the TUM3.yaml / BONN.yaml values */

/* Host arrays in, host arrays out.
 *   Xw        [n_points][3]   MapPoint::GetWorldPos()
 *   obs_ptr   [n_points+1]    observations of point i are obs_*[obs_ptr[i] .. obs_ptr[i+1])
 *   obs_kf    [n_obs]         index of the observing keyframe
 *   obs_kp    [n_obs][2]      pKF->mvKeysUn[fid].pt as doubles (Point2d, Tracking.cc:1832)
 *   kf_pose   [n_kf][12]      row-major 3x4 [Rcw | tcw];  kf_intr [n_kf][4] fx fy cx cy;
 *   kf_bounds [n_kf][4]       mnMinX mnMaxX mnMinY mnMaxY
 *   match_prob[n_points]      mvFeatureMatchProb per candidate, or NULL if that map is empty
 * Outputs (each [n_points]): observation count (as float, like the reference's vector<float>),
 * mean reprojection error, mean depth, rough label (0 moving, 1 static, -1 for a point without
 * observations, which the reference drops at Tracking.cc:1858).                              */
int  lccrf_unary_build(int device_id, int n_points, const float *Xw, const int32_t *obs_ptr,
                       const int32_t *obs_kf, const double *obs_kp, int n_kf, const float *kf_pose,
                       const float *kf_intr, const float *kf_bounds, const double *match_prob,
                       const lccrf_crf_params *params, float *observs_out, float *error_out,
                       float *depth_out, int16_t *label_out);

/* ======================================================================================
 * 4. Static-feature matcher (another "next" row)
 *
 * Tracking::BfMatch (src/Tracking.cc:1747-1766): cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2)
 * of the current frame's ORB descriptors (query) against a frame 15 frames back (train), kept
 * when `match[0].distance < match[1].distance * 0.6`.  Host arrays in, host arrays out:
 *   desc_query [n_query][32], desc_train [n_train][32]   256-bit ORB descriptors (Frame::mDescriptors rows)
 *   ratio                                                0.6 in the reference
 *   train_of_query_out [n_query]                         asso[fid1] = fid2 of :1762, or -1 (no entry)
 *   n_matches_out                                        asso.size(), may be NULL
 * Ties follow OpenCV's batchDistance: the two nearest are the two smallest (distance, train
 * index) pairs.  Parity is unpinned (no OpenCV here); exact against the oracle's restatement.
 * Fewer than two train descriptors give no matches (match.size() != 2).                    */
int  lccrf_bf_match(int device_id, int n_query, const uint8_t *desc_query, int n_train,
                    const uint8_t *desc_train, double ratio, int32_t *train_of_query_out,
                    int32_t *n_matches_out);

/* ======================================================================================
 * 5. Pose optimisation -- the step right after the CRF
 *
 * Optimizer::PoseOptimization (src/Optimizer.cc:239-450, called at src/Tracking.cc:1002): motion-only bundle
 * adjustment of the frame pose on the matches the CRF left standing -- g2o Levenberg-Marquardt on one SE3 vertex,
 * pose-only reprojection edges (monocular where u_right < 0, stereo otherwise), Huber kernel, 4 rounds of 10
 * iterations from the same initial pose with chi2 re-classification (5.991 / 7.815) in between.  PARITY UNPINNED:
 * g2o needs Eigen (absent here) and the reference holds no fixture for it; csrc/pose_opt.hip states what is and is
 * not reproduced.  Double precision on the device, one workgroup per frame.
 *   Xw [n][3]         MapPoint::GetWorldPos()              kp [n][2]   mvKeysUn[i].pt
 *   u_right [n]       mvuRight[i] (< 0: monocular edge)    inv_sigma2 [n]  mvInvLevelSigma2[kpUn.octave]
 *   valid [n]         mvpMapPoints[i] != NULL, or NULL for "all"
 *   label [n]         CRF labels, or NULL: a point labelled 0 (moving) has been nulled by
 *                     Tracking::DynamicDetectionWithCRF (Tracking.cc:1945-1955) and contributes no edge
 *   K4                fx fy cx cy;  bf = mbf;  Tcw row-major 4x4 float (pFrame->mTcw in, SetPose out)
 *   outlier_out [n]   mvbOutlier (entries of points without an edge are left as they were)
 *   n_inliers_out     the return value nInitialCorrespondences - nBad (0 with < 3 correspondences: pose untouched)
 * Synchronous, host arrays in and out; thread-safe (calls on one device share a cached staging area and take turns);
 * at most 16384 keypoints (up to 4096 the frame's edges are staged in LDS).                                        */
int  lccrf_pose_optimization(int device_id, int n_points, const float *Xw, const float *kp, const float *u_right,
                             const float *inv_sigma2, const uint8_t *valid, const int16_t *label, const float *K4,
                             float bf, const float *Tcw_in, float *Tcw_out, uint8_t *outlier_out,
                             int32_t *n_inliers_out);
/* The same for every frame of a batch, on DEVICE arrays strided by the batch's max_points ([F][max_points][..],
 * Tcw [F][16], counts [F]), with the labels of the batch's last inference read where the kernel left them: the
 * labels never visit the host between the CRF and the pose.  Asynchronous on `stream` (NULL: the batch's own);
 * behind a lccrf_batch_run whose fallback is still unresolved it first settles that (one synchronisation).
 * LCCRF_E_STATE if the last inference ran with with_map = 0 (no labels).
 * CRF-ORDER CONTRACT: arrays are indexed by CRF point index i (the order in which DynamicDetectionWithCRF pushed
 * its candidates, Tracking.cc:1849-1870), label i gates edge i.  The reference's PoseOptimization instead walks all
 * pFrame->N keypoints with a non-null map point (Optimizer.cc:281-360): that includes map points the CRF skipped
 * because observs == 0 (Tracking.cc:1857-1859), which still contribute an edge there.  Append those as extra points
 * behind a frame's CRF points -- rows [n_crf, n_points) with d_valid = 1 -- and say how many CRF points each frame
 * has through lccrf_batch_pose_set_crf_counts(); points beyond that count are treated as static (label 1).          */
int  lccrf_batch_pose_optimization(lccrf_batch_handle b, const float *d_Xw, const float *d_kp, const float *d_u_right,
                                   const float *d_inv_sigma2, const uint8_t *d_valid, const float *K4, float bf,
                                   const float *d_Tcw_in, float *d_Tcw_out, uint8_t *d_outlier,
                                   int32_t *d_n_inliers, int32_t *d_n_initial, void *stream);
/* Optional: d_n_total[f] >= the CRF's n_points[f] (device array [F], bound, not copied) = CRF points + the extra
 * non-CRF edges of the contract above; NULL (default) = only the CRF's points carry edges.                          */
int  lccrf_batch_pose_set_crf_counts(lccrf_batch_handle b, const int32_t *d_n_total);

#ifdef __cplusplus
}
#endif
#endif /* LCCRF_H */

// api_tools.hip -- the entry points of include/lccrf.h that own no handle: version, errors, devices, process-wide defaults, and the
// stateless tools around the CRF (unary builder, matcher, pose optimisation).  The calling thread's error text lives here, and
// nowhere else.
#include "api_common.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

using namespace lccrf;

namespace {

thread_local std::string g_err;

// lccrf_pose_optimization's staging area (device + pinned host + stream), one per device, kept between calls: the
// reference calls Optimizer::PoseOptimization once per frame (src/Tracking.cc:1002) and an allocation costs more than the solve.
struct PoseStage {
    std::mutex m;
    char *d = nullptr, *h = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
};
constexpr int kMaxDevices = 64;
PoseStage g_pose_stage[kMaxDevices];

std::atomic<int> g_default_single_wg{0};
std::atomic<int> g_default_frame_general{0};
std::atomic<int> g_default_fused_multilabel{0};
}  // namespace

int lccrf::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int lccrf::use_device(int device_id)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(LCCRF_E_NO_DEVICE, "no HIP device (hipGetDeviceCount: %s); this library has no CPU fallback",
                    hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(LCCRF_E_INVALID, "device_id %d out of range [0,%d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    return LCCRF_OK;
}

bool lccrf::default_single_wg() { return g_default_single_wg.load(std::memory_order_relaxed) != 0; }
bool lccrf::default_frame_general() { return g_default_frame_general.load(std::memory_order_relaxed) != 0; }
bool lccrf::default_fused_multilabel() { return g_default_fused_multilabel.load(std::memory_order_relaxed) != 0; }

// lccrf_trim_cache: the pose-optimisation staging areas
void lccrf::trim_pose_stages()
{
    for (int d = 0; d < kMaxDevices; ++d) {
        PoseStage &ps = g_pose_stage[d];
        std::lock_guard<std::mutex> g(ps.m);
        if (!ps.d && !ps.h && !ps.stream) continue;
        (void)hipSetDevice(d);
        if (ps.stream) { (void)hipStreamSynchronize(ps.stream); (void)hipStreamDestroy(ps.stream); }
        if (ps.d) (void)hipFree(ps.d);
        if (ps.h) (void)hipHostFree(ps.h);
        ps.d = ps.h = nullptr; ps.stream = nullptr; ps.cap = 0;
    }
}

extern "C" {

int lccrf_abi_version(void) { return LCCRF_ABI_VERSION; }
const char *lccrf_last_error(void) { return g_err.c_str(); }

int lccrf_device_count(int *count)
{
    if (!count) return fail(LCCRF_E_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(LCCRF_E_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return LCCRF_OK;
}

int lccrf_set_default_option(int option, int value)
{
    switch (option) {
    case LCCRF_OPT_SINGLE_WORKGROUP: g_default_single_wg.store(value != 0, std::memory_order_relaxed); return LCCRF_OK;
    case LCCRF_OPT_FRAME_GENERAL: g_default_frame_general.store(value != 0, std::memory_order_relaxed); return LCCRF_OK;
    case LCCRF_OPT_FUSED_MULTILABEL: g_default_fused_multilabel.store(value != 0, std::memory_order_relaxed); return LCCRF_OK;
    default: return fail(LCCRF_E_INVALID, "option %d has no process-wide default", option);
    }
}

void lccrf_default_params(lccrf_crf_params *p)       // Examples/RGB-D/TUM3.yaml:78-101
{
    if (!p) return;
    p->w1 = 10.0f; p->w2 = 30.0f;
    p->u_alpha = 1.7f; p->stdev_alpha = 0.6f;
    p->u_beta = 5.4f; p->stdev_beta = 1.5f;
    p->u_gamma = 0.3f; p->stdev_gamma = 0.2f;
    p->point3d_stdev = 0.5f; p->point2d_stdev = 18.0f;
    p->u_depth = 2.75f; p->pth = 0.8f; p->confidence = 0.7f;
}

int lccrf_unary_build(int device_id, int n_points, const float *Xw, const int32_t *obs_ptr, const int32_t *obs_kf,
                      const double *obs_kp, int n_kf, const float *kf_pose, const float *kf_intr, const float *kf_bounds,
                      const double *match_prob, const lccrf_crf_params *params, float *observs_out, float *error_out,
                      float *depth_out, int16_t *label_out)
{
    if (n_points < 0 || n_kf < 0) return fail(LCCRF_E_INVALID, "negative size");
    if (!params || !obs_ptr) return fail(LCCRF_E_INVALID, "params / obs_ptr is NULL");
    if (n_points && (!Xw || !observs_out || !error_out || !depth_out || !label_out))
        return fail(LCCRF_E_INVALID, "NULL array");
    const int n_obs = n_points ? obs_ptr[n_points] : 0;
    if (n_obs < 0 || (n_obs && (!obs_kf || !obs_kp || !kf_pose || !kf_intr || !kf_bounds)))
        return fail(LCCRF_E_INVALID, "observation arrays missing");
    for (int i = 0; i < n_points; ++i)
        if (obs_ptr[i + 1] < obs_ptr[i]) return fail(LCCRF_E_INVALID, "obs_ptr not monotone at %d", i);
    for (int o = 0; o < n_obs; ++o)
        if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) return fail(LCCRF_E_INVALID, "obs_kf[%d]=%d out of range", o, obs_kf[o]);
    int rc = use_device(device_id);
    if (rc) return rc;
    hipError_t e = run_unary_build(device_id, n_points, Xw, obs_ptr, obs_kf, obs_kp, n_kf, kf_pose, kf_intr, kf_bounds,
                                   match_prob, params, observs_out, error_out, depth_out, label_out);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? LCCRF_E_NOMEM : LCCRF_E_HIP, "unary builder: %s", hipGetErrorString(e));
    return LCCRF_OK;
}

int lccrf_bf_match(int device_id, int n_query, const uint8_t *desc_query, int n_train, const uint8_t *desc_train,
                   double ratio, int32_t *train_of_query_out, int32_t *n_matches_out)
{
    if (n_query < 0 || n_train < 0) return fail(LCCRF_E_INVALID, "negative size");
    if (n_train >= (1 << 22)) return fail(LCCRF_E_CAPACITY, "at most %d train descriptors", (1 << 22) - 1);
    if ((n_query && (!desc_query || !train_of_query_out)) || (n_train && !desc_train))
        return fail(LCCRF_E_INVALID, "NULL descriptor / output array");
    if (!(ratio >= 0.0)) return fail(LCCRF_E_INVALID, "ratio must be >= 0");
    int rc = use_device(device_id);
    if (rc) return rc;
    hipError_t e = run_bf_match(device_id, n_query, desc_query, n_train, desc_train, ratio, train_of_query_out, n_matches_out);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? LCCRF_E_NOMEM : LCCRF_E_HIP, "bf_match: %s", hipGetErrorString(e));
    return LCCRF_OK;
}

int lccrf_pose_optimization(int device_id, int n_points, const float *Xw, const float *kp, const float *u_right,
                            const float *inv_sigma2, const uint8_t *valid, const int16_t *label, const float *K4, float bf,
                            const float *Tcw_in, float *Tcw_out, uint8_t *outlier_out, int32_t *n_inliers_out)
{
    if (n_points < 0) return fail(LCCRF_E_INVALID, "n_points < 0");
    if (n_points > 16384) return fail(LCCRF_E_CAPACITY, "at most 16384 keypoints per frame");
    if (!K4 || !Tcw_in || !Tcw_out) return fail(LCCRF_E_INVALID, "K4 / Tcw is NULL");
    if (n_points && (!Xw || !kp || !u_right || !inv_sigma2 || !outlier_out)) return fail(LCCRF_E_INVALID, "NULL array");
    int rc = use_device(device_id);
    if (rc) return rc;
    if (device_id >= kMaxDevices) return fail(LCCRF_E_INVALID, "device_id %d beyond the staging table", device_id);
    const size_t n = (size_t)std::max(n_points, 1), n16 = (n + 15) & ~(size_t)15;
    // one staging area per call, laid out the same in pinned host memory and in device memory:
    //   [Xw | kp | ur | is2 | Tin | Tout | ints (n_points, n_inliers, n_initial, -) | outlier | label | valid]
    // one copy in (everything), one copy out ([Tout | ints | outlier]), on the context's own stream.
    const size_t off_kp = n * 12, off_ur = off_kp + n * 8, off_is2 = off_ur + n * 4, off_tin = off_is2 + n * 4, off_tout = off_tin + 64,
                 off_int = off_tout + 64, off_out = off_int + 16, off_lab = off_out + n16, off_val = off_lab + 2 * n16, total = off_val + n16;
    PoseStage &ps = g_pose_stage[device_id];
    std::lock_guard<std::mutex> guard(ps.m);
    if (ps.cap < total) {
        if (ps.d) (void)hipFree(ps.d);
        if (ps.h) (void)hipHostFree(ps.h);
        ps.d = ps.h = nullptr; ps.cap = 0;
        const size_t want = std::max<size_t>(total + total / 2, 1 << 16);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ps.d), want));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ps.h), want));
        if (!ps.stream) HIP_TRY(hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking));
        ps.cap = want;
    }
    char *d = ps.d, *h = ps.h;
    if (n_points) {
        memcpy(h, Xw, (size_t)n_points * 12);
        memcpy(h + off_kp, kp, (size_t)n_points * 8);
        memcpy(h + off_ur, u_right, (size_t)n_points * 4);
        memcpy(h + off_is2, inv_sigma2, (size_t)n_points * 4);
        if (label) memcpy(h + off_lab, label, (size_t)n_points * 2);
        if (valid) memcpy(h + off_val, valid, (size_t)n_points);
        memcpy(h + off_out, outlier_out, (size_t)n_points);                      // entries of invalid points pass through
    }
    memcpy(h + off_tin, Tcw_in, 64);
    int *hints = reinterpret_cast<int *>(h + off_int);
    hints[0] = n_points; hints[1] = hints[2] = hints[3] = 0;
    HIP_TRY(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ps.stream));
    int *ints = reinterpret_cast<int *>(d + off_int);
    hipError_t er = launch_pose_optimization(1, (int)n, ints, reinterpret_cast<float *>(d), reinterpret_cast<float *>(d + off_kp),
                                             reinterpret_cast<float *>(d + off_ur), reinterpret_cast<float *>(d + off_is2),
                                             valid ? reinterpret_cast<uint8_t *>(d + off_val) : nullptr,
                                             label ? reinterpret_cast<int16_t *>(d + off_lab) : nullptr, K4, bf,
                                             reinterpret_cast<float *>(d + off_tin), reinterpret_cast<float *>(d + off_tout),
                                             reinterpret_cast<uint8_t *>(d + off_out), ints + 1, ints + 2, ps.stream);
    if (er != hipSuccess) return fail(LCCRF_E_HIP, "pose optimisation: %s", hipGetErrorString(er));
    HIP_TRY(hipMemcpyAsync(h + off_tout, d + off_tout, 64 + 16 + (size_t)n_points, hipMemcpyDeviceToHost, ps.stream));
    HIP_TRY(hipStreamSynchronize(ps.stream));
    memcpy(Tcw_out, h + off_tout, 64);
    if (n_points) memcpy(outlier_out, h + off_out, (size_t)n_points);
    if (n_inliers_out) *n_inliers_out = hints[1];
    return LCCRF_OK;
}

}  // extern "C"

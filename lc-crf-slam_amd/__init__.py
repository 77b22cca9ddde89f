"""lc-crf-slam_amd -- MI355X-native dense-CRF mean-field path of LC-CRF-SLAM.

Python here is plumbing only: a ctypes binding of the C-ABI in include/lccrf.h
(liblccrf_hip.so, hand-written gfx950 HIP kernels) plus numpy-facing mirrors of the
reference's operator interface (densecrf_base.h: DenseCRF / PairwisePotential) so that
the parity tests read like the reference's call site (src/Tracking.cc:1919-1930).

There is no CPU fallback: if the library is missing, or no GPU is usable, calls raise.

Import with  importlib.import_module("lc-crf-slam_amd")  (the directory name is fixed
by the project layout and is not a valid identifier).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LCCRF_LIB selects another build of the same library (e.g. liblccrf_hip_instr.so from `make INSTRUMENT=1`,
# used by scripts/gpu_stamps.sh); it must exist -- there is no fallback of any kind.
LIB_PATH = os.environ.get("LCCRF_LIB") or os.path.join(_HERE, "liblccrf_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lccrf.h")

MAX_KERNELS = 8
OPT_SINGLE_WORKGROUP = 1        # lccrf_option (include/lccrf.h)
OPT_VERTEX_ORDER = 2
OPT_FRAME_GENERAL = 5           # a learnt model (matrices, normalisation modes) may take the one-launch route of a fresh frame
OPT_FUSED_BACKWARD = 6          # gradients of tracker-sized two-label frames in one launch (include/lccrf.h section 1j)
OPT_FUSED_BACKWARD_LEARNT = 7   # ... of learnt models (matrices, normalisation modes) and dL/dmu (include/lccrf.h section 1k)
OPT_FUSED_BACKWARD_FEATURES = 8 # ... with feature gradients on Potts terms normalised AFTER (include/lccrf.h section 1l)
OPT_FUSED_MULTILABEL = 9        # frames of three to eight labels on lattices in HBM infer in one launch (csrc/fused_multilabel.hip)
MULTILABEL_POTTS, MULTILABEL_LEARNT = 1, 2   # lccrf_set_multilabel_routes' bits: POTTS is OPT_FUSED_MULTILABEL, LEARNT moves matrices and modes
BACKWARD_NONE, BACKWARD_STREAM, BACKWARD_FUSED = 0, 1, 2   # lccrf_backward_route
IMAGE_NONE, IMAGE_U8, IMAGE_F32 = 0, 1, 2   # lccrf_add_image_kernel's image formats
NORMALIZE_AFTER, NORMALIZE_BEFORE, NORMALIZE_SYMMETRIC, NORMALIZE_NONE = 0, 1, 2, 3   # lccrf_normalization (section 1g)
STOP_DELTA, STOP_LABELS = 1, 2   # lccrf_inference_converged's criterion bits (section 1h)
OK = 0
_STATUS = {0: "OK", -1: "E_INVALID", -2: "E_NO_DEVICE", -3: "E_HIP", -4: "E_NOMEM", -5: "E_STATE",
           -6: "E_CAPACITY"}

_f32p = C.POINTER(C.c_float)
_i16p = C.POINTER(C.c_int16)
_i32p = C.POINTER(C.c_int32)


class LccrfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lccrf %s (%d): %s" % (_STATUS.get(code, "?"), code, msg))
        self.code = code


class CrfParams(C.Structure):
    """lccrf_crf_params: the CRF block of TUM3.yaml (Tracking.cc:151-171)."""
    _fields_ = [(n, C.c_float) for n in (
        "w1", "w2", "u_alpha", "stdev_alpha", "u_beta", "stdev_beta", "u_gamma", "stdev_gamma",
        "point3d_stdev", "point2d_stdev", "u_depth", "pth", "confidence")]


class SplatPlan(C.Structure):
    """lccrf_splat_plan"""
    _fields_ = [(n, C.c_int32) for n in ("passes", "halo", "window", "lanes", "vertices_per_lane", "long_mode")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BlurPlan(C.Structure):
    """lccrf_blur_plan"""
    _fields_ = [(n, C.c_int32) for n in ("in_splat", "paired_table", "paired_plain", "alone_32bit", "alone_compact", "in_slice",
                                         "nontemporal", "first_table_pair")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BuildReport(C.Structure):
    """lccrf_build_report"""
    _fields_ = [(n, C.c_int32) for n in ("sorted_build", "direct_codes", "long_buckets", "long_by_bitmap", "long_by_network_uniform",
                                         "long_by_network_mixed", "long_by_network_wide", "max_buckets_per_workgroup", "phantom_entries",
                                         "empty_row_vertices", "long_rows", "point_buckets_over_64", "largest_point_bucket")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BatchDesc(C.Structure):
    _fields_ = [("max_frames", C.c_int), ("max_points", C.c_int), ("n_labels", C.c_int),
                ("n_kernels", C.c_int), ("feat_dims", C.c_int * MAX_KERNELS),
                ("weights", C.c_float * MAX_KERNELS)]


def build_library(quiet=True):
    """Compile liblccrf_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", _HERE, "-j4", "all"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            LIB_PATH + " is missing: build it with `make -C lc-crf-slam_amd` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lccrf_last_error.restype = C.c_char_p
    L.lccrf_device_count.argtypes = [C.POINTER(C.c_int)]
    L.lccrf_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int]
    L.lccrf_destroy.argtypes = [vp]
    L.lccrf_destroy.restype = None
    L.lccrf_trim_cache.argtypes = []
    L.lccrf_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.lccrf_batch_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.lccrf_set_default_option.argtypes = [C.c_int, C.c_int]
    L.lccrf_set_unary.argtypes = [vp, _f32p]
    L.lccrf_set_unary_from_label.argtypes = [vp, _i16p, _f32p]
    L.lccrf_add_pairwise.argtypes = [vp, _f32p, C.c_int, C.c_float]
    L.lccrf_add_appearance_kernel.argtypes = [vp, C.c_float, _f32p, _f32p, C.c_float, C.c_float]
    L.lccrf_add_smooth_kernel.argtypes = [vp, C.c_float, _f32p, C.c_float]
    L.lccrf_start_inference.argtypes = [vp]
    L.lccrf_step_inference.argtypes = [vp, C.c_float]
    L.lccrf_build_map.argtypes = [vp]
    L.lccrf_inference.argtypes = [vp, C.c_int, C.c_int, C.c_float]
    L.lccrf_get_map.argtypes = [vp, _i16p]
    L.lccrf_get_probability.argtypes = [vp, _f32p]
    L.lccrf_get_engine.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lccrf_get_unary.argtypes = [vp, _f32p]
    L.lccrf_inference_converged.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float]
    L.lccrf_get_convergence.argtypes = [vp, C.POINTER(C.c_int), _f32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lccrf_batch_inference_converged.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp]
    L.lccrf_run_converged.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float]
    L.lccrf_batch_run_converged.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp]
    L.lccrf_batch_get_convergence_host.argtypes = [vp, _i32p, _f32p, _i32p, _i32p]
    L.lccrf_batch_device_convergence.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.lccrf_get_lattice_size.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.lccrf_pairwise_apply.argtypes = [vp, C.c_int, _f32p, _f32p]
    L.lccrf_exp_and_normalize.argtypes = [vp, _f32p, _f32p, C.c_float, C.c_float]
    L.lccrf_step_init.argtypes = [vp, _f32p]
    L.lccrf_map_of.argtypes = [vp, _f32p, _i16p]
    L.lccrf_lattice_filter.argtypes = [C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.POINTER(C.c_int)]
    L.lccrf_get_norm.argtypes = [vp, C.c_int, _f32p]
    L.lccrf_get_lattice.argtypes = [vp, C.c_int, _i32p, _f32p, _i32p]
    L.lccrf_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.lccrf_synchronize.argtypes = [vp]
    L.lccrf_set_unary_device.argtypes = [vp, vp]
    L.lccrf_set_unary_from_label_device.argtypes = [vp, vp, _f32p]
    L.lccrf_add_pairwise_device.argtypes = [vp, vp, C.c_int, C.c_float]
    L.lccrf_add_image_kernel.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, C.c_float]
    L.lccrf_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.lccrf_pairwise_apply_device.argtypes = [vp, C.c_int, vp, vp]
    L.lccrf_exp_and_normalize_device.argtypes = [vp, vp, vp, C.c_float, C.c_float]
    L.lccrf_step_init_device.argtypes = [vp, vp]
    L.lccrf_map_of_device.argtypes = [vp, vp, vp]
    L.lccrf_set_pairwise_weight.argtypes = [vp, C.c_int, C.c_float]
    L.lccrf_inference_backward.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp]
    L.lccrf_inference_backward_features.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp)]
    for name in ("lccrf_get_backward_route", "lccrf_batch_get_backward_route"):   # (section 1j: probe by symbol -- a library from before
        if hasattr(L, name):                                                      #  the route, named through LCCRF_LIB, has neither)
            getattr(L, name).argtypes = [vp, C.POINTER(C.c_int)]
    for prefix in ("lccrf_", "lccrf_batch_"):                                     # (added without an ABI step: probe by symbol too)
        if hasattr(L, prefix + "set_multilabel_routes"):
            getattr(L, prefix + "set_multilabel_routes").argtypes = [vp, C.c_uint]
            getattr(L, prefix + "get_multilabel_routes").argtypes = [vp, C.POINTER(C.c_uint)]
    L.lccrf_set_pairwise_compatibility.argtypes = [vp, C.c_int, _f32p]
    L.lccrf_get_pairwise_compatibility.argtypes = [vp, C.c_int, _f32p, C.POINTER(C.c_int)]
    L.lccrf_inference_backward_compat.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, vp]
    L.lccrf_inference_backward_all.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp), vp]
    L.lccrf_inference_backward_modes.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp), vp]
    L.lccrf_set_pairwise_normalization.argtypes = [vp, C.c_int, C.c_int]
    L.lccrf_get_pairwise_normalization.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.lccrf_batch_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(BatchDesc)]
    L.lccrf_batch_destroy.argtypes = [vp]
    L.lccrf_batch_destroy.restype = None
    L.lccrf_batch_set_inputs_host.argtypes = [vp, C.c_int, _i32p, _f32p, _i16p, _f32p, C.POINTER(_f32p)]
    L.lccrf_batch_bind_inputs_device.argtypes = [vp, C.c_int, vp, vp, vp, _f32p, C.POINTER(vp)]
    L.lccrf_batch_set_inputs_host_async.argtypes = [vp, C.c_int, vp, vp, vp, _f32p, C.POINTER(vp), C.c_int]
    L.lccrf_batch_wait_inputs.argtypes = [vp]
    L.lccrf_batch_download_async.argtypes = [vp, C.c_int]
    L.lccrf_batch_wait_download.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(vp)]
    L.lccrf_batch_build.argtypes = [vp, vp]
    L.lccrf_batch_inference.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp]
    L.lccrf_batch_run.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp]
    L.lccrf_batch_synchronize.argtypes = [vp]
    L.lccrf_batch_get_map_host.argtypes = [vp, _i16p]
    L.lccrf_batch_get_probability_host.argtypes = [vp, _f32p]
    L.lccrf_batch_get_lattice_sizes_host.argtypes = [vp, C.c_int, _i32p]
    L.lccrf_batch_get_norm_host.argtypes = [vp, C.c_int, _f32p]
    L.lccrf_batch_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.lccrf_batch_device_label_bits.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
    L.lccrf_batch_set_engine.argtypes = [vp, C.c_int]
    L.lccrf_batch_get_engine.argtypes = [vp, C.POINTER(C.c_int)]
    L.lccrf_batch_get_fallback_frames.argtypes = [vp, C.POINTER(C.c_int)]
    L.lccrf_batch_get_fused_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lccrf_batch_get_locality_mode.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lccrf_batch_get_splat_plan.argtypes = [vp, C.c_int, C.POINTER(SplatPlan)]
    L.lccrf_get_splat_plan.argtypes = [vp, C.c_int, C.POINTER(SplatPlan)]
    L.lccrf_batch_get_blur_plan.argtypes = [vp, C.c_int, C.POINTER(BlurPlan)]
    L.lccrf_get_blur_plan.argtypes = [vp, C.c_int, C.POINTER(BlurPlan)]
    L.lccrf_batch_get_build_report.argtypes = [vp, C.c_int, C.c_int, C.POINTER(BuildReport)]
    L.lccrf_get_build_report.argtypes = [vp, C.c_int, C.POINTER(BuildReport)]
    L.lccrf_batch_get_built_lattice.argtypes = [vp, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _f32p, _i32p, _i32p, _f32p, _i32p,
                                                C.POINTER(C.c_uint8), C.POINTER(C.c_int)]
    L.lccrf_batch_pose_set_crf_counts.argtypes = [vp, vp]
    L.lccrf_batch_last_timing.argtypes = [vp, _f32p, _f32p]
    L.lccrf_batch_last_prepare.argtypes = [vp, _f32p, C.POINTER(C.c_int)]
    L.lccrf_batch_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.lccrf_batch_time_blur_pass.argtypes = [vp, C.c_int, C.c_int, _f32p, C.POINTER(C.c_int64)]
    L.lccrf_batch_set_pairwise_weight.argtypes = [vp, C.c_int, C.c_float]
    L.lccrf_batch_set_unary_device.argtypes = [vp, vp]
    L.lccrf_batch_inference_backward.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, vp]
    L.lccrf_batch_inference_backward_features.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp), vp]
    L.lccrf_batch_inference_backward_all.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp), vp, vp, vp]
    L.lccrf_batch_inference_backward_modes.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, C.POINTER(vp), vp, vp, vp]
    if hasattr(L, "lccrf_batch_inference_backward_converged"):                    # (section 2j: probe by symbol)
        L.lccrf_batch_inference_backward_converged.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, vp, vp]
    if hasattr(L, "lccrf_batch_inference_backward_all_converged"):                # (section 2k: probe by symbol)
        L.lccrf_batch_inference_backward_all_converged.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "lccrf_batch_inference_backward_modes_converged"):              # (section 2l: probe by symbol)
        L.lccrf_batch_inference_backward_modes_converged.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp, vp, C.POINTER(vp), vp, vp, vp]
    L.lccrf_batch_set_pairwise_compatibility.argtypes = [vp, C.c_int, _f32p]
    L.lccrf_batch_get_pairwise_compatibility.argtypes = [vp, C.c_int, _f32p, C.POINTER(C.c_int)]
    L.lccrf_batch_set_pairwise_normalization.argtypes = [vp, C.c_int, C.c_int]
    L.lccrf_batch_get_pairwise_normalization.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.lccrf_bf_match.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, _i32p, _i32p]
    L.lccrf_pose_optimization.argtypes = [C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, C.c_void_p, _i16p, _f32p, C.c_float,
                                          _f32p, _f32p, C.c_void_p, _i32p]
    L.lccrf_batch_pose_optimization.argtypes = [vp, vp, vp, vp, vp, vp, _f32p, C.c_float, vp, vp, vp, vp, vp, vp]
    L.lccrf_default_params.argtypes = [C.POINTER(CrfParams)]
    L.lccrf_default_params.restype = None
    L.lccrf_unary_build.argtypes = [C.c_int, C.c_int, _f32p, _i32p, _i32p, C.POINTER(C.c_double), C.c_int, _f32p,
                                    _f32p, _f32p, C.POINTER(C.c_double), C.POINTER(CrfParams), _f32p, _f32p, _f32p,
                                    _i16p]
    _lib = L
    return L


def _check(rc):
    if rc != OK:
        raise LccrfError(rc, lib().lccrf_last_error().decode("utf-8", "replace"))


def _addr(p):
    """a raw device address (or None / 0: NULL) as a C pointer argument"""
    return C.c_void_p(int(p)) if p else None


def _addr_list(ps):
    """a list of raw device addresses (None entries: NULL) as a host array of pointers; None: NULL"""
    if ps is None:
        return None
    return (C.c_void_p * max(len(ps), 1))(*[_addr(p) for p in ps])


def set_default_option(option, value):
    _check(lib().lccrf_set_default_option(int(option), int(value)))


def device_count():
    n = C.c_int(0)
    _check(lib().lccrf_device_count(C.byref(n)))
    return n.value


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a, t):
    return a.ctypes.data_as(t)


class _Handle:
    """What DenseCRFHIP and BatchCRF share: the calls of sections 1 and 2 that differ in the C name's prefix alone (_PREFIX:
    lccrf_ / lccrf_batch_), on the handle self.h of self.L labels.  For a batch they act on every frame."""
    _PREFIX = None

    def _c(self, name):
        return getattr(lib(), self._PREFIX + name)

    def close(self):
        if getattr(self, "h", None):
            self._c("destroy")(self.h)
            self.h = None

    __del__ = close

    def set_option(self, option, value):
        _check(self._c("set_option")(self.h, int(option), int(value)))

    def set_multilabel_routes(self, routes):
        """Which one-launch kernels a fixed count on frames of three to eight labels may take: a mask of MULTILABEL_POTTS (the same
        switch as OPT_FUSED_MULTILABEL: engine 5) and MULTILABEL_LEARNT (terms with a matrix or a normalisation mode: engine 6).  Same
        bits on every route (include/lccrf.h: lccrf_set_multilabel_routes)."""
        _check(self._c("set_multilabel_routes")(self.h, int(routes)))

    def multilabel_routes(self):
        r = C.c_uint(0)
        _check(self._c("get_multilabel_routes")(self.h, C.byref(r)))
        return r.value

    def set_pairwise_weight(self, k, w):
        """PottsPotential3D::w_ of term k; the next inference equals that of a handle or batch created with weight w."""
        _check(self._c("set_pairwise_weight")(self.h, int(k), float(w)))

    # -- label-compatibility matrices (include/lccrf.h sections 1e and 2g) ----------------------------------------------------------
    def set_pairwise_compatibility(self, k, compat):
        """The [L][L] matrix mu of term k: next[i][l] += w * norm[i] * sum_l' mu[l][l'] * Phi(Q)[i][l'].  None: Potts again."""
        m = None
        if compat is not None:
            m = _f32(compat).reshape(-1)
            if m.size != self.L * self.L:
                raise ValueError("compat must have L*L entries")
        _check(self._c("set_pairwise_compatibility")(self.h, int(k), None if m is None else _p(m, _f32p)))

    def get_pairwise_compatibility(self, k):
        """(matrix [L][L], is_set) of term k; the identity for a term without a matrix."""
        out = np.empty((self.L, self.L), np.float32)
        flag = C.c_int(0)
        _check(self._c("get_pairwise_compatibility")(self.h, int(k), _p(out, _f32p), C.byref(flag)))
        return out, bool(flag.value)

    # -- normalisation modes (include/lccrf.h sections 1g and 2g) -------------------------------------------------------------------
    def set_normalization(self, k, mode):
        """Where term k applies its norm: NORMALIZE_AFTER (the reference, the default), _BEFORE, _SYMMETRIC or _NONE."""
        _check(self._c("set_pairwise_normalization")(self.h, int(k), int(mode)))

    def get_normalization(self, k):
        mode = C.c_int(0)
        _check(self._c("get_pairwise_normalization")(self.h, int(k), C.byref(mode)))
        return mode.value

    # -- what the two-label step does for the lattices now in HBM -------------------------------------------------------------------
    def splat_plan(self, k):
        """How the two-label step splats term k for the lattices now in HBM (lccrf_splat_plan): dict(passes, halo, window, lanes,
        vertices_per_lane, long_mode)."""
        p = SplatPlan()
        _check(self._c("get_splat_plan")(self.h, int(k), C.byref(p)))
        return p.as_dict()

    def blur_plan(self, k):
        """Which way the d + 1 blur passes of term k go in the two-label step for the lattices now in HBM (lccrf_blur_plan): dict(in_splat,
        paired_table, paired_plain, alone_32bit, alone_compact, in_slice, nontemporal, first_table_pair)."""
        p = BlurPlan()
        _check(self._c("get_blur_plan")(self.h, int(k), C.byref(p)))
        return p.as_dict()


class DenseCRFHIP(_Handle):
    """Mirror of DenseCRF3D<M> + PottsPotential3D<M,F> (densecrf3d.h, pairwise3d.h) on the
    HIP path.  Same method meaning and call order as the reference; host arrays in/out."""
    _PREFIX = "lccrf_"

    def __init__(self, N, L, device=0):
        self.N, self.L = int(N), int(L)
        self._d = []
        self.h = C.c_void_p()
        _check(lib().lccrf_create(C.byref(self.h), int(device), self.N, self.L))

    # -- unary -------------------------------------------------------------------------
    def set_unary(self, unary):
        u = _f32(unary).reshape(-1)
        if u.size != self.N * self.L:
            raise ValueError("unary must have N*L entries")
        _check(lib().lccrf_set_unary(self.h, _p(u, _f32p)))

    def set_unary_from_label(self, label, conf):
        lab = np.ascontiguousarray(label, np.int16)
        if lab.size != self.N:
            raise ValueError("label must have N entries")
        cf = _f32(np.broadcast_to(np.asarray(conf, np.float32), (self.L,)))
        _check(lib().lccrf_set_unary_from_label(self.h, _p(lab, _i16p), _p(cf, _f32p)))

    # -- pairwise ----------------------------------------------------------------------
    def add_pairwise(self, features, w):
        f = _f32(features)
        f = f.reshape(self.N, f.shape[-1] if f.ndim == 2 else -1)
        _check(lib().lccrf_add_pairwise(self.h, _p(f, _f32p), f.shape[1], float(w)))
        self._d.append(f.shape[1])

    def add_appearance_kernel(self, w, vobserv, verror, sd_observ, sd_error):
        a, b = _f32(vobserv), _f32(verror)
        _check(lib().lccrf_add_appearance_kernel(self.h, float(w), _p(a, _f32p), _p(b, _f32p),
                                                 float(sd_observ), float(sd_error)))
        self._d.append(2)

    def add_smooth_kernel(self, w, xy, sd2d):
        a = _f32(xy)
        _check(lib().lccrf_add_smooth_kernel(self.h, float(w), _p(a, _f32p), float(sd2d)))
        self._d.append(2)

    # -- inference ---------------------------------------------------------------------
    def start_inference(self):
        _check(lib().lccrf_start_inference(self.h))

    def step_inference(self, relax=1.0):
        _check(lib().lccrf_step_inference(self.h, float(relax)))

    def build_map(self):
        _check(lib().lccrf_build_map(self.h))

    def inference(self, n_iter, with_map=False, relax=1.0):
        _check(lib().lccrf_inference(self.h, int(n_iter), int(bool(with_map)), float(relax)))

    inference_native = inference

    def inference_converged(self, max_iterations, criterion=STOP_LABELS, tol=0.0, with_map=False, relax=1.0):
        """Mean-field iterations until every condition of `criterion` holds (STOP_DELTA: max |Q_t - Q_t-1| <= tol, STOP_LABELS: no
        MAP label changed), at most max_iterations (include/lccrf.h section 1h).  Returns convergence()."""
        _check(lib().lccrf_inference_converged(self.h, int(max_iterations), int(criterion), float(tol), int(bool(with_map)),
                                               float(relax)))
        return self.convergence()

    def run_converged(self, max_iterations, criterion=STOP_LABELS, tol=0.0, with_map=False, relax=1.0):
        """inference_converged() from inputs alone (include/lccrf.h section 1i): a fresh frame is built, normalised and inferred
        until converged in ONE launch.  Asynchronous: map() right behind it takes the labels as they arrive, convergence() the
        report."""
        _check(lib().lccrf_run_converged(self.h, int(max_iterations), int(criterion), float(tol), int(bool(with_map)), float(relax)))

    def convergence(self):
        """dict(iterations, delta (np.float32), changed, converged) of the last inference_converged() / run_converged()."""
        it, ch, cv, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        _check(lib().lccrf_get_convergence(self.h, C.byref(it), C.byref(d), C.byref(ch), C.byref(cv)))
        return dict(iterations=it.value, delta=np.float32(d.value), changed=ch.value, converged=cv.value)

    def run_trace(self, n_iter, relax=1.0):
        out = np.empty((n_iter + 1, self.N, self.L), np.float32)
        self.start_inference()
        out[0] = self.probability()
        for t in range(n_iter):
            self.step_inference(relax)
            out[t + 1] = self.probability()
        return out

    # -- the reference's plug-in points (densecrf_base.h:18,34-36) on host arrays ------------
    def apply(self, k, out, x):
        """PairwisePotential::apply of kernel k: returns out + w * norm * compute(x)."""
        o = _f32(out).reshape(self.N, self.L).copy()
        xin = _f32(x).reshape(self.N, self.L)
        _check(lib().lccrf_pairwise_apply(self.h, int(k), _p(o, _f32p), _p(xin, _f32p)))
        return o

    def exp_and_normalize(self, x, scale=1.0, relax=1.0, old=None):
        xin = _f32(x).reshape(self.N, self.L)
        o = np.zeros_like(xin) if old is None else _f32(old).reshape(self.N, self.L).copy()
        _check(lib().lccrf_exp_and_normalize(self.h, _p(o, _f32p), _p(xin, _f32p), float(scale), float(relax)))
        return o

    def step_init(self):
        o = np.empty((self.N, self.L), np.float32)
        _check(lib().lccrf_step_init(self.h, _p(o, _f32p)))
        return o

    def map_of(self, prob):
        p = _f32(prob).reshape(self.N, self.L)
        m = np.empty(self.N, np.int16)
        _check(lib().lccrf_map_of(self.h, _p(p, _f32p), _p(m, _i16p)))
        return m

    # -- device arrays (include/lccrf.h section 1b) ---------------------------------------
    # Pointers are raw device addresses (e.g. torch_tensor.data_ptr()), read and written in order on the handle's stream
    # (stream()); work on another stream that produces them must be ordered before it by the caller (an event, or
    # torch.cuda.ExternalStream(h.stream()).wait_stream(producer)).
    def stream(self):
        """The handle's own stream (a hipStream_t address)."""
        s = C.c_void_p()
        _check(lib().lccrf_get_stream(self.h, C.byref(s)))
        return s.value or 0

    def synchronize(self):
        _check(lib().lccrf_synchronize(self.h))

    def set_unary_device(self, d_unary):
        _check(lib().lccrf_set_unary_device(self.h, C.c_void_p(d_unary)))

    def set_unary_from_label_device(self, d_label, conf):
        cf = _f32(np.broadcast_to(np.asarray(conf, np.float32), (self.L,)))
        _check(lib().lccrf_set_unary_from_label_device(self.h, C.c_void_p(d_label), _p(cf, _f32p)))

    def add_pairwise_device(self, d_features, d, w):
        _check(lib().lccrf_add_pairwise_device(self.h, C.c_void_p(d_features), int(d), float(w)))
        self._d.append(int(d))

    def add_image_kernel(self, width, height, w, posdev, d_image=None, image_format=IMAGE_NONE, featuredev=0.0):
        """PottsPotentialCPU<M,F>::FromImage with the image (uint8 or float RGB, HWC) on the device."""
        _check(lib().lccrf_add_image_kernel(self.h, int(width), int(height), float(w), float(posdev),
                                            _addr(d_image), int(image_format), float(featuredev)))
        self._d.append(2 if image_format == IMAGE_NONE else 5)

    def device_buffers(self):
        """Addresses of the handle-owned HBM arrays: unary, current (Q), next, tmp, map.  Moves the labels to HBM."""
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().lccrf_device_buffers(self.h, *[C.byref(x) for x in p]))
        return dict(zip(("unary", "current", "next", "tmp", "map"), (x.value for x in p)))

    def pairwise_apply_device(self, k, d_out, d_in):
        _check(lib().lccrf_pairwise_apply_device(self.h, int(k), C.c_void_p(d_out), C.c_void_p(d_in)))

    def exp_and_normalize_device(self, d_out, d_in, scale=1.0, relax=1.0):
        _check(lib().lccrf_exp_and_normalize_device(self.h, C.c_void_p(d_out), C.c_void_p(d_in), float(scale), float(relax)))

    def step_init_device(self, d_next):
        _check(lib().lccrf_step_init_device(self.h, C.c_void_p(d_next)))

    def map_of_device(self, d_prob, d_map):
        _check(lib().lccrf_map_of_device(self.h, C.c_void_p(d_prob), C.c_void_p(d_map)))

    # -- gradients of inference() (include/lccrf.h section 1c; the torch layer: autograd.py) ----------------------------------
    def inference_backward_device(self, n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights=None):
        """dL/dU [N][L] and dL/dw [K] of inference(n_iterations, relax) from dL/dQ [N][L]; device addresses, on stream()."""
        _check(lib().lccrf_inference_backward(self.h, int(n_iterations), float(relax), _addr(d_grad_prob), _addr(d_grad_unary),
                                              _addr(d_grad_weights)))

    def inference_backward_features_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                           d_grad_features=None):
        """inference_backward_device plus dL/d features: d_grad_features is a list of K device addresses ([N][d_k] each) or None
        entries (that term is skipped); d_grad_unary / d_grad_weights may be None (include/lccrf.h section 1d)."""
        _check(lib().lccrf_inference_backward_features(self.h, int(n_iterations), float(relax), _addr(d_grad_prob),
                                                       _addr(d_grad_unary), _addr(d_grad_weights), _addr_list(d_grad_features)))

    # -- ... with respect to the label-compatibility matrices (include/lccrf.h section 1e) -------------------------------------
    def inference_backward_compat_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                         d_grad_compat=None):
        """inference_backward_device plus dL/dmu: d_grad_compat is the device address of a [K][L][L] array (None: the call is
        inference_backward_device); d_grad_unary / d_grad_weights may then be None."""
        _check(lib().lccrf_inference_backward_compat(self.h, int(n_iterations), float(relax), _addr(d_grad_prob),
                                                     _addr(d_grad_unary), _addr(d_grad_weights), _addr(d_grad_compat)))

    # -- features and matrices in one sweep (include/lccrf.h section 1f) ----------------------------------------------------------
    def inference_backward_all_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                      d_grad_features=None, d_grad_compat=None):
        """inference_backward_device plus dL/d features and dL/dmu of the forward with the handle's matrices: d_grad_features as
        inference_backward_features_device takes it, d_grad_compat as inference_backward_compat_device; any output may be None."""
        _check(lib().lccrf_inference_backward_all(self.h, int(n_iterations), float(relax), _addr(d_grad_prob), _addr(d_grad_unary),
                                                  _addr(d_grad_weights), _addr_list(d_grad_features), _addr(d_grad_compat)))

    # -- ... and under every normalisation mode (include/lccrf.h section 1m) ------------------------------------------------------
    def inference_backward_modes_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                        d_grad_features=None, d_grad_compat=None):
        """inference_backward_all_device without its refusal of feature gradients on a handle with a term that is not normalised
        AFTER: the norm's factors are differentiated in the features too.  With every term AFTER it is that call."""
        _check(lib().lccrf_inference_backward_modes(self.h, int(n_iterations), float(relax), _addr(d_grad_prob), _addr(d_grad_unary),
                                                    _addr(d_grad_weights), _addr_list(d_grad_features), _addr(d_grad_compat)))

    # -- results -----------------------------------------------------------------------
    def map(self):
        out = np.empty(self.N, np.int16)
        _check(lib().lccrf_get_map(self.h, _p(out, _i16p)))
        return out

    def probability(self):
        out = np.empty((self.N, self.L), np.float32)
        _check(lib().lccrf_get_probability(self.h, _p(out, _f32p)))
        return out

    def engine(self):
        """(engine, shape) of the last inference(): 1 streaming, 2 fused, 3 one launch per frame, 4 the fused engine's kernel for
        terms with a matrix or a normalisation mode, 5 its kernel for three to eight labels (OPT_FUSED_MULTILABEL), 6 that
        kernel's form for a learnt model (MULTILABEL_LEARNT); shape (engines 2, 4, 5 and 6, else 0): lanes per workgroup | points per lane << 16 |
        first term on chain rows << 20.  Report only (include/lccrf.h: lccrf_get_engine)."""
        e, s = C.c_int(0), C.c_int(0)
        _check(lib().lccrf_get_engine(self.h, C.byref(e), C.byref(s)))
        return e.value, s.value

    def backward_route(self):
        """the route of the last successful backward call: BACKWARD_NONE, BACKWARD_STREAM or BACKWARD_FUSED (OPT_FUSED_BACKWARD).
        Report only (include/lccrf.h section 1j)."""
        r = C.c_int(0)
        _check(lib().lccrf_get_backward_route(self.h, C.byref(r)))
        return r.value

    def unary(self):
        out = np.empty((self.N, self.L), np.float32)
        _check(lib().lccrf_get_unary(self.h, _p(out, _f32p)))
        return out

    def build_report(self, k):
        """What the build kernels counted while they built term k's lattice now in HBM (lccrf_build_report), as a dict."""
        r = BuildReport()
        _check(lib().lccrf_get_build_report(self.h, int(k), C.byref(r)))
        return r.as_dict()

    def kernel(self, k):
        d = self._d[k]
        V = C.c_int(0)
        _check(lib().lccrf_get_lattice_size(self.h, k, C.byref(V)))
        V = V.value
        norm = np.empty(self.N, np.float32)
        off = np.empty((self.N, d + 1), np.int32)
        bary = np.empty((self.N, d + 1), np.float32)
        nbr = np.empty((d + 1, V, 2), np.int32)
        _check(lib().lccrf_get_norm(self.h, k, _p(norm, _f32p)))
        _check(lib().lccrf_get_lattice(self.h, k, _p(off, _i32p), _p(bary, _f32p), _p(nbr, _i32p)))
        return dict(d=d, V=V, norm=norm, offset=off, bary=bary, nbr=nbr)


class BatchCRF(_Handle):
    """Frames-in-flight: F independent CRFs with a common stride (include/lccrf.h section 2)."""
    _PREFIX = "lccrf_batch_"

    def __init__(self, max_frames, max_points, n_labels, feat_dims, weights, device=0):
        self.F, self.maxN, self.L = int(max_frames), int(max_points), int(n_labels)
        self.dims = [int(d) for d in feat_dims]
        if len(self.dims) > MAX_KERNELS:
            raise LccrfError(-1, "%d pairwise kernels: at most %d" % (len(self.dims), MAX_KERNELS))
        d = BatchDesc()
        d.max_frames, d.max_points, d.n_labels, d.n_kernels = self.F, self.maxN, self.L, len(self.dims)
        for i, (fd, w) in enumerate(zip(self.dims, weights)):
            d.feat_dims[i] = fd
            d.weights[i] = float(w)
        self.h = C.c_void_p()
        self.n_frames, self.n_points = 0, None        # n_points: the host counts of the inputs bound, when they came from the host
        self.inputs_serial = 0                        # counts the calls that gave the batch inputs: who bound last can tell (autograd.py)
        _check(lib().lccrf_batch_create(C.byref(self.h), int(device), C.byref(d)))
        self._keep = None

    def set_inputs_host(self, n_points, features, unary=None, label=None, conf=None):
        npts = np.ascontiguousarray(n_points, np.int32)
        F = npts.size
        feats = [_f32(f).reshape(F, self.maxN, d) for f, d in zip(features, self.dims)]
        arr = (_f32p * len(feats))(*[_p(f, _f32p) for f in feats])
        u = l = cf = None
        if unary is not None:
            u = _f32(unary).reshape(F, self.maxN, self.L)
        if label is not None:
            l = np.ascontiguousarray(label, np.int16).reshape(F, self.maxN)
            cf = _f32(np.broadcast_to(np.asarray(conf, np.float32), (self.L,)))
        _check(lib().lccrf_batch_set_inputs_host(
            self.h, F, _p(npts, _i32p), _p(u, _f32p) if u is not None else None,
            _p(l, _i16p) if l is not None else None, _p(cf, _f32p) if cf is not None else None, arr))
        self.n_frames, self.n_points = F, npts.copy()
        self.inputs_serial += 1

    HOST_PINNED = 1
    DOWNLOAD_LABEL_BITS, DOWNLOAD_MAP, DOWNLOAD_PROBABILITY = 1, 2, 4
    OPT_COPY_THREADS = 3
    OPT_EVENT_TIMING = 4
    OPT_FRAME_GENERAL = 5
    OPT_FUSED_BACKWARD = 6
    OPT_FUSED_BACKWARD_LEARNT = 7
    OPT_FUSED_BACKWARD_FEATURES = 8
    OPT_FUSED_MULTILABEL = 9
    MULTILABEL_POTTS, MULTILABEL_LEARNT = 1, 2

    def set_inputs_host_async(self, n_points, features, unary=None, label=None, conf=None, pinned=False):
        """lccrf_batch_set_inputs_host_async: the arrays are staged and uploaded without a host wait.  The arrays must already be
        C-contiguous of the right dtype (nothing is converted here: a hidden copy would be timed as part of the call); with
        pinned=True they must live in pinned memory and stay untouched until wait_inputs() or a result of this batch."""
        npts = np.ascontiguousarray(n_points, np.int32)
        F = npts.size

        def addr(a, dtype, count):
            assert a.dtype == dtype and a.flags["C_CONTIGUOUS"] and a.size == count, (a.dtype, a.shape, count)
            return C.c_void_p(a.ctypes.data)
        arr = (C.c_void_p * len(features))(*[addr(f, np.float32, F * self.maxN * d) for f, d in zip(features, self.dims)])
        u = l = cf = None
        if unary is not None:
            u = addr(unary, np.float32, F * self.maxN * self.L)
        if label is not None:
            l = addr(label, np.int16, F * self.maxN)
            cf = _f32(np.broadcast_to(np.asarray(conf, np.float32), (self.L,)))
        _check(lib().lccrf_batch_set_inputs_host_async(
            self.h, F, C.c_void_p(npts.ctypes.data), u, l, _p(cf, _f32p) if cf is not None else None, arr,
            self.HOST_PINNED if pinned else 0))
        self.n_frames, self.n_points = F, npts.copy()
        self.inputs_serial += 1

    def wait_inputs(self):
        _check(lib().lccrf_batch_wait_inputs(self.h))

    def download_async(self, what=1):
        _check(lib().lccrf_batch_download_async(self.h, int(what)))

    def wait_download(self, copy=True):
        """-> dict with the arrays that were asked for ('bits' uint64 [F][words], 'map' int16 [F][maxN], 'prob' float32 [F][maxN][L]);
        copy=False hands out views of the batch's pinned memory (valid until the next download_async)."""
        bits, mp, pr, words = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        _check(lib().lccrf_batch_wait_download(self.h, C.byref(bits), C.byref(words), C.byref(mp), C.byref(pr)))
        out, F = {}, self.n_frames

        def view(ptr, ctype, shape, dtype):
            n = int(np.prod(shape))
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (max(n, 1),))[:n].reshape(shape).view(dtype)
            return a.copy() if copy else a
        if bits.value:
            out["bits"] = view(bits, C.c_uint64, (F, words.value), np.uint64)
        if mp.value:
            out["map"] = view(mp, C.c_int16, (F, self.maxN), np.int16)
        if pr.value:
            out["prob"] = view(pr, C.c_float, (F, self.maxN, self.L), np.float32)
        return out

    def bind_inputs_device(self, n_frames, d_n_points, d_features, d_unary=None, d_label=None, conf=None):
        """Pointers are raw device addresses (e.g. torch_tensor.data_ptr())."""
        arr = (C.c_void_p * len(d_features))(*[C.c_void_p(int(p)) for p in d_features])
        cf = None
        if d_label is not None:
            cf = _f32(np.broadcast_to(np.asarray(conf, np.float32), (self.L,)))
        _check(lib().lccrf_batch_bind_inputs_device(
            self.h, int(n_frames), C.c_void_p(int(d_n_points)), _addr(d_unary), _addr(d_label),
            _p(cf, _f32p) if cf is not None else None, arr))
        self.n_frames, self.n_points = int(n_frames), None        # (the counts live on the device)
        self.inputs_serial += 1

    def build(self, stream=None):
        _check(lib().lccrf_batch_build(self.h, _addr(stream)))

    def inference(self, n_iter, with_map=True, relax=1.0, stream=None):
        _check(lib().lccrf_batch_inference(self.h, int(n_iter), int(bool(with_map)), float(relax), _addr(stream)))

    def inference_converged(self, max_iterations, criterion=STOP_LABELS, tol=0.0, with_map=True, relax=1.0, stream=None):
        """Every frame iterated until ITS criterion holds, at most max_iterations, on built lattices (include/lccrf.h section 2e);
        asynchronous like inference()."""
        _check(lib().lccrf_batch_inference_converged(self.h, int(max_iterations), int(criterion), float(tol), int(bool(with_map)),
                                                     float(relax), _addr(stream)))

    def run_converged(self, max_iterations, criterion=STOP_LABELS, tol=0.0, with_map=True, relax=1.0, stream=None):
        """run() with inference_converged()'s stop rule (include/lccrf.h section 2f): from inputs alone, every frame built and
        inferred until ITS criterion holds in one launch; asynchronous like run()."""
        _check(lib().lccrf_batch_run_converged(self.h, int(max_iterations), int(criterion), float(tol), int(bool(with_map)),
                                               float(relax), _addr(stream)))

    def convergence(self):
        """dict of [n_frames] arrays: iterations, delta, changed, converged of the last inference_converged() / run_converged()
        (waits for the batch)."""
        F = self.n_frames
        it, ch, cv = (np.zeros(F, np.int32) for _ in range(3))
        d = np.zeros(F, np.float32)
        _check(lib().lccrf_batch_get_convergence_host(self.h, _p(it, _i32p), _p(d, _f32p), _p(ch, _i32p), _p(cv, _i32p)))
        return dict(iterations=it, delta=d, changed=ch, converged=cv)

    def device_convergence(self):
        """device addresses of the four [max_frames] arrays: iterations (int32), delta (float32), changed (int32), converged (int32)"""
        p = [C.c_void_p() for _ in range(4)]
        _check(lib().lccrf_batch_device_convergence(self.h, *[C.byref(x) for x in p]))
        return dict(zip(("iterations", "delta", "changed", "converged"), (x.value for x in p)))

    def run(self, n_iter, with_map=True, relax=1.0, stream=None):
        """Lattice build + normalisation + inference of every frame in one launch (lccrf_batch_run)."""
        _check(lib().lccrf_batch_run(self.h, int(n_iter), int(bool(with_map)), float(relax), _addr(stream)))

    def synchronize(self):
        _check(lib().lccrf_batch_synchronize(self.h))

    def set_unary_device(self, d_unary):
        """Unaries [n_frames][max_points][L] of the frames now bound, copied from a device address on the batch's stream."""
        _check(lib().lccrf_batch_set_unary_device(self.h, C.c_void_p(int(d_unary))))

    def inference_backward_device(self, n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights=None, stream=None):
        """Per frame dL/dU [n_frames][max_points][L] and dL/dw [n_frames][K] of inference(n_iterations, relax) from dL/dQ
        [n_frames][max_points][L]; device addresses (include/lccrf.h section 2c)."""
        _check(lib().lccrf_batch_inference_backward(self.h, int(n_iterations), float(relax), C.c_void_p(int(d_grad_prob)),
                                                    C.c_void_p(int(d_grad_unary)), _addr(d_grad_weights), _addr(stream)))

    def inference_backward_converged_device(self, max_iterations, relax, d_iterations, d_grad_prob, d_grad_unary, d_grad_weights=None,
                                            stream=None):
        """inference_backward_device with every frame at its own iteration count (include/lccrf.h section 2j): d_iterations is the
        device address of [n_frames] int32 -- device_convergence()["iterations"] behind inference_converged(), or a copy of it --
        clamped per frame to [0, max_iterations] by the kernels and never read by the host."""
        _check(lib().lccrf_batch_inference_backward_converged(self.h, int(max_iterations), float(relax), _addr(d_iterations),
                                                              C.c_void_p(int(d_grad_prob)), C.c_void_p(int(d_grad_unary)),
                                                              _addr(d_grad_weights), _addr(stream)))

    def inference_backward_features_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                           d_grad_features=None, stream=None):
        """inference_backward_device plus dL/d features: d_grad_features is a list of K device addresses
        ([n_frames][max_points][d_k] each) or None entries (include/lccrf.h section 2d)."""
        _check(lib().lccrf_batch_inference_backward_features(self.h, int(n_iterations), float(relax), C.c_void_p(int(d_grad_prob)),
                                                             _addr(d_grad_unary), _addr(d_grad_weights), _addr_list(d_grad_features),
                                                             _addr(stream)))

    def inference_backward_all_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                      d_grad_features=None, d_grad_compat=None, d_grad_model=None, stream=None):
        """The gradients of a batch with or without matrices and modes (include/lccrf.h section 2h): per frame dL/dU, dL/dw [F][K],
        dL/d features (a list of K device addresses or None entries) and dL/dmu [F][K][L][L], and d_grad_model [K + K*L*L], the
        sums over the frames of dL/dw and dL/dmu in ascending frame order; device addresses, any output may be None."""
        _check(lib().lccrf_batch_inference_backward_all(self.h, int(n_iterations), float(relax), C.c_void_p(int(d_grad_prob)),
                                                        _addr(d_grad_unary), _addr(d_grad_weights), _addr_list(d_grad_features),
                                                        _addr(d_grad_compat), _addr(d_grad_model), _addr(stream)))

    def inference_backward_all_converged_device(self, max_iterations, relax, d_iterations, d_grad_prob, d_grad_unary=None,
                                                d_grad_weights=None, d_grad_compat=None, d_grad_model=None, stream=None):
        """inference_backward_all_device without feature gradients, every frame at its own iteration count (include/lccrf.h section
        2k): d_iterations as inference_backward_converged_device takes it -- device_convergence()["iterations"] behind
        inference_converged(), or a copy of it, clamped per frame to [0, max_iterations] and never read by the host."""
        _check(lib().lccrf_batch_inference_backward_all_converged(self.h, int(max_iterations), float(relax), _addr(d_iterations),
                                                                  _addr(d_grad_prob), _addr(d_grad_unary), _addr(d_grad_weights),
                                                                  _addr(d_grad_compat), _addr(d_grad_model), _addr(stream)))

    def inference_backward_modes_device(self, n_iterations, relax, d_grad_prob, d_grad_unary=None, d_grad_weights=None,
                                        d_grad_features=None, d_grad_compat=None, d_grad_model=None, stream=None):
        """inference_backward_all_device with the feature gradients of terms in any normalisation mode (include/lccrf.h section 2i);
        with every term AFTER it is that call."""
        _check(lib().lccrf_batch_inference_backward_modes(self.h, int(n_iterations), float(relax), C.c_void_p(int(d_grad_prob)),
                                                          _addr(d_grad_unary), _addr(d_grad_weights), _addr_list(d_grad_features),
                                                          _addr(d_grad_compat), _addr(d_grad_model), _addr(stream)))

    def inference_backward_modes_converged_device(self, max_iterations, relax, d_iterations, d_grad_prob, d_grad_unary=None,
                                                  d_grad_weights=None, d_grad_features=None, d_grad_compat=None, d_grad_model=None,
                                                  stream=None):
        """inference_backward_modes_device with every frame at its own iteration count (include/lccrf.h section 2l): d_iterations as
        inference_backward_converged_device takes it -- device_convergence()["iterations"] behind inference_converged(), or a copy of
        it, clamped per frame to [0, max_iterations] and never read by the host.  Without a feature array it is
        inference_backward_all_converged_device."""
        _check(lib().lccrf_batch_inference_backward_modes_converged(self.h, int(max_iterations), float(relax), _addr(d_iterations),
                                                                    _addr(d_grad_prob), _addr(d_grad_unary), _addr(d_grad_weights),
                                                                    _addr_list(d_grad_features), _addr(d_grad_compat),
                                                                    _addr(d_grad_model), _addr(stream)))

    pairwise_compatibility, normalization = _Handle.get_pairwise_compatibility, _Handle.get_normalization   # (the batch's own names)

    def set_engine(self, engine):
        _check(lib().lccrf_batch_set_engine(self.h, int(engine)))

    def engine(self):
        e = C.c_int(0)
        _check(lib().lccrf_batch_get_engine(self.h, C.byref(e)))
        return e.value

    def backward_route(self):
        """the route of the last successful backward call: BACKWARD_NONE, BACKWARD_STREAM or BACKWARD_FUSED (OPT_FUSED_BACKWARD)"""
        r = C.c_int(0)
        _check(lib().lccrf_batch_get_backward_route(self.h, C.byref(r)))
        return r.value

    def fused_shape(self):
        """(lanes per frame, frames per CU) of the last fused-engine launch; (0, 0) if there was none."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().lccrf_batch_get_fused_shape(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def locality_mode(self):
        """(internal point order in use, sorted build in use) for the lattices now in HBM."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().lccrf_batch_get_locality_mode(self.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def build_report(self, k, frame=0):
        """What the build kernels counted while they built the lattice of term k, frame `frame`, now in HBM (lccrf_build_report), as a
        dict; all 0 for lattices of the one-workgroup build."""
        r = BuildReport()
        _check(lib().lccrf_batch_get_build_report(self.h, int(k), int(frame), C.byref(r)))
        return r.as_dict()

    def built_lattice(self, k, frame=0):
        """Parity probe: the tables of term k, frame `frame` as built, in the engine's internal order and numbering, without a rebuild
        (lccrf_batch_get_built_lattice): dict(N, V, perm, offset, bary, rowptr, csr_pt, csr_w, nbr, fastn or None)."""
        d = self.dims[k]
        npad, nv, has = C.c_int32(0), C.c_int32(0), C.c_int(0)
        fn = lib().lccrf_batch_get_built_lattice
        _check(fn(self.h, int(k), int(frame), C.byref(npad), C.byref(nv), None, None, None, None, None, None, None, None, C.byref(has)))
        Np, V = npad.value, nv.value
        N = int(self.n_points[frame]) if self.n_points is not None else None
        perm = np.empty(Np, np.int32)
        off = np.empty((Np, d + 1), np.int32)
        bary = np.empty((Np, d + 1), np.float32)
        rowptr = np.empty(V + 1, np.int32)
        nbr = np.empty((d + 1, V, 2), np.int32)
        fastn = np.empty(V, np.uint8)
        _check(fn(self.h, int(k), int(frame), None, None, _p(perm, _i32p), _p(off, _i32p), _p(bary, _f32p), _p(rowptr, _i32p), None, None,
                  _p(nbr, _i32p), fastn.ctypes.data_as(C.POINTER(C.c_uint8)), None))
        nr = int(rowptr[V])                             # (= N (d + 1): the real entries)
        if N is None:
            N = nr // (d + 1)
        csr_pt = np.empty(N * (d + 1), np.int32)
        csr_w = np.empty(N * (d + 1), np.float32)
        _check(fn(self.h, int(k), int(frame), None, None, None, None, None, None, _p(csr_pt, _i32p), _p(csr_w, _f32p), None, None, None))
        return dict(d=d, N=N, V=V, perm=perm, offset=off, bary=bary, rowptr=rowptr, csr_pt=csr_pt, csr_w=csr_w, nbr=nbr,
                    fastn=fastn if has.value else None)

    def fallback_frames(self):
        """Frames of the last run() that did not fit the one-launch kernel and were re-run on the two-kernel path."""
        n = C.c_int(0)
        _check(lib().lccrf_batch_get_fallback_frames(self.h, C.byref(n)))
        return n.value

    def pose_set_crf_counts(self, d_n_total):
        """lccrf_batch_pose_set_crf_counts: device int32[F] of CRF points + extra non-CRF edges per frame (None: off)."""
        _check(lib().lccrf_batch_pose_set_crf_counts(self.h, _addr(d_n_total)))

    def map(self):
        out = np.empty((self.n_frames, self.maxN), np.int16)
        _check(lib().lccrf_batch_get_map_host(self.h, _p(out, _i16p)))
        return out

    def probability(self):
        out = np.empty((self.n_frames, self.maxN, self.L), np.float32)
        _check(lib().lccrf_batch_get_probability_host(self.h, _p(out, _f32p)))
        return out

    def lattice_sizes(self, k):
        out = np.empty(self.n_frames, np.int32)
        _check(lib().lccrf_batch_get_lattice_sizes_host(self.h, k, _p(out, _i32p)))
        return out

    def norm(self, k):
        out = np.empty((self.n_frames, self.maxN), np.float32)
        _check(lib().lccrf_batch_get_norm_host(self.h, k, _p(out, _f32p)))
        return out

    def device_buffers(self):
        m, q = C.c_void_p(), C.c_void_p()
        _check(lib().lccrf_batch_device_buffers(self.h, C.byref(m), C.byref(q)))
        return m.value, q.value

    def device_label_bits(self):
        """(device address, words per frame) of the bit-packed MAP labels (binary CRFs only)."""
        p, w = C.c_void_p(), C.c_int(0)
        _check(lib().lccrf_batch_device_label_bits(self.h, C.byref(p), C.byref(w)))
        return p.value, w.value

    def time_blur_pass(self, kernel=0, reps=50):
        """(ms per launch, vertices per launch) of one blur pass of `kernel` over all frames (streaming engine)."""
        ms, nv = C.c_float(0), C.c_int64(0)
        _check(lib().lccrf_batch_time_blur_pass(self.h, int(kernel), int(reps), C.byref(ms), C.byref(nv)))
        return ms.value, nv.value

    def pose_optimization(self, d_Xw, d_kp, d_u_right, d_inv_sigma2, K4, bf, d_Tcw_in, d_Tcw_out, d_outlier, d_n_inliers,
                          d_n_initial, d_valid=None, stream=None):
        """lccrf_batch_pose_optimization: raw device addresses; consumes the labels of the last inference on the device."""
        K, v = _f32(K4), _addr
        _check(lib().lccrf_batch_pose_optimization(self.h, v(d_Xw), v(d_kp), v(d_u_right), v(d_inv_sigma2), v(d_valid), _p(K, _f32p),
                                                   float(bf), v(d_Tcw_in), v(d_Tcw_out), v(d_outlier), v(d_n_inliers),
                                                   v(d_n_initial), _addr(stream)))

    def last_timing(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().lccrf_batch_last_timing(self.h, C.byref(a), C.byref(b)))
        return dict(inference_ms=a.value, build_ms=b.value)

    def own_stream(self):
        """The batch's own hipStream_t as an integer (what stream=None means): wrap it with torch.cuda.ExternalStream to order torch work behind it."""
        p = C.c_void_p()
        _check(lib().lccrf_batch_get_stream(self.h, C.byref(p)))
        return p.value

    def last_prepare(self):
        """(prepare_ms, runs) of the two-frames-per-CU kernel's prepared launch records (include/lccrf.h: lccrf_batch_last_prepare)."""
        ms, n = C.c_float(0), C.c_int(0)
        _check(lib().lccrf_batch_last_prepare(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def lattice_filter(features, x, device=0):
    """PermutohedralLatticeCPU::init + compute on the GPU (lccrf_lattice_filter): returns (y, V)."""
    f = _f32(features)
    N, d = f.shape
    xa = _f32(x)
    xin = xa.reshape(N, xa.shape[-1] if xa.ndim == 2 else max(xa.size // max(N, 1), 1))
    out = np.empty_like(xin)
    V = C.c_int(0)
    _check(lib().lccrf_lattice_filter(int(device), _p(f, _f32p), N, d, _p(xin, _f32p), xin.shape[1], _p(out, _f32p), C.byref(V)))
    return out, V.value


def pose_optimization(Xw, kp, u_right, inv_sigma2, K4, bf, Tcw, valid=None, label=None, device=0, outlier=None):
    """Optimizer::PoseOptimization on the GPU (lccrf_pose_optimization): (Tcw_out [4,4], outlier u8[n], n_inliers).
    `outlier`: what mvbOutlier holds before the call (default zeros); entries of points without an edge come back as given."""
    Xw, kp = _f32(Xw).reshape(-1, 3), _f32(kp).reshape(-1, 2)
    n = Xw.shape[0]
    ur, is2, K, T = _f32(u_right), _f32(inv_sigma2), _f32(K4), _f32(Tcw).reshape(16)
    va = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    la = None if label is None else np.ascontiguousarray(label, np.int16)
    out = np.empty(16, np.float32)
    outl = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n)
    ninl = np.zeros(1, np.int32)
    _check(lib().lccrf_pose_optimization(int(device), n, _p(Xw, _f32p), _p(kp, _f32p), _p(ur, _f32p), _p(is2, _f32p),
                                         va.ctypes.data if va is not None else None, _p(la, _i16p) if la is not None else None,
                                         _p(K, _f32p), float(bf), _p(T, _f32p), _p(out, _f32p), outl.ctypes.data, _p(ninl, _i32p)))
    return out.reshape(4, 4), outl, int(ninl[0])


def default_params():
    p = CrfParams()
    lib().lccrf_default_params(C.byref(p))
    return p


def unary_build(Xw, obs_ptr, obs_kf, obs_kp, kf_pose, kf_intr, kf_bounds, match_prob=None, params=None, device=0):
    """ComputeMapPointErrAndObserv + RroughClassify for a whole frame on the GPU
    (src/Tracking.cc:1803-1839, 1961-2013; include/lccrf.h section 3)."""
    if params is None:
        params = default_params()
    Xw = _f32(Xw).reshape(-1, 3)
    n = Xw.shape[0]
    ptr = np.ascontiguousarray(obs_ptr, np.int32)
    kf = np.ascontiguousarray(obs_kf, np.int32)
    kp = np.ascontiguousarray(obs_kp, np.float64).reshape(-1, 2)
    pose, intr, bnd = _f32(kf_pose).reshape(-1, 12), _f32(kf_intr).reshape(-1, 4), _f32(kf_bounds).reshape(-1, 4)
    mp = None
    if match_prob is not None:
        match_prob = np.ascontiguousarray(match_prob, np.float64)
        mp = match_prob.ctypes.data_as(C.POINTER(C.c_double))
    obs, err, dep = (np.empty(n, np.float32) for _ in range(3))
    lab = np.empty(n, np.int16)
    _check(lib().lccrf_unary_build(int(device), n, _p(Xw, _f32p), _p(ptr, _i32p), _p(kf, _i32p),
                                   kp.ctypes.data_as(C.POINTER(C.c_double)), pose.shape[0], _p(pose, _f32p),
                                   _p(intr, _f32p), _p(bnd, _f32p), mp, C.byref(params), _p(obs, _f32p),
                                   _p(err, _f32p), _p(dep, _f32p), _p(lab, _i16p)))
    return obs, err, dep, lab


def bf_match(desc_query, desc_train, ratio=0.6, device=0):
    """Tracking::BfMatch on the GPU (src/Tracking.cc:1747-1766; include/lccrf.h section 4):
    train index per query or -1, and the number of matches."""
    q = np.ascontiguousarray(desc_query, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(desc_train, np.uint8).reshape(-1, 32)
    out = np.empty(q.shape[0], np.int32)
    nm = np.zeros(1, np.int32)
    _check(lib().lccrf_bf_match(int(device), q.shape[0], q.ctypes.data, t.shape[0], t.ctypes.data, float(ratio),
                                _p(out, _i32p), _p(nm, _i32p)))
    return out, int(nm[0])

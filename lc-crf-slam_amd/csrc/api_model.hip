// api_model.hip -- the entry points a handle and a batch share word for word: the terms' weights (sections 1c / 2c of include/lccrf.h),
// label-compatibility matrices (1e / 2g) and normalisation modes (1g / 2g), the backward route (1j), the splat and blur plans and the
// one-launch routes of frames of three to eight labels (lccrf_set_multilabel_routes).
//
// One body per entry point, on the Engine (host_engine.h); below them the two extern "C" forms of each, side by side: the checks in
// the form's own order, then the body.  Every setter settles a pending one-launch run first (it may still be re-run: with the model
// it was asked with) and touches no lattice, norm or prepared launch record.
#include "api_common.h"

#include <cmath>

using namespace lccrf;

// The orders of the checks.  A handle's form looks at the handle first, and so do a batch's forms of section 2c and of the plans.  A
// batch's forms of section 2g check first what needs no batch -- a mode outside 0 .. 3, a kernel index no batch can have, a NULL
// output -- so those answers need no device.
#define HANDLE_FIRST(h, k) CHECK_H(h); CHECK_K(h, k)
#define INDEX_FIRST(b, k) CHECK_K_ANY(k); CHECK_H(b); CHECK_K(b, k)
#define CHECK_MODE(mode)                                                 \
    if ((mode) < LCCRF_NORMALIZE_AFTER || (mode) > LCCRF_NORMALIZE_NONE) \
    return fail(LCCRF_E_INVALID, "normalization mode %d is none of LCCRF_NORMALIZE_AFTER / _BEFORE / _SYMMETRIC / _NONE", (mode))
#define CHECK_OUT(p, name) if (!(p)) return fail(LCCRF_E_INVALID, name " is NULL")

namespace {

int set_weight(Engine &e, int kernel, float w)
{
    if (int rl = e.resolve_late()) return rl;
    e.set_weight(kernel, w);
    return LCCRF_OK;
}

int set_matrix(Engine &e, int kernel, const float *compat)
{
    for (int i = 0; compat && i < e.L * e.L; ++i)
        if (!std::isfinite(compat[i])) return fail(LCCRF_E_INVALID, "compat[%d][%d] is not finite", i / e.L, i % e.L);
    if (int rl = e.resolve_late()) return rl;
    return e.model.set_matrix(e, kernel, compat);
}

int get_matrix(const Engine &e, int kernel, float *compat_out, int *is_set)
{
    const bool set = e.model.has_matrix(kernel);
    if (is_set) *is_set = set ? 1 : 0;
    for (int i = 0; compat_out && i < e.L * e.L; ++i)     // (a Potts term reads as the identity it is)
        compat_out[i] = set ? e.model.matrix(kernel)[i] : (i / e.L == i % e.L ? 1.0f : 0.0f);
    return LCCRF_OK;
}

int set_mode(Engine &e, int kernel, int mode)
{
    if (int rl = e.resolve_late()) return rl;
    e.model.set_mode(e, kernel, mode);
    return LCCRF_OK;
}

int get_mode(const Engine &e, int kernel, int *mode)
{
    *mode = e.model.mode(kernel);
    return LCCRF_OK;
}

// (report only: no device is selected, nothing is settled)
int get_route(const Engine *e, int *route)
{
    if (!e || !route) return fail(LCCRF_E_INVALID, "handle / route is NULL");
    *route = e->report.backward_route;
    return LCCRF_OK;
}

// The one-launch routes of frames of three to eight labels: bit 0 IS Options::fused_multilabel (LCCRF_OPT_FUSED_MULTILABEL), bit 1
// Options::fused_multilabel_learnt.  Like lccrf_set_option: no device is selected, nothing is settled; the next inference decides.
constexpr unsigned kMultilabelRoutes = LCCRF_MULTILABEL_POTTS | LCCRF_MULTILABEL_LEARNT;
int set_routes(Engine *e, unsigned routes)
{
    if (!e) return fail(LCCRF_E_INVALID, "handle is NULL");
    if (routes & ~kMultilabelRoutes)
        return fail(LCCRF_E_INVALID, "routes 0x%x has bits beyond LCCRF_MULTILABEL_POTTS | LCCRF_MULTILABEL_LEARNT", routes);
    e->opt.fused_multilabel = (routes & LCCRF_MULTILABEL_POTTS) != 0;
    e->opt.fused_multilabel_learnt = (routes & LCCRF_MULTILABEL_LEARNT) != 0;
    e->choose_sized_engine();
    return LCCRF_OK;
}

int get_routes(const Engine *e, unsigned *routes)
{
    if (!e || !routes) return fail(LCCRF_E_INVALID, "handle / routes is NULL");
    *routes = (e->opt.fused_multilabel ? LCCRF_MULTILABEL_POTTS : 0u) | (e->opt.fused_multilabel_learnt ? LCCRF_MULTILABEL_LEARNT : 0u);
    return LCCRF_OK;
}

// The plans are made from what the build measured.  A handle builds its staged lattices, the plain way, and learns their sizes; a
// batch is brought up to date only once lccrf_batch_build has run.
int plan_ready(Engine &e)
{
    const unsigned needs = !e.batch_owned ? Engine::kSettled | Engine::kSized : e.built ? Engine::kSized : 0u;
    return needs ? e.make_ready(needs) : LCCRF_OK;
}

int splat_plan(Engine &e, int kernel, lccrf_splat_plan *out)
{
    if (int rc = plan_ready(e)) return rc;
    report_splat_plan(e.kernels[kernel].dev, e.crf.F, out);
    return LCCRF_OK;
}

int blur_plan_of(Engine &e, int kernel, lccrf_blur_plan *out)
{
    if (int rc = plan_ready(e)) return rc;
    *out = blur_plan(e.kernels[kernel].dev, e.crf.F, e.kernels[kernel].maxV).counts;     // (what launch_step_stream is given)
    return LCCRF_OK;
}

// what the streaming build counted for the lattices now in HBM (engine.h: BuildStat; they came along with the build's copy of rowmax)
int build_report_of(Engine &e, int kernel, int frame, lccrf_build_report *out)
{
    if (frame < 0 || frame >= e.F) return fail(LCCRF_E_INVALID, "frame %d not in [0, %d)", frame, e.F);
    if (int rc = plan_ready(e)) return rc;
    *out = lccrf_build_report{};
    const KernelState &ks = e.kernels[kernel];
    if (!ks.build_counted) return LCCRF_OK;               // (the one-workgroup build, or no build yet)
    const int *st = e.row_host + kernel * e.row_stride() + e.Fcap + (size_t)frame * kBuildStats;
    out->point_buckets_over_64 = st[kBsPtOver64];
    out->largest_point_bucket = st[kBsPtLargest];
    if (!ks.dev.vorder) {                                 // the hash build: the sorted build's counters may be those of an abandoned attempt
        out->long_rows = st[kBsLongRows];
        return LCCRF_OK;
    }
    out->sorted_build = 1;
    out->direct_codes = st[kBsDirect];
    out->long_buckets = st[kBsLongBuckets];
    out->long_by_bitmap = st[kBsBitmap];
    out->long_by_network_uniform = st[kBsNetUniform];
    out->long_by_network_mixed = st[kBsNetMixed];
    out->long_by_network_wide = st[kBsNetWide];
    out->max_buckets_per_workgroup = st[kBsMaxPerWg];
    out->phantom_entries = st[kBsPhantom];
    out->empty_row_vertices = st[kBsEmptyRows];
    return LCCRF_OK;
}

}  // namespace

extern "C" {

// sections 1c and 2c: the terms' weights (the gradients of inference are in api_backward.hip)
int lccrf_set_pairwise_weight(lccrf_handle h, int kernel, float w) { HANDLE_FIRST(h, kernel); return set_weight(h->eng, kernel, w); }
int lccrf_batch_set_pairwise_weight(lccrf_batch_handle b, int kernel, float w) { HANDLE_FIRST(b, kernel); return set_weight(b->eng, kernel, w); }

// sections 1e and 2g: label-compatibility matrices of the pairwise terms (a batch: one per term for every frame)
int lccrf_set_pairwise_compatibility(lccrf_handle h, int kernel, const float *compat) { HANDLE_FIRST(h, kernel); return set_matrix(h->eng, kernel, compat); }
int lccrf_batch_set_pairwise_compatibility(lccrf_batch_handle b, int kernel, const float *compat) { INDEX_FIRST(b, kernel); return set_matrix(b->eng, kernel, compat); }
int lccrf_get_pairwise_compatibility(lccrf_handle h, int kernel, float *out, int *is_set) { HANDLE_FIRST(h, kernel); return get_matrix(h->eng, kernel, out, is_set); }
int lccrf_batch_get_pairwise_compatibility(lccrf_batch_handle b, int kernel, float *out, int *is_set) { INDEX_FIRST(b, kernel); return get_matrix(b->eng, kernel, out, is_set); }

// sections 1g and 2g: where each pairwise term applies its norm
int lccrf_set_pairwise_normalization(lccrf_handle h, int kernel, int mode) { HANDLE_FIRST(h, kernel); CHECK_MODE(mode); return set_mode(h->eng, kernel, mode); }
int lccrf_batch_set_pairwise_normalization(lccrf_batch_handle b, int kernel, int mode) { CHECK_MODE(mode); INDEX_FIRST(b, kernel); return set_mode(b->eng, kernel, mode); }
int lccrf_get_pairwise_normalization(lccrf_handle h, int kernel, int *mode) { HANDLE_FIRST(h, kernel); CHECK_OUT(mode, "mode"); return get_mode(h->eng, kernel, mode); }
int lccrf_batch_get_pairwise_normalization(lccrf_batch_handle b, int kernel, int *mode) { CHECK_OUT(mode, "mode"); INDEX_FIRST(b, kernel); return get_mode(b->eng, kernel, mode); }

// section 1j: which route the last successful backward call took
int lccrf_get_backward_route(lccrf_handle h, int *route) { return get_route(h ? &h->eng : nullptr, route); }
int lccrf_batch_get_backward_route(lccrf_batch_handle b, int *route) { return get_route(b ? &b->eng : nullptr, route); }

// which one-launch kernels frames of three to eight labels may take
int lccrf_set_multilabel_routes(lccrf_handle h, unsigned routes) { return set_routes(h ? &h->eng : nullptr, routes); }
int lccrf_get_multilabel_routes(lccrf_handle h, unsigned *routes) { return get_routes(h ? &h->eng : nullptr, routes); }
int lccrf_batch_set_multilabel_routes(lccrf_batch_handle b, unsigned routes) { return set_routes(b ? &b->eng : nullptr, routes); }
int lccrf_batch_get_multilabel_routes(lccrf_batch_handle b, unsigned *routes) { return get_routes(b ? &b->eng : nullptr, routes); }

// the splat and blur plans of a term's lattices
int lccrf_get_splat_plan(lccrf_handle h, int kernel, lccrf_splat_plan *out) { HANDLE_FIRST(h, kernel); CHECK_OUT(out, "out"); return splat_plan(h->eng, kernel, out); }
int lccrf_batch_get_splat_plan(lccrf_batch_handle b, int kernel, lccrf_splat_plan *out) { HANDLE_FIRST(b, kernel); CHECK_OUT(out, "out"); return splat_plan(b->eng, kernel, out); }
int lccrf_get_blur_plan(lccrf_handle h, int kernel, lccrf_blur_plan *out) { HANDLE_FIRST(h, kernel); CHECK_OUT(out, "out"); return blur_plan_of(h->eng, kernel, out); }
int lccrf_batch_get_blur_plan(lccrf_batch_handle b, int kernel, lccrf_blur_plan *out) { HANDLE_FIRST(b, kernel); CHECK_OUT(out, "out"); return blur_plan_of(b->eng, kernel, out); }
int lccrf_get_build_report(lccrf_handle h, int kernel, lccrf_build_report *out) { HANDLE_FIRST(h, kernel); CHECK_OUT(out, "out"); return build_report_of(h->eng, kernel, 0, out); }
int lccrf_batch_get_build_report(lccrf_batch_handle b, int kernel, int frame, lccrf_build_report *out) { HANDLE_FIRST(b, kernel); CHECK_OUT(out, "out"); return build_report_of(b->eng, kernel, frame, out); }

}  // extern "C"

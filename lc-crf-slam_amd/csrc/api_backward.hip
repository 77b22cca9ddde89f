// api_backward.hip -- gradients of mean-field inference: sections 1c - 1f, 1m (a handle) and 2c, 2d, 2h - 2l (a batch) of include/lccrf.h.
//
// One path behind every entry point (backward_call); the replay and the sweep themselves are Engine::backward (host_engine.hip) and
// meanfield_backward.hip; the route getters of section 1j are in api_model.hip.
#include "api_common.h"

#include <cmath>

using namespace lccrf;

// Every backward entry point, of a handle (sections 1c - 1f, 1m) and of a batch (2c, 2d, 2h, 2i), fills a BackwardRequest (engine.h), says where
// it runs and what it allows, and calls backward_call.  A handle is a batch of one whose area has its own row stride.
struct BackwardTarget {
    Engine &e;
    int rows;                  // points per frame: N of a handle, maxN of a batch (the caller's arrays are [F][rows][.])
    size_t slice;              // floats per array of the area: backward_stride(N, L), or F * maxN * L
    bool ready;                // the state the call needs ...
    const char *not_ready;     // ... and what it says without it
    bool batch;                // a batch's call: timed, on `stream`, every frame's lattices in HBM and built the plain way
    void *stream;
};
constexpr bool kGradUnaryRequired = true, kGradUnaryOptional = false;   // may the entry point's d_grad_unary be NULL?

// The one path of every backward call.  In this order: the arguments (which outputs may be NULL is the entry point's to say:
// need_grad_unary, and what it leaves out of the request), the state, a pending one-launch inference, the area -- before anything
// runs, so that a handle that cannot have it is left as it was -- and then the replay and the sweep (Engine::backward).
static int backward_call(const BackwardTarget &t, const BackwardRequest &rq, bool need_grad_unary)
{
    Engine &e = t.e;
    if (rq.T < 0) return fail(LCCRF_E_INVALID, "n_iterations < 0");
    if (!std::isfinite(rq.relax)) return fail(LCCRF_E_INVALID, "relax must be finite");
    const size_t K = e.kernels.size(), points = (size_t)e.F * t.rows, nl = points * e.L;
    int rc;
    if ((rc = check_device_array(e, rq.grad_prob, nl * sizeof(float), "d_grad_prob"))) return rc;
    if ((need_grad_unary || rq.grad_unary) && (rc = check_device_array(e, rq.grad_unary, nl * sizeof(float), "d_grad_unary"))) return rc;
    if (rq.grad_weights && (rc = check_device_array(e, rq.grad_weights, e.F * K * sizeof(float), "d_grad_weights"))) return rc;
    if (rq.counts && (rc = check_device_array(e, rq.counts, e.F * sizeof(int32_t), "d_iterations"))) return rc;
    for (size_t k = 0; k < K && rq.grad_features; ++k)
        if (rq.grad_features[k] &&
            (rc = check_device_array(e, rq.grad_features[k], points * e.kernels[k].dev.d * sizeof(float), "d_grad_features[k]")))
            return rc;
    // (K = 0: zero bytes, nothing to check)
    if (rq.grad_compat && (rc = check_device_array(e, rq.grad_compat, e.F * K * e.L * e.L * sizeof(float), "d_grad_compat"))) return rc;
    if (rq.grad_model && (rc = check_device_array(e, rq.grad_model, K * (1 + (size_t)e.L * e.L) * sizeof(float), "d_grad_model"))) return rc;
    if (!t.ready) return fail(LCCRF_E_STATE, "%s", t.not_ready);
    auto run = [&] {
        int rr = e.resolve_late();
        if (rr) return rr;
        if ((rr = e.ensure_backward_area(e.backward_need(rq, t.slice, t.rows)))) return rr;   // (a handle's phantom rows stay zero: engine.h)
        if (t.batch && (rr = e.make_ready(Engine::kCallerOrder | Engine::kSized))) return rr;
        return e.backward(rq, t.slice, t.rows);
    };
    return t.batch ? timed_batch_call(e, t.stream, e.ev[2], e.ev[3], e.timed_inf, run) : run();
}

static BackwardTarget backward_target(lccrf_crf *h)
{
    return {h->eng, h->N, backward_stride(h->N, h->eng.L), h->eng.unary_set, "unary energies not set", false, nullptr};
}

static BackwardTarget backward_target(lccrf_batch *b, void *stream)
{
    Engine &e = b->eng;
    // (started: lccrf_batch_run on the one-launch kernel leaves no lattice in HBM -- they are built here)
    return {e, e.maxN, (size_t)e.F * e.maxN * e.L, b->inputs_set && (e.built || e.started),
            "lccrf_batch_build or lccrf_batch_run has not run for these inputs", true, stream};
}

// Sections 2c and 2d differentiate Potts terms normalised AFTER, and keep refusing a batch with a matrix or another mode (section 2g)
// before anything is looked at or touched: the gradients of such a batch -- every frame with the bits of a handle's section 1e and 1g
// gradients -- are section 2h's, lccrf_batch_inference_backward_all below.
static int batch_is_plain(const lccrf_batch *b)
{
    if (b->eng.model.n_compat) return fail(LCCRF_E_STATE, "batch gradients are not available while a term has a label-compatibility matrix: lccrf_batch_inference_backward_all");
    if (b->eng.model.n_modes) return fail(LCCRF_E_STATE, "batch gradients are not available while a term is not normalised AFTER the filter: lccrf_batch_inference_backward_all");
    return LCCRF_OK;
}

extern "C" {

// --------------------------------------------------------------------------------------
// section 1c: gradients of inference()

int lccrf_inference_backward(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                             float *d_grad_weights)
{
    CHECK_H(h);
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.compat_form = h->eng.model.n_compat > 0;                 // (section 1e: the gradients of the forward with the matrices)
    return backward_call(backward_target(h), rq, kGradUnaryRequired);
}

// --------------------------------------------------------------------------------------
// section 1d: ... and with respect to the features of the pairwise terms

int lccrf_inference_backward_features(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                      float *d_grad_weights, float *const *d_grad_features)
{
    CHECK_H(h);
    if (h->eng.model.n_compat) return fail(LCCRF_E_STATE, "feature gradients are not available while a term has a label-compatibility matrix");
    if (h->eng.model.n_modes) return fail(LCCRF_E_STATE, "feature gradients are not available while a term is not normalised AFTER the filter");
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    return backward_call(backward_target(h), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 1e: ... and with respect to the label-compatibility matrices

int lccrf_inference_backward_compat(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                    float *d_grad_weights, float *d_grad_compat)
{
    if (!d_grad_compat) return lccrf_inference_backward(h, n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights);
    CHECK_H(h);
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_compat = d_grad_compat;
    rq.compat_form = true;
    return backward_call(backward_target(h), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 1f: ... and with respect to the features and the matrices in one sweep

int lccrf_inference_backward_all(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                 float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat)
{
    CHECK_H(h);
    if (d_grad_features && h->eng.model.n_modes)                // (section 1g: the norm's factors are not differentiated in the features)
        return fail(LCCRF_E_STATE, "feature gradients are not available while a term is not normalised AFTER the filter");
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    rq.grad_compat = d_grad_compat;
    rq.compat_form = h->eng.model.n_compat > 0 || d_grad_compat;
    return backward_call(backward_target(h), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 2c: gradients of a batch's inference

int lccrf_batch_inference_backward(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                   float *d_grad_weights, void *stream)
{
    CHECK_H(b);
    if (int rc = batch_is_plain(b)) return rc;
    const BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    return backward_call(backward_target(b, stream), rq, kGradUnaryRequired);
}

// --------------------------------------------------------------------------------------
// section 2j: section 2c with one iteration count per frame -- the gradients of lccrf_batch_inference_converged's result.  The counts
// stay on the device (the kernels clamp them to [0, max_iterations]); what needs no handle is checked before the handle is looked at,
// so those answers need no device.

int lccrf_batch_inference_backward_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                             const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights, void *stream)
{
    if (max_iterations < 0) return fail(LCCRF_E_INVALID, "max_iterations < 0");
    if (!std::isfinite(relax)) return fail(LCCRF_E_INVALID, "relax must be finite");
    if (!d_iterations) return fail(LCCRF_E_INVALID, "d_iterations is NULL");
    CHECK_H(b);
    if (int rc = batch_is_plain(b)) return rc;
    BackwardRequest rq{max_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.counts = d_iterations;
    return backward_call(backward_target(b, stream), rq, kGradUnaryRequired);
}

// --------------------------------------------------------------------------------------
// section 2d: ... and with respect to the features of the pairwise terms

int lccrf_batch_inference_backward_features(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob,
                                            float *d_grad_unary, float *d_grad_weights, float *const *d_grad_features, void *stream)
{
    CHECK_H(b);
    if (int rc = batch_is_plain(b)) return rc;
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    return backward_call(backward_target(b, stream), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 2h: section 1f for every frame of a batch, Potts or learnt, and the sums over the frames

int lccrf_batch_inference_backward_all(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                       float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat, float *d_grad_model,
                                       void *stream)
{
    CHECK_H(b);
    if (d_grad_features && b->eng.model.n_modes)                // (section 1g: the norm's factors are not differentiated in the features)
        return fail(LCCRF_E_STATE, "feature gradients are not available while a term is not normalised AFTER the filter");
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    rq.grad_compat = d_grad_compat;
    rq.grad_model = d_grad_model;
    rq.compat_form = b->eng.model.n_compat > 0 || d_grad_compat || d_grad_model;   // (the sums hold dL/dmu: section 1e's form)
    return backward_call(backward_target(b, stream), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 2k: section 2h without the feature gradients, with section 2j's count per frame -- the gradients of
// lccrf_batch_inference_converged's result under a learnt model.  The request is section 2h's with `counts` set: on a batch without
// matrices or modes, with neither dL/dmu nor the sums asked for, it is section 2j's request.  What needs no handle is checked first.

int lccrf_batch_inference_backward_all_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                                 const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights,
                                                 float *d_grad_compat, float *d_grad_model, void *stream)
{
    if (max_iterations < 0) return fail(LCCRF_E_INVALID, "max_iterations < 0");
    if (!std::isfinite(relax)) return fail(LCCRF_E_INVALID, "relax must be finite");
    if (!d_iterations) return fail(LCCRF_E_INVALID, "d_iterations is NULL");
    CHECK_H(b);
    BackwardRequest rq{max_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_compat = d_grad_compat;
    rq.grad_model = d_grad_model;
    rq.compat_form = b->eng.model.n_compat > 0 || d_grad_compat || d_grad_model;   // (as section 2h sets it)
    rq.counts = d_iterations;
    return backward_call(backward_target(b, stream), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// sections 1m and 2i: sections 1f and 2h with the feature gradients of terms in any normalisation mode.  The request is section
// 1f's / 2h's; Engine::backward hands the sweep the modes when a term is not AFTER and a feature array is asked for, and that request
// streams (no fused route takes feature gradients of a model with a mode).  Every other request IS the other call.

int lccrf_inference_backward_modes(lccrf_handle h, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                   float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat)
{
    CHECK_H(h);
    if (!d_grad_features || !h->eng.model.n_modes)
        return lccrf_inference_backward_all(h, n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights, d_grad_features, d_grad_compat);
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    rq.grad_compat = d_grad_compat;
    rq.compat_form = h->eng.model.n_compat > 0 || d_grad_compat;
    return backward_call(backward_target(h), rq, kGradUnaryOptional);
}

int lccrf_batch_inference_backward_modes(lccrf_batch_handle b, int n_iterations, float relax, const float *d_grad_prob, float *d_grad_unary,
                                         float *d_grad_weights, float *const *d_grad_features, float *d_grad_compat, float *d_grad_model,
                                         void *stream)
{
    CHECK_H(b);
    if (!d_grad_features || !b->eng.model.n_modes)
        return lccrf_batch_inference_backward_all(b, n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights, d_grad_features,
                                                  d_grad_compat, d_grad_model, stream);
    BackwardRequest rq{n_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    rq.grad_compat = d_grad_compat;
    rq.grad_model = d_grad_model;
    rq.compat_form = b->eng.model.n_compat > 0 || d_grad_compat || d_grad_model;
    return backward_call(backward_target(b, stream), rq, kGradUnaryOptional);
}

// --------------------------------------------------------------------------------------
// section 2l: section 2i with section 2j's count per frame -- the gradients of lccrf_batch_inference_converged's result with respect to
// the features too, under any model.  The request is section 2i's with `counts` set; without a feature array it IS section 2k's call.
// What needs no handle is checked first.

int lccrf_batch_inference_backward_modes_converged(lccrf_batch_handle b, int max_iterations, float relax, const int32_t *d_iterations,
                                                   const float *d_grad_prob, float *d_grad_unary, float *d_grad_weights,
                                                   float *const *d_grad_features, float *d_grad_compat, float *d_grad_model, void *stream)
{
    if (max_iterations < 0) return fail(LCCRF_E_INVALID, "max_iterations < 0");
    if (!std::isfinite(relax)) return fail(LCCRF_E_INVALID, "relax must be finite");
    if (!d_iterations) return fail(LCCRF_E_INVALID, "d_iterations is NULL");
    CHECK_H(b);
    bool no_features = true;
    for (size_t k = 0; k < b->eng.kernels.size() && d_grad_features; ++k) no_features &= d_grad_features[k] == nullptr;
    if (no_features)
        return lccrf_batch_inference_backward_all_converged(b, max_iterations, relax, d_iterations, d_grad_prob, d_grad_unary,
                                                            d_grad_weights, d_grad_compat, d_grad_model, stream);
    BackwardRequest rq{max_iterations, relax, d_grad_prob, d_grad_unary, d_grad_weights};
    rq.grad_features = d_grad_features;
    rq.grad_compat = d_grad_compat;
    rq.grad_model = d_grad_model;
    rq.compat_form = b->eng.model.n_compat > 0 || d_grad_compat || d_grad_model;   // (as sections 2h and 2i set it)
    rq.counts = d_iterations;
    return backward_call(backward_target(b, stream), rq, kGradUnaryOptional);
}

}  // extern "C"

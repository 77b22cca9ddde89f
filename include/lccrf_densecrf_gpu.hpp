// lccrf_densecrf_gpu.hpp -- header-only C++ mirror of the reference's GPU operator classes (Thirdparty/DenseCRF/README.md,
// "GPU Version": DenseCRFGPU<M>, PottsPotentialGPU<M,F>::FromImage; "all pointers should be device pointers") on top of
// section 1b of the C-ABI (lccrf.h).  C++14; no HIP header is needed: the C-ABI hides the runtime.
//
// The reference's GPU example compiles against it with the type names as they are and this header in place of its two
// .cuh headers:
//
//     DenseCRFGPU<M> crf(W * H);
//     crf.setUnaryEnergyFromLabel(labelGPU, 0.5);
//     crf.addPairwiseEnergy(PottsPotentialGPU<M, 2>::FromImage<>(W, H, 3.0, 3.0));
//     crf.addPairwiseEnergy(PottsPotentialGPU<M, 5>::FromImage<float>(W, H, 10.0, 60.0, rgbFeatGPU, 20.0));
//     crf.inference(10, true);
//     short *mapGPU = crf.getMap();
//
// Both classes derive from the same DenseCRF / PairwisePotential bases as lccrf_densecrf.hpp's (the reference's own with its tree
// on the include path).  Differences from the reference, all deliberate:
//   * the device arrays handed to a PottsPotentialGPU (features, image) are CONSUMED WHEN THE ADOPTING CRF ADDS THE TERM
//     (addPairwiseEnergy, or a stand-alone apply()): a kernel on that CRF's stream copies them into the CRF then.  They must stay
//     valid until that stream has passed it -- crf.synchronize(), or any call below that waits (inference() does).  The reference
//     consumes them in the potential's constructor;
//   * inference(), startInference() and stepInference() end with a synchronisation of the CRF's stream, so getMap() /
//     getProbability() hand out device arrays that are complete and may be read on any stream (hipMemcpy);
//   * setUnaryEnergyFromLabel reads the M confidences (a device array, as every pointer here) when it is called;
//   * errors throw std::runtime_error, as in lccrf_densecrf.hpp.
#pragma once

#include <type_traits>
#include <vector>

#include "lccrf_densecrf.hpp"

namespace DenseCRF {

// What a DenseCRFGPU needs to know about a potential whose inputs live on the device.
class GpuPotential {
public:
    virtual ~GpuPotential() = default;
    virtual void addTo(lccrf_handle crf) const = 0;                 // enqueue this term on crf (consumes the device arrays)
    virtual void bind(lccrf_handle crf, int kernel) const = 0;      // from now on apply() is term `kernel` of that CRF
};

// PottsPotentialGPU<M,F>: PottsPotentialCPU<M,F> (pairwise_cpu.h:8-58) on device arrays
template <int M, int F>
class PottsPotentialGPU : public PairwisePotential, public GpuPotential {
protected:
    float w_;
    const void *src_;                               // device features [N][F], or the image of FromImage (or null)
    int image_format_ = -1;                         // -1: src_ holds features; else LCCRF_IMAGE_*
    int width_ = 0, height_ = 0;
    float posdev_ = 1.0f, featuredev_ = 0.0f;
    mutable lccrf_handle h_ = nullptr;              // the CRF this term belongs to, or a private one-term CRF (own_)
    mutable int k_ = -1;
    mutable bool own_ = false;
    int device_id_ = 0;

public:
    // the device features [N][F], already divided by the stdevs
    PottsPotentialGPU(const float *d_features, int N, float w, int device_id = 0)
        : PairwisePotential(N), w_(w), src_(d_features), device_id_(device_id) {}
    PottsPotentialGPU(const PottsPotentialGPU &) = delete;
    ~PottsPotentialGPU() override
    {
        if (own_) lccrf_destroy(h_);
    }

    // pairwise_cpu.h:33-51: features (x, y) / posdev of pixel y * w + x, then (F = 5) its RGB / featuredev.  d_image is a device
    // array [w*h][3] (HWC) of float or unsigned char; F = 2 ignores it, as the reference does.
    template <class T = float>
    static PottsPotentialGPU<M, F> *FromImage(int w, int h, float weight, float posdev, const T *d_image = nullptr, float featuredev = 0.0)
    {
        static_assert(std::is_same<T, float>::value || std::is_same<T, unsigned char>::value,
                      "FromImage takes a float or an unsigned char image");
        static_assert(F == 2 || F == 5, "FromImage forms 2 (position) or 5 (position + RGB) features");
        if (F == 5 && !d_image) throw std::runtime_error("PottsPotentialGPU<M,5>::FromImage needs an image");
        auto *p = new PottsPotentialGPU<M, F>(nullptr, w * h, weight);
        p->width_ = w;
        p->height_ = h;
        p->posdev_ = posdev;
        if (F == 5) {
            p->src_ = d_image;
            p->image_format_ = std::is_same<T, float>::value ? LCCRF_IMAGE_F32 : LCCRF_IMAGE_U8;
            p->featuredev_ = featuredev;
        } else {
            p->image_format_ = LCCRF_IMAGE_NONE;
        }
        return p;
    }

    int device() const { return device_id_; }
    void addTo(lccrf_handle crf) const override
    {
        if (image_format_ < 0)
            lccrf_check(lccrf_add_pairwise_device(crf, static_cast<const float *>(src_), F, w_), "lccrf_add_pairwise_device");
        else
            lccrf_check(lccrf_add_image_kernel(crf, width_, height_, w_, posdev_, src_, image_format_, featuredev_), "lccrf_add_image_kernel");
    }
    void bind(lccrf_handle crf, int kernel) const override
    {
        if (own_) lccrf_destroy(h_);
        own_ = false;
        h_ = crf;
        k_ = kernel;
    }

    // densecrf_base.h:18: out_values += w * norm * compute(in_values), both [N][M] device arrays; `tmp` is unused (the scratch
    // lives in the CRF).  A potential that belongs to no CRF yet builds a private one-term CRF; the call returns when it is done.
    void apply(float *out_values, const float *in_values, float * /*tmp*/) const override
    {
        if (!h_) {
            lccrf_check(lccrf_create(&h_, device_id_, N_, M), "lccrf_create");
            own_ = true;
            k_ = 0;
            addTo(h_);
        }
        lccrf_check(lccrf_pairwise_apply_device(h_, k_, out_values, in_values), "lccrf_pairwise_apply_device");
        if (own_) lccrf_check(lccrf_synchronize(h_), "lccrf_synchronize");
    }
};

// DenseCRFGPU<M>: the reference's DenseCRFGPU on this library's kernels; unary_, current_, next_, tmp_ and map_ are the handle's
// own HBM arrays (lccrf_device_buffers).
template <int M>
class DenseCRFGPU : public DenseCRF {
protected:
    lccrf_handle h_ = nullptr;
    size_t adopted_ = 0;                  // pairwise_[0, adopted_) have been looked at
    int n_terms_ = 0;                     // ... of which this many are terms of the handle
    std::vector<int> term_;               // per pairwise_ entry: its term in the handle, or -1 (a foreign potential)
    bool mixed_ = false;                  // some potential is not ours: stepping through the base class on device arrays
    int conv_iterations_ = 0, conv_changed_ = 0, conv_converged_ = 0;   // what the last inferenceConverged() reported
    float conv_delta_ = 0.0f;

    void adopt()
    {
        for (; adopted_ < pairwise_.size(); ++adopted_) {
            PairwisePotential *p = pairwise_[adopted_];
            int k = -1;
            if (const GpuPotential *gp = dynamic_cast<const GpuPotential *>(p)) {
                gp->addTo(h_);
                k = n_terms_++;
                gp->bind(h_, k);
            } else if (const HipPotential *hp = dynamic_cast<const HipPotential *>(p)) {   // host features: a term all the same
                lccrf_check(lccrf_add_pairwise(h_, hp->features(), hp->dims(), hp->weight()), "lccrf_add_pairwise");
                k = n_terms_++;
                hp->bind(h_, k);
            } else {
                mixed_ = true;
            }
            term_.push_back(k);
        }
    }
    void sync() const { lccrf_check(lccrf_synchronize(h_), "lccrf_synchronize"); }

    // DenseCRF's protected virtuals (densecrf_base.h:34-36) on the device arrays, each one kernel on the CRF's stream
    void expAndNormalize(float *out, const float *in, float scale = 1.0, float relax = 1.0) override
    {
        lccrf_check(lccrf_exp_and_normalize_device(h_, out, in, scale, relax), "lccrf_exp_and_normalize_device");
    }
    void stepInit() override { lccrf_check(lccrf_step_init_device(h_, next_), "lccrf_step_init_device"); }
    void buildMap() override
    {
        if (mixed_) lccrf_check(lccrf_map_of_device(h_, current_, map_), "lccrf_map_of_device");
        else lccrf_check(lccrf_build_map(h_), "lccrf_build_map");
    }

public:
    explicit DenseCRFGPU(int N, int device_id = 0) : DenseCRF(N)
    {
        lccrf_check(lccrf_create(&h_, device_id, N, M), "lccrf_create");
        const float *u = nullptr;
        float *cur = nullptr, *next = nullptr, *tmp = nullptr;
        int16_t *map = nullptr;
        const int rc = lccrf_device_buffers(h_, &u, &cur, &next, &tmp, &map);
        if (rc != LCCRF_OK) {
            lccrf_destroy(h_);
            lccrf_check(rc, "lccrf_device_buffers");
        }
        unary_ = const_cast<float *>(u);  // (written by setUnaryEnergy*, read by startInference)
        current_ = cur;
        next_ = next;
        tmp_ = tmp;
        map_ = reinterpret_cast<short *>(map);
    }
    ~DenseCRFGPU() override
    {
        lccrf_destroy(h_);
        unary_ = current_ = next_ = tmp_ = nullptr;
        map_ = nullptr;
    }
    DenseCRFGPU(DenseCRFGPU &) = delete;

    // densecrf_base.h:54 -- ownership of the potential moves to the CRF; a PottsPotentialGPU's device arrays are consumed here
    void addPairwiseEnergy(PairwisePotential *potential)
    {
        DenseCRF::addPairwiseEnergy(potential);
        adopt();
    }

    // all pointers are device pointers
    void setUnaryEnergy(const float *unary) override { lccrf_check(lccrf_set_unary_device(h_, unary), "lccrf_set_unary_device"); }
    void setUnaryEnergyFromLabel(const short *label, float *confidences) override
    {
        lccrf_check(lccrf_set_unary_from_label_device(h_, reinterpret_cast<const int16_t *>(label), confidences),
                    "lccrf_set_unary_from_label_device");
    }
    void setUnaryEnergyFromLabel(const short *label, float confidence = 0.5) override
    {
        float c[M];                       // (host values: the one array of this interface that is not the caller's)
        for (int i = 0; i < M; ++i) c[i] = confidence;
        lccrf_check(lccrf_set_unary_from_label_device(h_, reinterpret_cast<const int16_t *>(label), c),
                    "lccrf_set_unary_from_label_device");
    }

    void inference(int n_iterations, bool with_map = false, float relax = 1.0) override
    {
        adopt();
        if (mixed_) {
            startInference();
            for (int it = 0; it < n_iterations; ++it) stepInference(relax);
            if (with_map) buildMap();
        } else {
            lccrf_check(lccrf_inference(h_, n_iterations, with_map ? 1 : 0, relax), "lccrf_inference");
        }
        sync();
    }
    // Mean-field iterations until converged, at most max_iterations (include/lccrf.h section 1h; DenseCRFHIP::inferenceConverged
    // on device arrays); ends with a synchronisation like inference().  Not supported with foreign potentials (mixed()): throws.
    void inferenceConverged(int max_iterations, int criterion = LCCRF_STOP_LABELS, float tol = 0.0f, bool with_map = false,
                            float relax = 1.0)
    {
        adopt();
        if (mixed_) throw std::runtime_error("inferenceConverged: not supported with foreign potentials");
        lccrf_check(lccrf_inference_converged(h_, max_iterations, criterion, tol, with_map ? 1 : 0, relax), "lccrf_inference_converged");
        lccrf_check(lccrf_get_convergence(h_, &conv_iterations_, &conv_delta_, &conv_changed_, &conv_converged_), "lccrf_get_convergence");
        sync();
    }
    // inferenceConverged() from inputs alone (include/lccrf.h section 1i): a fresh frame is built, normalised and inferred until
    // converged in ONE kernel launch.  Results and accessors as inferenceConverged's; ends with a synchronisation.
    void runConverged(int max_iterations, int criterion = LCCRF_STOP_LABELS, float tol = 0.0f, bool with_map = false, float relax = 1.0)
    {
        adopt();
        if (mixed_) throw std::runtime_error("runConverged: not supported with foreign potentials");
        lccrf_check(lccrf_run_converged(h_, max_iterations, criterion, tol, with_map ? 1 : 0, relax), "lccrf_run_converged");
        lccrf_check(lccrf_get_convergence(h_, &conv_iterations_, &conv_delta_, &conv_changed_, &conv_converged_), "lccrf_get_convergence");
        sync();
    }
    int iterations() const { return conv_iterations_; }        // of the last inferenceConverged() / runConverged(): t, d_t, c_t, the criterion was met
    float delta() const { return conv_delta_; }
    int changed() const { return conv_changed_; }
    bool converged() const { return conv_converged_ != 0; }
    void startInference() override                // densecrf_base.h:78-80, unary_ being the handle's device unaries
    {
        adopt();
        if (mixed_) expAndNormalize(current_, unary_, -1);
        else lccrf_check(lccrf_start_inference(h_), "lccrf_start_inference");
        sync();
    }
    // densecrf_base.h:82-91.  A foreign potential's apply() is called with the CRF's stream idle and must have finished writing
    // next_ when it returns (it knows nothing of that stream).
    void stepInference(float relax = 1.0) override
    {
        adopt();
        if (!mixed_) {
            lccrf_check(lccrf_step_inference(h_, relax), "lccrf_step_inference");
            sync();
            return;
        }
        stepInit();
        for (size_t i = 0; i < pairwise_.size(); ++i) {
            if (term_[i] >= 0) {
                lccrf_check(lccrf_pairwise_apply_device(h_, term_[i], next_, current_), "lccrf_pairwise_apply_device");
            } else {
                sync();
                pairwise_[i]->apply(next_, current_, tmp_);
            }
        }
        expAndNormalize(current_, next_, 1.0, relax);
        sync();
    }

    // densecrf_base.h:74-75: the handle's HBM arrays, valid until destruction
    short *getMap() const { return map_; }
    float *getProbability() const { return current_; }

    int latticeSize(int kernel)
    {
        adopt();
        int V = 0;
        lccrf_check(lccrf_get_lattice_size(h_, kernel, &V), "lccrf_get_lattice_size");
        return V;
    }
    // lccrf_set_option (include/lccrf.h); setOption(LCCRF_OPT_FRAME_GENERAL, 1) keeps a learnt model on the one-launch route of a fresh frame.
    // setOption(LCCRF_OPT_FUSED_BACKWARD_LEARNT, 1): the gradients of such a model, dL/dmu included, run in one launch (section 1k).
    void setOption(int option, int value) { lccrf_check(lccrf_set_option(h_, option, value), "lccrf_set_option"); }
    // lccrf_get_backward_route (include/lccrf.h section 1j): the route of the last successful backward call on this handle -- 0 none yet,
    // 1 the streaming sweep, 2 one launch (setOption(LCCRF_OPT_FUSED_BACKWARD, 1) / (LCCRF_OPT_FUSED_BACKWARD_LEARNT, 1)).  Report only.
    int backwardRoute() const
    {
        int r = 0;
        lccrf_check(lccrf_get_backward_route(h_, &r), "lccrf_get_backward_route");
        return r;
    }
    void synchronize() const { sync(); }
    void *stream() const
    {
        void *s = nullptr;
        lccrf_check(lccrf_get_stream(h_, &s), "lccrf_get_stream");
        return s;
    }
    bool mixed() const { return mixed_; }
    lccrf_handle handle() const { return h_; }
};

}  // namespace DenseCRF

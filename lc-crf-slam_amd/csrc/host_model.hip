// host_model.hip -- Engine::LearntModel (host_engine.h): the terms' label-compatibility matrices and normalisation modes, the factors
// the modes need, and the one place that counts them.
#include "host_engine.h"

#include <cstring>

namespace lccrf {

void Engine::LearntModel::clear(Engine &e)
{
    for (int k = 0; k < LCCRF_MAX_KERNELS; ++k) {
        compat_ptr[k] = nullptr;
        norm_mode[k] = LCCRF_NORMALIZE_AFTER;
    }
    n_compat = n_modes = 0;
    e.choose_sized_engine();
}

// m: host [L][L] (finite, checked by the caller) or null.
int Engine::LearntModel::set_matrix(Engine &e, int k, const float *m)
{
    ll = (size_t)e.L * e.L;
    if (m) {
        if (!compat_dev) {
            int rc = e.mem.alloc_pinned(&compat_host, (size_t)LCCRF_MAX_KERNELS * ll);
            if (!rc) rc = e.mem.alloc(&compat_dev, (size_t)LCCRF_MAX_KERNELS * ll);
            if (rc) { compat_dev = nullptr; return rc; }
            HIP_TRY(hipEventCreateWithFlags(&compat_ev, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(compat_ev, e.stream));
        }
        HIP_TRY(hipEventSynchronize(compat_ev));        // (an earlier upload may still be reading the pinned copy)
        memcpy(compat_host + k * ll, m, ll * sizeof(float));   // (the caller's array is free again when the call returns)
        HIP_TRY(hipMemcpyAsync(compat_dev + k * ll, compat_host + k * ll, ll * sizeof(float), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipEventRecord(compat_ev, e.stream));
    }
    const float *p = m ? compat_dev + k * ll : nullptr;
    n_compat += (p != nullptr) - (compat_ptr[k] != nullptr);
    compat_ptr[k] = p;
    e.choose_sized_engine();
    return LCCRF_OK;
}

void Engine::LearntModel::views_changed() { factors_dirty = true; }

// mode: 0 .. 3, checked by the caller.
void Engine::LearntModel::set_mode(Engine &e, int k, int mode)
{
    n_modes += (mode != LCCRF_NORMALIZE_AFTER) - (norm_mode[k] != LCCRF_NORMALIZE_AFTER);
    norm_mode[k] = mode;
    factors_dirty = true;
    e.choose_sized_engine();
}

// The model as it is now, on the engine g (its first K terms): cleared, then set through g's own setters.
int Engine::LearntModel::put_on(Engine &g, int K) const
{
    g.model.clear(g);
    for (int k = 0; k < K; ++k) {
        if (int rc = has_matrix(k) ? g.model.set_matrix(g, k, matrix(k)) : LCCRF_OK) return rc;
        g.model.set_mode(g, k, norm_mode[k]);
    }
    return LCCRF_OK;
}

// Behind kSized, before anything reads step_kdevs() / pre_arg(): the factors the terms' modes need -- the square roots of a
// SYMMETRIC term's norm, formed on the stream right behind the norm itself (in its point order, locality mode included) when a build
// or a mode change has left them stale, and the array of ones -- and the views that point at them.
int Engine::LearntModel::ensure_factors(Engine &e)
{
    if (!n_modes || !factors_dirty) return LCCRF_OK;   // (a build clears root_valid and goes through sync_views: dirty again)
    const size_t np = (size_t)e.Fcap * e.maxN;
    kdevs_post = e.kdevs;
    for (size_t k = 0; k < e.kernels.size(); ++k) {
        KernelState &ks = e.kernels[k];
        const int mode = norm_mode[k];
        pre_ptr[k] = nullptr;
        if (mode == LCCRF_NORMALIZE_SYMMETRIC) {
            if (!ks.norm_root) {
                int rc = e.mem.alloc(&ks.norm_root, np);
                if (rc) { ks.norm_root = nullptr; return rc; }
                ks.root_valid = false;
            }
            if (!ks.root_valid) launch_norm_factor(e.crf, ks.dev.norm, ks.norm_root, 1, e.stream);
            ks.root_valid = true;
            pre_ptr[k] = kdevs_post[k].norm = ks.norm_root;
        } else if (mode != LCCRF_NORMALIZE_AFTER) {
            if (!ones) {
                int rc = e.mem.alloc(&ones, np, false);
                if (rc) { ones = nullptr; return rc; }
                CrfDev all = e.crf;                        // every frame the engine can hold: a batch's next inputs may bind more
                all.F = e.Fcap;                            //   frames than its first (a handle has one)
                launch_norm_factor(all, nullptr, ones, 0, e.stream);
            }
            if (mode == LCCRF_NORMALIZE_BEFORE) pre_ptr[k] = ks.dev.norm;
            kdevs_post[k].norm = ones;
        }
    }
    HIP_TRY(hipGetLastError());
    factors_dirty = false;
    return LCCRF_OK;
}

}  // namespace lccrf

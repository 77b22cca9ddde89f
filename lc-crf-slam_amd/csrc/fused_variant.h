// fused_variant.h -- the launch plan that the fused engine's variants in units of their own (k_general, k_converge,
// k_general_converge) share, and the host helper that fills the general kernels' terms.
//
// Their kernels open with k_fused's self-contained prologue (MODE 0 / 1).  It lives once, in fused_prologue.inc, and all four kernels
// include it as text in front of their first barrier.  Text, not a function: as two shared __forceinline__ functions the prologue
// compiled within every pinned figure, but on an MI355X the c2 frame then ran k_converge in 38.75 / 38.75 / 38.78 us against
// 38.57 / 38.63 / 38.57 and k_general (matrices) in 35.85 / 35.86 / 35.93 against 35.65 / 35.73 / 35.78 -- outside the parent's
// spread.  Included text compiles every one of these kernels to the instructions its own copy gave (notes/fused_general.md section 6).
#pragma once

#include "fused_loop.h"
#include "dispatch.h"

namespace lccrf {
namespace {

// Frames of up to MaxPPT x 1024 active points on lattices that fit the fused plan with `extra_lds` bytes behind it: fills a.lay and
// a.kd, then calls launch(points per lane, K, kernel 0 on chain rows) -- three integral_constants -- which names the kernel.
// Returns fused_report() of the shape, or 0 with `launch` not called.
template <int MaxPPT, typename Args, typename Launch>
int plan_variant(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, size_t extra_lds, Args &a, Launch launch)
{
    using namespace fl;
    const int NA = active_points(c);
    if (NA > MaxPPT * kNT || !slam_shaped(c, kds, true)) return 0;
    if (!layout_core(NA, c.K, maxV, maxRow ? maxRow[0] : 0, &a.lay)) return 0;
    if ((size_t)a.lay.total + extra_lds > kLdsLimit) return 0;
    for (int k = 0; k < c.K; ++k) a.kd[k] = kds[k];
    const int ppt = std::max((NA + kNT - 1) / kNT, 1);
    with_dims<1, kMaxFusedK>(c.K, [&](auto kk) {
        with_dims<0, 1>(a.lay.chain0 ? 1 : 0, [&](auto ch) { with_dims<1, MaxPPT>(ppt, [&](auto p) { launch(p, kk, ch); }); });
    });
    return fused_report(kNT, ppt, a.lay.chain0);
}

// The general kernels' terms (GeneralArgs, GeneralConvergeArgs: pre[], has_mu, mu[][]) from the request's: the factors in front of
// the filter and the matrices, each null for a term without one.  Called behind the plan's guard: c.K <= kMaxFusedK.
template <typename Args>
void fill_general_terms(Args &a, const CrfDev &c, const TermModel &t)
{
    for (int k = 0; k < c.K; ++k) a.pre[k] = t.pre ? t.pre[k] : nullptr;
    a.has_mu = copy_matrices(t, c.K, a.mu);
}
// ... and the converged kernels' run and report (ConvergeArgs, GeneralConvergeArgs)
template <typename Args>
void fill_converge_run(Args &a, const SizedRequest &rq)
{
    a.max_iter = rq.run.n_iter;
    a.with_map = rq.run.with_map;
    a.criterion = rq.run.criterion;
    a.relax = rq.run.relax;
    a.tol = rq.run.tol;
    a.out = rq.out;
}

}  // namespace

// The variants' units behind launch_inference() (fused_engine.hip): k_general, k_converge, k_general_converge.  Each returns
// fused_report() of what it launched, or 0 with nothing launched.
int launch_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s);
int launch_converge(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s);
int launch_general_converge(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq,
                            hipStream_t s);
// ... and k_multilabel (fused_multilabel.hip): frames of 3 to 8 labels, a fixed count of Potts iterations; the same return value
int launch_multilabel(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq, hipStream_t s);
// ... and k_multilabel_general (fused_multilabel_general.hip): the same frames under terms with a matrix or a mode (rq.terms.general();
// kds: Engine::step_kdevs(), the matrices read from rq.terms.mats_dev); the same return value
int launch_multilabel_general(const CrfDev &c, const KernelDev *kds, const int *maxV, const int *maxRow, const SizedRequest &rq,
                              hipStream_t s);

}  // namespace lccrf

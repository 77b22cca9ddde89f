// dispatch.h -- what the engines' host sides share: the step from a run-time value to a template argument, the launch of a
// one-workgroup-per-frame kernel, and the instrumented builds' stamp buffer.
#pragma once
#include <algorithm>
#include <stdio.h>
#include <type_traits>
#include "engine.h"

namespace lccrf {
namespace {

// The one dispatch on a value known at compile time: fn(std::integral_constant<int, D>) for the D in [Lo, Hi] that equals d;
// returns whether there was one
template <int Lo, int Hi, typename Fn>
bool with_dims(int d, Fn fn)
{
    if constexpr (Lo > Hi) return false;
    else if (d == Lo) return fn(std::integral_constant<int, Lo>{}), true;
    else return with_dims<Lo + 1, Hi>(d, fn);
}

constexpr int kWorkgroupLdsMax = 160 * 1024;              // MI355X: 160 KiB of LDS per CU, one workgroup may own it all

// `grid` workgroups of `lanes` lanes and `lds_bytes` of dynamic LDS each
template <typename Kernel, typename... Args>
void launch_workgroups(Kernel fn, int grid, int lanes, int lds_bytes, hipStream_t s, const Args &...args)
{
    // (the attribute is per (function, device): cheap enough to repeat in every call, and safe with several devices in one process)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kWorkgroupLdsMax);
    fn<<<dim3(grid), dim3(lanes), lds_bytes, s>>>(args...);
}

// Instrumented builds: the shader-clock stamps of ONE workgroup's lane -- <env> = block index + 1, <env_lane> = the lane -- read
// back and printed after the launch (synchronous: debugging only).  One per engine, with static lifetime.
struct StampBuffer {
    const char *env, *env_lane, *name;
    const bool want;
    long long *buf = nullptr;
    StampBuffer(const char *e, const char *el, const char *n) : env(e), env_lane(el), name(n), want(LCCRF_INSTRUMENT != 0 && ab_env(e) != nullptr) {}
    // the three kernel arguments of a launch of `blocks` workgroups of up to `lanes` (a power of two) lanes
    void arm(int blocks, int lanes, long long **timing, int *block, int *lane)
    {
        if (want && !buf) (void)hipMalloc(&buf, 64 * sizeof(long long));
        *timing = want ? buf : nullptr;
        *block = want ? std::max(atoi(ab_env(env)) - 1, 0) : 0;
        if (*block >= blocks) *block = 0;
        *lane = (want && ab_env(env_lane)) ? atoi(ab_env(env_lane)) & (lanes - 1) : 0;
    }
    void print(hipStream_t s) const
    {
        if (!want || !buf) return;
        long long h[64];
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);
        fprintf(stderr, "[lccrf %s timing] %lld stamps, deltas (shader clocks):", name, h[63]);
        for (int i = 1; i < h[63] && i < 63; ++i) fprintf(stderr, " %lld", h[i] - h[i - 1]);
        fprintf(stderr, "\n");
    }
};

}  // namespace
}  // namespace lccrf

// stack_sorted_inst.h -- one translation unit per column capacity NP
// instantiates the sorted-path kernels for every rejection type it supports;
// sgpu_capi.cpp picks the smallest NP >= N.  Each (NP, rejection) pair has
// its own lane-group width G (E = NP/G samples per lane) and occupancy
// target W (waves per SIMD the register allocator must allow): loop-heavy
// types with data-dependent trip counts (WINSORIZED) want more pixels per
// wave to be cheap (small E) but fewer of them diverging (G > 1); straight
// rejection types want G = 1 (no cross-lane reductions at all).
#pragma once
#include "stack_sorted_impl.h"
#include "stack_sorted_gw.h"
#include "stack_wz.h"

#ifndef SGPU_WZ_TAIL_PASSES
#define SGPU_WZ_TAIL_PASSES 0   // tail passes of the split rounds: 0 by the launch's sigmas (wz_tail_passes); 1 / 2 fixed (A/B)
#endif
static_assert(SGPU_WZ_TAIL_PASSES >= 0 && SGPU_WZ_TAIL_PASSES <= 2,
              "each of the two stripe-counter sets is zeroed once per chunk and appended to by one pass");

#include <algorithm>
#include <cstdlib>

namespace sgpu {

// Real-slot variants (stack_sorted_rs*.hip): the moment path's prep kernel
// (kind 0; N > 128) and the float SIGMA / PERCENTILE / median kernels (kind =
// the rejection type) with their sort networks
// pruned to the first rs slots of every lane (rs_pick), or null when this
// NP has none (the full network runs)
using KernelFn = void (*)(KParams);
KernelFn rs_kernel_128(int kind, int xf, int rs);
// the float prep kernel at NP = 128, one lane per pixel (k_stack_wz_prep1;
// E = 128): bounds 72 .. 120 in steps of 8 and the full network (rs == 128)
KernelFn prep1_kernel_128(int xf, int rs);
int rs_pick_prep1(int N);
// the fused prep + capped rounds kernel (k_stack_wz_fused1) on the one-lane
// prep's bounds
using FusedFn = void (*)(KParams, WzSplit);
FusedFn fused1_kernel_128(int xf, int rs);
KernelFn rs_kernel_256(int kind, int xf, int rs);
KernelFn rs_kernel_512(int kind, int xf, int rs);
template <int NP> inline KernelFn rs_kernel(int kind, int xf, int rs) {
    if constexpr (NP == 128) return rs_kernel_128(kind, xf, rs);
    else if constexpr (NP == 256) return rs_kernel_256(kind, xf, rs);
    else if constexpr (NP == 512) return rs_kernel_512(kind, xf, rs);
    else return nullptr;
}
inline bool launch_fn(KernelFn f, unsigned grid, unsigned block, hipStream_t s, const KParams &p) {
    KParams k = p;
    void *args[] = {&k};
    return hipLaunchKernel((const void *)f, dim3(grid), dim3(block), args, 0, s) == hipSuccess;
}

}  // namespace sgpu

#include "stack_wz_launch.h"

namespace sgpu {

template <int NP, int G, int RT, int W, int U16 = 0>
static int launch_one(const KParams &p, hipStream_t s) {
    const long long threads = p.npix * (long long)G;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    // sort network pruned to the slots that can hold samples (rs_pick)
    constexpr int E = NP / G;
    const int rs = rs_pick(E, G, p.nframes);
    // 32-bit buffer offsets of the gather (gather_column)
    const unsigned long long es = U16 ? 2ull : 4ull;
    if ((unsigned long long)(G - 1) * (unsigned long long)p.frame_stride * es +
            (unsigned long long)p.npix * es >= 0xffffffffull)
        return 1;
    // WINSORIZED columns of 65..1024 samples (float and DATA_USHORT): the
    // moment path (stack_wz_launch.h) with the register-resident kernel over
    // its fallbacks, when the host gave it its lists and workspace.  (Float
    // NP = 128 is the one-lane prep, compiled for the N of this capacity's
    // real-slot buckets, 65..128; a smaller N takes the kernel below.)
    if constexpr (RT == WINSORIZED && NP >= 128) {
        if (p.wz_form != kWzSortedOnly && p.fb2_list && p.wz_ws && (U16 || NP > 128 || p.nframes > NP / 2))
            return wz_launch<NP, G, RT, W, U16>(p, s);
    }
    if constexpr ((RT == SIGMA || RT == PERCENTILE || RT == KMEDIAN) && !U16) {
        if (rs < E) {
            if (const KernelFn f = rs_kernel<NP>(RT, p.shiftx ? 1 : 0, rs)) return launch_fn(f, grid, 256, s, p) ? 0 : -1;
        }
    }
    if (p.shiftx)   // host sets shiftx only when shifts / normalization are needed
        hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 1, W, U16>), grid, 256, 0, s, p);
    else
        hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 0, W, U16>), grid, 256, 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sgpu

#define SGPU_CASE(NP, RT, G, W) \
    case RT: return launch_one<NP, G, RT, W>(p, s);
// GW: a macro expanding to "G, W" (tuning knobs, see the np*.hip files)
#define SGPU_CASE_I(...) SGPU_CASE(__VA_ARGS__)
#define SGPU_CASEX(NP, RT, GW) SGPU_CASE_I(NP, RT, GW)

// 16-bit (DATA_USHORT) sorted path: every rejection type and the median stack
// (LINEARFIT / GESDT single-lane, N <= 128)
#define SGPU_CASE16(NP, RT, G, W) \
    case RT: return launch_one<NP, G, RT, W, 1>(p, s);
#define SGPU_CASE16_I(...) SGPU_CASE16(__VA_ARGS__)
#define SGPU_CASE16X(NP, RT, GW) SGPU_CASE16_I(NP, RT, GW)

// returns 0 launched, 1 not on the sorted path (exact kernel), -1 launch error
#define SGPU_DEFINE_SORTED_LAUNCHER(NP, CASES)                                 \
    namespace sgpu {                                                           \
    int launch_sorted_##NP(const KParams &p, hipStream_t s) {                  \
        switch (p.rtype) {                                                     \
            CASES                                                              \
            default:                                                           \
                return 1;                                                      \
        }                                                                      \
    }                                                                          \
    }

#define SGPU_DEFINE_SORTED16_LAUNCHER(NP, CASES)                              \
    namespace sgpu {                                                           \
    int launch_sorted16_##NP(const KParams &p, hipStream_t s) {                \
        switch (p.rtype) {                                                     \
            CASES                                                              \
            default:                                                           \
                return 1;                                                      \
        }                                                                      \
    }                                                                          \
    }

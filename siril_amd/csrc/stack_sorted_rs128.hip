// stack_sorted_rs128.hip -- real-slot variants for N <= 128 (see
// stack_sorted_inst.h rs_kernel): the moment path's prep kernel (two lanes
// per pixel: E = 64 slots per lane, bounds 36..60 in steps of 4; four lanes
// per pixel: E = 32, bounds 20..28 and the full network; one lane per pixel:
// E = 128, bounds 72..120 in steps of 8 and the full network) and the float SIGMA,
// PERCENTILE and median kernels
// (E = 128, bounds 72..120 in steps of 8) whose sort networks leave out every comparator on a slot that
// only padding can occupy (oem_sort's RS).  Measured (profiles/r04q_ab_real_slots.txt):
// config 2 14.59 -> 13.69 ms, sigma400 43.56 -> 41.68 ms.
#include "stack_sorted_inst.h"
#include "stack_sorted_gw.h"

namespace sgpu {
namespace {
template <int NP, int G, int W, int RS>
KernelFn prep_rs(int xf, int rs) {
    if constexpr (RS >= NP / G) {
        return nullptr;
    } else {
        if (rs == RS) return xf ? &k_stack_wz_prep<NP, G, 1, W, RS> : &k_stack_wz_prep<NP, G, 0, W, RS>;
        return prep_rs<NP, G, W, RS + 4>(xf, rs);
    }
}
// four lanes per pixel (prep4_kernel_128): bounds RS, RS + STEP, .. < 32, then 32
template <int W, int RS, int STEP>
KernelFn prep4(int xf, int rs) {
    constexpr int R = RS < 32 ? RS : 32;
    if (rs == R || R == 32) return xf ? &k_stack_wz_prep<128, 4, 1, W, R> : &k_stack_wz_prep<128, 4, 0, W, R>;
    if constexpr (R < 32) return prep4<W, RS + STEP, STEP>(xf, rs);
    return nullptr;
}
// one lane per pixel (prep1_kernel_128): bounds RS, RS + 8, .. < 128, then 128
template <int W, int RS>
KernelFn prep1(int xf, int rs) {
    if (rs == RS || RS == 128) return xf ? &k_stack_wz_prep1<128, 1, W, RS> : &k_stack_wz_prep1<128, 0, W, RS>;
    if constexpr (RS < 128) return prep1<W, RS + 8>(xf, rs);
    return nullptr;
}
// the fused kernel on the same bounds (fused1_kernel_128)
template <int W, int RS>
FusedFn fused1(int xf, int rs) {
    if (rs == RS || RS == 128) return xf ? &k_stack_wz_fused1<128, 1, W, RS> : &k_stack_wz_fused1<128, 0, W, RS>;
    if constexpr (RS < 128) return fused1<W, RS + 8>(xf, rs);
    return nullptr;
}
template <int NP, int RT, int G, int W, int RS>
KernelFn straight_rs(int xf, int rs) {
    constexpr int E = NP / G;
    if constexpr (RS >= E) {
        return nullptr;
    } else {
        if (rs == RS)
            return xf ? &k_stack_sorted<NP, G, RT, 1, W, 0, 0, RS> : &k_stack_sorted<NP, G, RT, 0, W, 0, 0, RS>;
        return straight_rs<NP, RT, G, W, RS + (E == 64 ? 4 : 8)>(xf, rs);
    }
}
}  // namespace

KernelFn rs_kernel_128(int kind, int xf, int rs) {
    switch (kind) {
        case 0: return prep_rs<128, 2, SGPU_WZ_PREP_W128_G2, 36>(xf, rs);
        case SIGMA: return straight_rs<128, SIGMA, SGPU_GW128, 72>(xf, rs);
        case PERCENTILE: return straight_rs<128, PERCENTILE, SGPU_GW128, 72>(xf, rs);
        case KMEDIAN: return straight_rs<128, KMEDIAN, SGPU_GW128, 72>(xf, rs);
        default: return nullptr;
    }
}

KernelFn prep4_kernel_128(int xf, int rs) { return prep4<SGPU_WZ_PREP_W128, SGPU_WZ_PREP4_RS0, SGPU_WZ_PREP4_RSSTEP>(xf, rs); }

// real-slot bound of the four-lane prep: the smallest compiled bound >=
// ceil(N / 4), or 32 (the full network)
int rs_pick_prep4(int N) {
    const int need = (N + 3) / 4;
    for (int rs = SGPU_WZ_PREP4_RS0; rs < 32; rs += SGPU_WZ_PREP4_RSSTEP)
        if (rs >= need) return rs;
    return 32;
}

KernelFn prep1_kernel_128(int xf, int rs) { return prep1<SGPU_WZ_PREP_W128_G1, 72>(xf, rs); }
FusedFn fused1_kernel_128(int xf, int rs) { return fused1<SGPU_WZ_FUSED_W128, 72>(xf, rs); }

// real-slot bound of the one-lane prep: rs_pick's steps of 8 (N in [rs - 7,
// rs], which k_stack_wz_prep1's compile-time slot ranges rest on), from 72
int rs_pick_prep1(int N) {
    const int rs = rs_pick(128, 1, N);
    return rs < 72 ? 72 : rs;
}
}  // namespace sgpu

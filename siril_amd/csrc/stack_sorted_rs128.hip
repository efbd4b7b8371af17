// stack_sorted_rs128.hip -- real-slot variants for N <= 128 (see
// stack_sorted_inst.h rs_kernel): the moment path's float prep kernel (one
// lane per pixel: E = 128, bounds 72..120 in steps of 8 and the full
// network), the fused prep + rounds kernel on the same bounds, and the float
// SIGMA, PERCENTILE and median kernels
// (E = 128, bounds 72..120 in steps of 8) whose sort networks leave out every comparator on a slot that
// only padding can occupy (oem_sort's RS).  Measured (profiles/r04q_ab_real_slots.txt):
// config 2 14.59 -> 13.69 ms, sigma400 43.56 -> 41.68 ms.
#include "stack_sorted_inst.h"
#include "stack_sorted_gw.h"

namespace sgpu {
namespace {
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
        case SIGMA: return straight_rs<128, SIGMA, SGPU_GW128, 72>(xf, rs);
        case PERCENTILE: return straight_rs<128, PERCENTILE, SGPU_GW128, 72>(xf, rs);
        case KMEDIAN: return straight_rs<128, KMEDIAN, SGPU_GW128, 72>(xf, rs);
        default: return nullptr;
    }
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

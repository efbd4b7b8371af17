// Microbenchmark: the FP64 VALU issue rate of gfx950 as a register-only
// multiply / add loop (v_mul_f64, v_add_f64; nothing contracted), 8
// independent chains per lane.  scripts/subsky_rbf_bench.py compiles this to a
// code object (hipcc --genco -ffp-contract=off), loads it into its own process
// and times it at 8 waves per SIMD: the yardstick of k_bkg_rbf_apply_vec.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

// 16 FP64 instructions per lane and iteration
extern "C" __global__ __launch_bounds__(256) void k_fp64_rate(double *out, double a, double b, int iters) {
    double d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = 1.0 + (double)threadIdx.x * 1e-9 + (double)i * 1e-3;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            d[i] = d[i] * a;
            d[i] = d[i] + b;
        }
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) s += d[i];
    if (s == 12345.0) out[threadIdx.x] = s;      // never true: keeps the loop alive
}

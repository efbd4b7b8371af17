// stretch_paths.hip -- one straight-line kernel per stretch that
// scripts/stretch_bench.py times, with the function, the form of q, the colour
// model and the clip mode as compile-time constants, so that the FP64 VALU
// instructions a sample costs on that path can be counted in the ISA:
//   hipcc -S --offload-device-only --offload-arch=gfx950 -O3 -ffp-contract=off -I siril_amd/csrc \
//       scripts/micro/stretch_paths.hip -o stretch_paths.s
// and, per kernel, the lines that match v_[a-z0-9_]*_f64 between its label and
// its s_endpgm.  The kernel of siril_amd/csrc/stretch.hip runs the same
// inlined functions behind scalar branches on its arguments.
#include <hip/hip_runtime.h>

#include "stretch_host.h"

#pragma clang fp contract(off)

using namespace sgpu_str_host;

template <int FN, int REGIME, int MODEL, int CLIPMODE>
__device__ __forceinline__ StrCoef coef(const double *c) {
    StrCoef k;
    for (int i = 0; i < SGPU_STRETCH_NCOEF; i++) k.c[i] = c[i];
    k.fn = FN, k.regime = REGIME, k.model = MODEL, k.clipmode = CLIPMODE, k.mask = 7;
    return k;
}

template <int FN, int REGIME>
__device__ __forceinline__ void one(const double *c, const float *in, float *out) {
    const StrCoef k = coef<FN, REGIME, 0, 0>(c);
    const int i = blockIdx.x * 256 + threadIdx.x;
    out[i] = (float)str_sample(k, str_widen(in[i]));
}

template <int FN, int REGIME, int MODEL, int CLIPMODE>
__device__ __forceinline__ void three(const double *c, const float *in, float *out, int n) {
    const StrCoef k = coef<FN, REGIME, MODEL, CLIPMODE>(c);
    const int i = blockIdx.x * 256 + threadIdx.x;
    double x[3], o[3];
    for (int ch = 0; ch < 3; ch++) x[ch] = str_widen(in[ch * n + i]);
    str_pixel3(k, x, o);
    for (int ch = 0; ch < 3; ch++) out[ch * n + i] = (float)o[ch];
}

extern "C" __global__ void k_path_mtf(const double *c, const float *in, float *out) {
    one<SGPU_STRETCH_MTF, 0>(c, in, out);
}
extern "C" __global__ void k_path_ght_pos(const double *c, const float *in, float *out) {
    one<SGPU_STRETCH_GHT, Q_POS>(c, in, out);
}
extern "C" __global__ void k_path_invght_pos(const double *c, const float *in, float *out) {
    one<SGPU_STRETCH_INVGHT, Q_POS>(c, in, out);
}
extern "C" __global__ void k_path_asinh_mono(const double *c, const float *in, float *out) {
    one<SGPU_STRETCH_ASINH, 0>(c, in, out);
}
// per pixel of three samples; rgbblend's per-channel transfers, which only clipping pixels run, are in the count
extern "C" __global__ void k_path_ght_pos_human_rgbblend(const double *c, const float *in, float *out, int n) {
    three<SGPU_STRETCH_GHT, Q_POS, SGPU_STRETCH_HUMAN, SGPU_STRETCH_RGBBLEND>(c, in, out, n);
}
extern "C" __global__ void k_path_ght_pos_human_clip(const double *c, const float *in, float *out, int n) {
    three<SGPU_STRETCH_GHT, Q_POS, SGPU_STRETCH_HUMAN, SGPU_STRETCH_CLIP>(c, in, out, n);
}
extern "C" __global__ void k_path_asinh_colour(const double *c, const float *in, float *out, int n) {
    three<SGPU_STRETCH_ASINH, 0, SGPU_STRETCH_EVEN, 0>(c, in, out, n);
}

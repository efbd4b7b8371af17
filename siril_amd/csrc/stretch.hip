// stretch.hip -- the non-linear stretches (`mtf`, `autostretch`, `linstretch`,
// `asinh`, `ght`, `invght`, `modasinh`, `invmodasinh`) of planes resident in
// HBM: one streaming pass.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// stretches are specified in DESIGN.md 6m (T0-T9), live in stretch_host.h and
// are restated in tests/stretch_ref.py; that restatement is the contract.
// Parity with a Siril binary is unpinned.
//
// One launch per parameter block, the coefficient block (T6, computed once on
// the host by the same header) in the kernel's arguments, so every choice of
// function, form of q, colour model and clip mode is the same in every lane
// and costs a scalar branch.  The piece of S is chosen without a branch (T7):
// every lane of a wavefront runs the same log / exp.
//   k_stretch<T, false>  a plane per blockIdx.y; sample by sample.
//   k_stretch<T, true>   an image of three planes per blockIdx.y: a pixel's
//                        three samples are read together, so the luminance
//                        never goes through memory; rgbblend's per-channel
//                        transfer runs only where a channel passes 1.
// Each lane handles four consecutive samples with one 16-byte load (8 bytes
// for WORD input) per plane and one 16-byte store.  A plane that does not
// start on a 16-byte boundary (H*W odd) has a head of up to three samples
// before its first whole vector and a tail after its last one, handled sample
// by sample; when the input and the output (and, for three planes together,
// the planes among themselves) do not share that head, the whole plane is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "sgpu_internal.h"
#include "stretch_host.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_str_host;

namespace sgpu {

constexpr int STR_BLOCK = 256, STR_MAX_BLOCKS = 4096;

struct StrArgs {
    StrCoef k;
    const void *in;         // T samples, plane p of the launch at in + p*in_ps
    long long in_ps;
    float *out;             // plane p at out + p*out_ps
    long long out_ps;
    long long npix;
    int masked;             // planes are the channels of three-channel images: k.mask applies
    int chan0;              // channel of the launch's first plane
};

template <typename T, bool JOINT>
__device__ __forceinline__ void str_one(const StrArgs &a, bool sel, const T *x, float *o) {
    if constexpr (JOINT) {
        double xw[3], r[3];
#pragma unroll
        for (int c = 0; c < 3; c++) xw[c] = str_widen(x[c]);
        str_pixel3(a.k, xw, r);
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = (a.k.mask >> c & 1) ? (float)r[c] : (float)xw[c];
    } else {
        const double xw = str_widen(x[0]);
        o[0] = sel ? (float)str_sample(a.k, xw) : (float)xw;
    }
}

template <typename T, bool JOINT>
__global__ __launch_bounds__(STR_BLOCK) void k_stretch(const StrArgs a) {
    constexpr int NC = JOINT ? 3 : 1;
    using V = std::conditional_t<sizeof(T) == 4, float4, ushort4>;
    const long long g = blockIdx.y;
    const T *in[NC];
    float *out[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        in[c] = static_cast<const T *>(a.in) + (g * NC + c) * a.in_ps;
        out[c] = a.out + (g * NC + c) * a.out_ps;
    }
    const bool sel = JOINT || !a.masked || (a.k.mask >> ((a.chan0 + (int)g) % 3) & 1);
    // the head: samples before the first 16-byte boundary of the output
    long long h = (long long)((4 - (((uintptr_t)out[0] >> 2) & 3)) & 3);
    h = h < a.npix ? h : a.npix;
    bool vec = true;
#pragma unroll
    for (int c = 0; c < NC; c++)
        vec = vec && ((uintptr_t)(out[c] + h) & 15) == 0 && ((uintptr_t)(in[c] + h) & (sizeof(V) - 1)) == 0;
    h = vec ? h : 0;
    const long long nvec = vec ? (a.npix - h) >> 2 : 0;
    const long long stride = (long long)gridDim.x * STR_BLOCK, first = (long long)blockIdx.x * STR_BLOCK + threadIdx.x;
    for (long long v = first; v < nvec; v += stride) {
        const long long j = h + 4 * v;
        V xv[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) xv[c] = *reinterpret_cast<const V *>(in[c] + j);
        float4 ov[NC];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            T x[NC];
            float o[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) x[c] = e == 0 ? xv[c].x : e == 1 ? xv[c].y : e == 2 ? xv[c].z : xv[c].w;
            str_one<T, JOINT>(a, sel, x, o);
#pragma unroll
            for (int c = 0; c < NC; c++) (e == 0 ? ov[c].x : e == 1 ? ov[c].y : e == 2 ? ov[c].z : ov[c].w) = o[c];
        }
#pragma unroll
        for (int c = 0; c < NC; c++) *reinterpret_cast<float4 *>(out[c] + j) = ov[c];
    }
    // the head and the tail, or the whole plane
    const long long ns = a.npix - 4 * nvec;
    for (long long s = first; s < ns; s += stride) {
        const long long j = s < h ? s : s + 4 * nvec;
        T x[NC];
        float o[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) x[c] = in[c][j];
        str_one<T, JOINT>(a, sel, x, o);
#pragma unroll
        for (int c = 0; c < NC; c++) out[c][j] = o[c];
    }
}

}  // namespace sgpu

// ===================================================================== host
namespace {

// true when the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const char *a0 = (const char *)a, *b0 = (const char *)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

template <typename T>
void launch(sgpu_context *c, const sgpu::StrArgs &a, int nplanes, bool joint) {
    const long long nv = (a.npix + 3) / 4, nb = (nv + sgpu::STR_BLOCK - 1) / sgpu::STR_BLOCK;
    const unsigned gx = (unsigned)std::max(1LL, std::min(nb, (long long)sgpu::STR_MAX_BLOCKS));
    if (joint)
        hipLaunchKernelGGL((sgpu::k_stretch<T, true>), dim3(gx, (unsigned)(nplanes / 3)), dim3(sgpu::STR_BLOCK), 0,
                           c->stream, a);
    else
        hipLaunchKernelGGL((sgpu::k_stretch<T, false>), dim3(gx, (unsigned)nplanes), dim3(sgpu::STR_BLOCK), 0,
                           c->stream, a);
}

}  // namespace

extern "C" int sgpu_stretch_check(const sgpu_stretch_params *p) {
    if (!p) return fail(SGPU_BAD_ARGUMENT, "stretch: no parameters");
    if (const char *why = str_check(*p)) return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_stretch_coeffs(const sgpu_stretch_params *p, double *coeffs) {
    if (!p || !coeffs) return fail(SGPU_BAD_ARGUMENT, "stretch_coeffs: null argument");
    StrCoef k;
    if (const char *why = str_coeffs(*p, &k)) return fail(SGPU_BAD_ARGUMENT, why);
    for (int i = 0; i < SGPU_STRETCH_NCOEF; i++) coeffs[i] = k.c[i];
    return SGPU_OK;
}

extern "C" int sgpu_autostretch_params(const double *stats, const int *status, int nimages, int nchannels, double unit,
                                       int linked, double shadows_clip, double target_bg, double *out) {
    if (const char *why = str_autostretch(stats, status, nimages, nchannels, unit, linked, shadows_clip, target_bg, out))
        return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_stretch_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nimages, int nchannels,
                                          int width, int height, long plane_stride, const sgpu_stretch_params *params,
                                          int nparams, float *d_out, long out_stride) {
    if (!c) return fail(SGPU_BAD_ARGUMENT, "stretch: no context");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "stretch: element size must be 2 or 4");
    if (width < 1 || height < 1) return fail(SGPU_BAD_ARGUMENT, "stretch: empty plane");
    if (nimages < 0 || nchannels < 1 || (long long)nimages * nchannels > 65535)
        return fail(SGPU_BAD_ARGUMENT, "stretch: bad number of planes");
    const long long npix = (long long)width * height;
    const int nplanes = nimages * nchannels;
    if (plane_stride < npix) return fail(SGPU_BAD_ARGUMENT, "stretch: plane_stride < width*height");
    if (out_stride < npix) return fail(SGPU_BAD_ARGUMENT, "stretch: out_stride < width*height");
    if (!params || (nparams != 1 && nparams != nimages && nparams != nplanes))
        return fail(SGPU_BAD_ARGUMENT, "stretch: one parameter block per call, per image or per plane");
    const int group = nparams == 1 ? nplanes : nparams == nimages ? nchannels : 1;
    std::vector<StrCoef> ks((size_t)nparams);
    for (int b = 0; b < nparams; b++) {
        if (const char *why = str_coeffs(params[b], &ks[(size_t)b])) return fail(SGPU_BAD_ARGUMENT, why);
        if (group < nchannels && str_joint(ks[(size_t)b], nchannels))
            return fail(SGPU_BAD_ARGUMENT, "stretch: a luminance model needs one parameter block per image, not per plane");
    }
    c->str_launches = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "stretch: null planes");
    if (overlaps(d_in, ((size_t)(nplanes - 1) * plane_stride + npix) * elem_size, d_out,
                 ((size_t)(nplanes - 1) * out_stride + npix) * sizeof(float)))
        return fail(SGPU_BAD_ARGUMENT, "stretch: the output overlaps the input");
    HIP_TRY(hipSetDevice(c->device));
    for (hipEvent_t &e : c->str_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->str_ev[0], c->stream));
    for (int b = 0; b < nparams; b++) {
        const long long p0 = (long long)b * group;
        sgpu::StrArgs a = {};
        a.k = ks[(size_t)b];
        a.in = (const char *)d_in + (size_t)p0 * plane_stride * elem_size;
        a.in_ps = plane_stride;
        a.out = d_out + (size_t)p0 * out_stride;
        a.out_ps = out_stride;
        a.npix = npix;
        a.masked = nchannels == 3;
        a.chan0 = (int)(p0 % nchannels);
        const bool joint = str_joint(a.k, nchannels);
        if (elem_size == 2)
            launch<uint16_t>(c, a, group, joint);
        else
            launch<float>(c, a, group, joint);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->str_ev[1], c->stream));
    c->str_launches = nparams;
    return SGPU_OK;
}

extern "C" int sgpu_stretch_last_kernel_ms(sgpu_context *c, float *ms, int *nlaunches) {
    if (!c || !ms || !nlaunches) return fail(SGPU_BAD_ARGUMENT, "stretch_last_kernel_ms: null argument");
    *nlaunches = c->str_launches;
    *ms = 0.0f;
    if (!c->str_launches) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->str_ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, c->str_ev[0], c->str_ev[1]));
    return SGPU_OK;
}

// epf.hip -- the edge-preserving filter (`epf -guided`: a guided filter,
// steered by the image itself or by a second image) of planes resident in
// HBM: d x d windows, d odd in 3 .. 25.  The bilateral filter of `epf` is
// specified next to it but not built: a kernel of it ran at the FP64 issue
// limit and still took 1.3 times fmedian's selection at the same window
// (DESIGN.md 6n), so mode 0 is refused.
//
// PARITY STATUS: Siril computes `epf` with OpenCV, which was not available to
// check against.  The filter is specified in DESIGN.md 6n (E0-E7), lives in
// epf_host.h and is restated in tests/epf_ref.py; that restatement is the
// contract, held bit for bit.  Parity with a Siril binary is unpinned.
//
// One workgroup of 256 per tile of 64 x 32 pixels (64 x 16 above d = 17, where
// two staged planes and the row sums would not fit 64 KB of LDS): the tile and
// a halo of r, reflected at load and widened to whole quads left and right, in
// LDS; lane t owns, in each pass over the tile's rows, four neighbouring pixels
// of a row and stores them as one quad.  d is a runtime bound.
//   k_epf_guided_a<T, G, VEC>      a and b.  Per quantity (I, I I, p, I p; two
//                  of them when the input guides itself) the row sums of every
//                  tile row go through LDS once, then every pixel adds its
//                  2r + 1 of them top to bottom.
//   k_epf_guided_b<TI, TP, VEC>    box(a) I + box(b) in the same way.
// Global accesses are 16 bytes per lane (8 for WORD input) when the width, the
// pointers and the strides are multiples of four samples / 16 bytes, and one
// sample per access otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "epf_host.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_epf_host;

namespace sgpu {

constexpr int EPF_TILE = 64, EPF_TILE_H = 32, EPF_TILE_H_WIDE = 16, EPF_WIDE_R = 8;

struct EpfArgs {
    const void *in;         // T samples, plane p at in + p*in_ps
    long long in_ps;
    const void *guide;      // G samples, plane p at guide + p*g_ps
    long long g_ps;
    float *a, *b;           // guided: the coefficient planes, plane p at a + p*ab_ps
    long long ab_ps;
    float *out;             // plane p at out + p*out_ps
    long long out_ps;
    double eps, inv_n;
    float modulation;
    int W, H, r, th;        // th: the tile's height
};

// the tile's geometry: the halo is widened to whole quads on the left and the right, so that every quad of the
// plane is a quad of the tile
struct EpfGeom {
    int r, d, R4, PITCH, ROWS, QROW, OFF;
    __device__ __host__ EpfGeom(int r_, int th) {
        r = r_, d = 2 * r + 1, R4 = (r + 3) & ~3;
        PITCH = EPF_TILE + 2 * R4 + 4;      // one quad of padding spreads the rows over the banks
        ROWS = th + 2 * r;
        QROW = (EPF_TILE + 2 * R4) / 4;
        OFF = R4 - r;                       // of a window's first column in the quads of its pixel
    }
};

template <typename T>
using EpfQuad = std::conditional_t<sizeof(T) == 4, float4, ushort4>;

// The tile (tx0, ty0) of one plane and its halo into s, reflected (E1) at load; conv makes an LDS element of a
// sample.  Past the reflection's reach (columns and rows no window of this tile reads) the index is only kept
// inside the plane.
template <typename T, bool VEC, typename E, class Conv>
__device__ __forceinline__ void epf_load_tile(const T *src, int W, int H, E *s, const EpfGeom &g, int tx0, int ty0,
                                              Conv conv) {
    const int total = g.QROW * g.ROWS;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int ly = i / g.QROW, q = i - ly * g.QROW, gx = tx0 - g.R4 + 4 * q;
        const T *row = src + (long long)min(max(wav_refl(ty0 - g.r + ly, H), 0), H - 1) * W;
        E *dst = s + ly * g.PITCH + 4 * q;
        if (VEC && gx >= 0 && gx + 3 < W) {
            const EpfQuad<T> v = *reinterpret_cast<const EpfQuad<T> *>(row + gx);
            dst[0] = conv(v.x), dst[1] = conv(v.y), dst[2] = conv(v.z), dst[3] = conv(v.w);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) dst[e] = conv(row[min(max(wav_refl(gx + e, W), 0), W - 1)]);
        }
    }
}

// the four samples at (x .. x+3, y) of a plane
template <typename T, bool VEC>
__device__ __forceinline__ void epf_read4(const T *plane, int W, int x, int y, T (&v)[4]) {
    const T *at = plane + (long long)y * W + x;
    if constexpr (VEC) {
        const EpfQuad<T> q = *reinterpret_cast<const EpfQuad<T> *>(at);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = x + e < W ? at[e] : T(0);
    }
}

template <bool VEC>
__device__ __forceinline__ void epf_write4(float *plane, int W, int x, int y, const float (&o)[4]) {
    float *dst = plane + (long long)y * W + x;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (x + e < W) dst[e] = o[e];
    }
}

// --------------------------------------------------------------------- guided
// A staged sample is kept as its own 32 bits (a WORD as the integer) and widened where it is read.
template <typename T>
__device__ __forceinline__ uint32_t epf_stage(T v) {
    if constexpr (sizeof(T) == 4)
        return __float_as_uint(v);
    else
        return (uint32_t)v;
}
template <typename T>
__device__ __forceinline__ double epf_staged(uint32_t u) {
    if constexpr (sizeof(T) == 4)
        return str_widen(__uint_as_float(u));
    else
        return str_widen((uint16_t)u);
}

// box(f) of the lane's pixels, E3's sums: first the row sums of every row of the tile and its halo, each added
// left to right by one lane for four neighbouring pixels (a sliding set of four samples) and left in rs; then every
// pixel adds the 2r + 1 row sums of its column top to bottom.  f(ly, j) is the sample j columns right of the
// window's first one of the lane's first pixel, row ly of the LDS.  res[i][e] is pixel e of the lane's pass i.
template <class F>
__device__ __forceinline__ void epf_box(F f, double *rs, const EpfGeom &g, int th, double inv_n, double (&res)[2][4]) {
    __syncthreads();        // rs is free, and the staged planes are complete
    for (int i = threadIdx.x; i < g.ROWS * 16; i += 256) {
        const int ly = i >> 4, q = i & 15;
        double w0 = f(ly, q, 0), w1 = f(ly, q, 1), w2 = f(ly, q, 2), w3 = f(ly, q, 3);
        double s0 = w0, s1 = w1, s2 = w2, s3 = w3;
#pragma unroll 1
        for (int j = 1; j < g.d; j++) {
            w0 = w1, w1 = w2, w2 = w3, w3 = f(ly, q, j + 3);
            s0 = s0 + w0, s1 = s1 + w1, s2 = s2 + w2, s3 = s3 + w3;
        }
        double *dst = rs + ly * EPF_TILE + 4 * q;
        dst[0] = s0, dst[1] = s1, dst[2] = s2, dst[3] = s3;
    }
    __syncthreads();
    const int qi = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ty = (threadIdx.x >> 4) + 16 * i;
        if (ty >= th) continue;
        const double *col = rs + ty * EPF_TILE + 4 * qi;
        double acc[4];
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = col[e];
#pragma unroll 1
        for (int dy = 1; dy < g.d; dy++) {
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] = acc[e] + col[dy * EPF_TILE + e];
        }
#pragma unroll
        for (int e = 0; e < 4; e++) res[i][e] = acc[e] * inv_n;
    }
}

// G is void when the input guides itself: the plane is staged once and mI, cII stand for mp, cIp
template <typename T, typename G, bool VEC>
__global__ __launch_bounds__(256) void k_epf_guided_a(const EpfArgs a) {
    constexpr bool SELF = std::is_void_v<G>;
    using TI = std::conditional_t<SELF, T, G>;
    extern __shared__ __attribute__((aligned(16))) unsigned char epf_smem[];
    const EpfGeom g(a.r, a.th);
    uint32_t *sp = reinterpret_cast<uint32_t *>(epf_smem), *sI = SELF ? sp : sp + g.ROWS * g.PITCH;
    double *rs = reinterpret_cast<double *>(sp + (SELF ? 1 : 2) * g.ROWS * g.PITCH);
    const int tx0 = blockIdx.x * EPF_TILE, ty0 = blockIdx.y * a.th, p = blockIdx.z;
    epf_load_tile<T, VEC>(static_cast<const T *>(a.in) + (long long)p * a.in_ps, a.W, a.H, sp, g, tx0, ty0,
                          [](T v) { return epf_stage(v); });
    if constexpr (!SELF)
        epf_load_tile<TI, VEC>(static_cast<const TI *>(a.guide) + (long long)p * a.g_ps, a.W, a.H, sI, g, tx0, ty0,
                               [](TI v) { return epf_stage(v); });
    auto at = [&g](int ly, int q, int j) { return ly * g.PITCH + g.OFF + 4 * q + j; };
    auto fI = [&](int ly, int q, int j) { return epf_staged<TI>(sI[at(ly, q, j)]); };
    auto fp = [&](int ly, int q, int j) { return epf_staged<T>(sp[at(ly, q, j)]); };
    auto fII = [&](int ly, int q, int j) {
        const double v = epf_staged<TI>(sI[at(ly, q, j)]);
        return v * v;
    };
    auto fIp = [&](int ly, int q, int j) {
        const double v = epf_staged<TI>(sI[at(ly, q, j)]), u = epf_staged<T>(sp[at(ly, q, j)]);
        return v * u;
    };
    double mI[2][4], mp[2][4], cII[2][4], cIp[2][4];
    epf_box(fI, rs, g, a.th, a.inv_n, mI);
    epf_box(fII, rs, g, a.th, a.inv_n, cII);
    if constexpr (!SELF) {
        epf_box(fp, rs, g, a.th, a.inv_n, mp);
        epf_box(fIp, rs, g, a.th, a.inv_n, cIp);
    }
    const int qi = threadIdx.x & 15, x = tx0 + 4 * qi;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ty = (threadIdx.x >> 4) + 16 * i, y = ty0 + ty;
        if (ty >= a.th || y >= a.H || x >= a.W) continue;
        float fa[4], fb[4];
#pragma unroll
        for (int e = 0; e < 4; e++)
            epf_coeffs(mI[i][e], SELF ? mI[i][e] : mp[i][e], cII[i][e], SELF ? cII[i][e] : cIp[i][e], a.eps, &fa[e],
                       &fb[e]);
        epf_write4<VEC>(a.a + (long long)p * a.ab_ps, a.W, x, y, fa);
        epf_write4<VEC>(a.b + (long long)p * a.ab_ps, a.W, x, y, fb);
    }
}

// a.guide is the guide or, when the input guides itself, the input; the input is read only for E4
template <typename TI, typename TP, bool VEC>
__global__ __launch_bounds__(256) void k_epf_guided_b(const EpfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char epf_smem[];
    const EpfGeom g(a.r, a.th);
    uint32_t *sa = reinterpret_cast<uint32_t *>(epf_smem), *sb = sa + g.ROWS * g.PITCH;
    double *rs = reinterpret_cast<double *>(sa + 2 * g.ROWS * g.PITCH);
    const int tx0 = blockIdx.x * EPF_TILE, ty0 = blockIdx.y * a.th, p = blockIdx.z;
    epf_load_tile<float, VEC>(a.a + (long long)p * a.ab_ps, a.W, a.H, sa, g, tx0, ty0,
                              [](float v) { return epf_stage(v); });
    epf_load_tile<float, VEC>(a.b + (long long)p * a.ab_ps, a.W, a.H, sb, g, tx0, ty0,
                              [](float v) { return epf_stage(v); });
    auto at = [&g](int ly, int q, int j) { return ly * g.PITCH + g.OFF + 4 * q + j; };
    double ma[2][4], mb[2][4];
    epf_box([&](int ly, int q, int j) { return (double)__uint_as_float(sa[at(ly, q, j)]); }, rs, g, a.th, a.inv_n, ma);
    epf_box([&](int ly, int q, int j) { return (double)__uint_as_float(sb[at(ly, q, j)]); }, rs, g, a.th, a.inv_n, mb);
    const int qi = threadIdx.x & 15, x = tx0 + 4 * qi;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ty = (threadIdx.x >> 4) + 16 * i, y = ty0 + ty;
        if (ty >= a.th || y >= a.H || x >= a.W) continue;
        TI I[4];
        epf_read4<TI, VEC>(static_cast<const TI *>(a.guide) + (long long)p * a.g_ps, a.W, x, y, I);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = epf_guided_out(ma[i][e], mb[i][e], str_widen(I[e]));
        if (a.modulation != 1.0f) {
            TP pv[4];
            epf_read4<TP, VEC>(static_cast<const TP *>(a.in) + (long long)p * a.in_ps, a.W, x, y, pv);
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = med_modulate(a.modulation, o[e], epf_centre(pv[e]));
        }
        epf_write4<VEC>(a.out + (long long)p * a.out_ps, a.W, x, y, o);
    }
}

}  // namespace sgpu

// ===================================================================== host
namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// true when the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const char *a0 = (const char *)a, *b0 = (const char *)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

dim3 epf_grid(const sgpu::EpfArgs &a, int P) {
    return dim3((unsigned)((a.W + sgpu::EPF_TILE - 1) / sgpu::EPF_TILE), (unsigned)((a.H + a.th - 1) / a.th), (unsigned)P);
}

template <typename T, typename G, bool VEC>
void launch_a(sgpu_context *c, const sgpu::EpfArgs &a, int P) {
    const sgpu::EpfGeom g(a.r, a.th);
    const size_t lds = (size_t)(std::is_void_v<G> ? 1 : 2) * g.ROWS * g.PITCH * 4 + (size_t)g.ROWS * sgpu::EPF_TILE * 8;
    hipLaunchKernelGGL((sgpu::k_epf_guided_a<T, G, VEC>), epf_grid(a, P), dim3(256), lds, c->stream, a);
}

template <typename TI, typename TP, bool VEC>
void launch_b(sgpu_context *c, const sgpu::EpfArgs &a, int P) {
    const sgpu::EpfGeom g(a.r, a.th);
    const size_t lds = (size_t)2 * g.ROWS * g.PITCH * 4 + (size_t)g.ROWS * sgpu::EPF_TILE * 8;
    hipLaunchKernelGGL((sgpu::k_epf_guided_b<TI, TP, VEC>), epf_grid(a, P), dim3(256), lds, c->stream, a);
}

// gs is the guide's element size, 0 when the input guides itself
template <typename T, bool VEC>
void launch_a_g(sgpu_context *c, const sgpu::EpfArgs &a, int P, int gs) {
    if (gs == 0) return launch_a<T, void, VEC>(c, a, P);
    if (gs == 2) return launch_a<T, uint16_t, VEC>(c, a, P);
    return launch_a<T, float, VEC>(c, a, P);
}
template <typename TP, bool VEC>
void launch_b_g(sgpu_context *c, const sgpu::EpfArgs &a, int P, int is) {
    if (is == 2) return launch_b<uint16_t, TP, VEC>(c, a, P);
    return launch_b<float, TP, VEC>(c, a, P);
}

template <bool VEC>
void launch_all(sgpu_context *c, sgpu::EpfArgs &a, int P, int es, int gs, int step) {
    if (step == 0) {
        if (es == 2) return launch_a_g<uint16_t, VEC>(c, a, P, gs);
        return launch_a_g<float, VEC>(c, a, P, gs);
    }
    // pass B reads I through a.guide
    sgpu::EpfArgs b = a;
    if (gs == 0) b.guide = a.in, b.g_ps = a.in_ps;
    if (es == 2) return launch_b_g<uint16_t, VEC>(c, b, P, gs ? gs : es);
    return launch_b_g<float, VEC>(c, b, P, gs ? gs : es);
}

}  // namespace

extern "C" int sgpu_epf_check(int width, int height, int mode, int d, double si, double ss, float modulation) {
    if (const char *why = epf_check(width, height, mode, d, si, ss, modulation)) return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_epf_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width, int height,
                                      long plane_stride, const void *d_guide, int guide_elem_size, long guide_stride,
                                      int mode, int d, double si, double ss, float modulation, float *d_out,
                                      long out_stride) {
    if (!c) return fail(SGPU_BAD_ARGUMENT, "epf: no context");
    c->epf_launches = 0;        // the timing hook describes this call, refused or not
    if (const char *why = epf_check(width, height, mode, d, si, ss, modulation)) return fail(SGPU_BAD_ARGUMENT, why);
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "epf: element size must be 2 or 4");
    if (nplanes < 0 || nplanes > 65535) return fail(SGPU_BAD_ARGUMENT, "epf: bad number of planes");
    const size_t npix = (size_t)width * height;
    if (plane_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "epf: plane_stride < width*height");
    if (out_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "epf: out_stride < width*height");
    if (d_guide) {
        if (guide_elem_size != 2 && guide_elem_size != 4)
            return fail(SGPU_BAD_ARGUMENT, "epf: the guide's element size must be 2 or 4");
        if (guide_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "epf: guide_stride < width*height");
    }
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "epf: null planes");
    const size_t out_bytes = ((size_t)(nplanes - 1) * out_stride + npix) * sizeof(float);
    if (overlaps(d_in, ((size_t)(nplanes - 1) * plane_stride + npix) * elem_size, d_out, out_bytes))
        return fail(SGPU_BAD_ARGUMENT, "epf: the output overlaps the input");
    if (d_guide && overlaps(d_guide, ((size_t)(nplanes - 1) * guide_stride + npix) * guide_elem_size, d_out, out_bytes))
        return fail(SGPU_BAD_ARGUMENT, "epf: the output overlaps the guide");
    HIP_TRY(hipSetDevice(c->device));
    d = epf_window(d, ss);
    sgpu::EpfArgs a = {};
    a.in = d_in, a.in_ps = plane_stride, a.guide = d_guide, a.g_ps = d_guide ? guide_stride : 0;
    a.out = d_out, a.out_ps = out_stride;
    a.modulation = modulation, a.W = width, a.H = height, a.r = (d - 1) / 2;
    const int nlaunch = 2;
    const long long ws_ps = ((long long)npix + 3) & ~3LL;
    if (int r = c->epf_ws.ensure((size_t)2 * nplanes * ws_ps * sizeof(float))) return r;
    a.a = (float *)c->epf_ws.p, a.b = a.a + (size_t)nplanes * ws_ps, a.ab_ps = ws_ps;
    a.eps = si * si;
    a.inv_n = 1.0 / (double)(d * d);
    a.th = a.r > sgpu::EPF_WIDE_R ? sgpu::EPF_TILE_H_WIDE : sgpu::EPF_TILE_H;
    const bool vec = width % 4 == 0 && aligned16(d_in) && plane_stride % 4 == 0 && aligned16(d_out) &&
                     out_stride % 4 == 0 && (!d_guide || (aligned16(d_guide) && guide_stride % 4 == 0));
    const int gs = d_guide ? guide_elem_size : 0;
    for (int t = 0; t < nlaunch; t++) {
        if (!c->epf_ev[t]) HIP_TRY(hipEventCreate(&c->epf_ev[t]));
        HIP_TRY(hipEventRecord(c->epf_ev[t], c->stream));
        c->epf_what[t] = 100 * (1 + t) + d;
        if (vec)
            launch_all<true>(c, a, nplanes, elem_size, gs, t);
        else
            launch_all<false>(c, a, nplanes, elem_size, gs, t);
        HIP_TRY(hipGetLastError());
    }
    if (!c->epf_ev[nlaunch]) HIP_TRY(hipEventCreate(&c->epf_ev[nlaunch]));
    HIP_TRY(hipEventRecord(c->epf_ev[nlaunch], c->stream));
    c->epf_launches = nlaunch;
    return SGPU_OK;
}

extern "C" int sgpu_epf_last_kernel_ms(sgpu_context *c, float *ms, int *what, int *nlaunches) {
    if (!c || !ms || !what || !nlaunches) return fail(SGPU_BAD_ARGUMENT, "epf_last_kernel_ms: null argument");
    *nlaunches = c->epf_launches;
    if (!c->epf_launches) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->epf_ev[c->epf_launches]));
    for (int k = 0; k < c->epf_launches; k++) {
        HIP_TRY(hipEventElapsedTime(&ms[k], c->epf_ev[k], c->epf_ev[k + 1]));
        what[k] = c->epf_what[k];
    }
    return SGPU_OK;
}

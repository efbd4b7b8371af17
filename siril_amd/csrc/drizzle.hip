// drizzle.hip -- drizzle the frames of a registered sequence onto the
// reference grid scaled by `scale` (seqapplyreg -drizzle): per frame a float
// image and the float weight plane the stack takes as its drizzle weights.
//
// PARITY STATUS: neither Siril's nor STScI's source was available.  The
// arithmetic is modelled on cdrizzle's do_kernel_square / turbo / point, boxer
// and sgarea and is specified in full in DESIGN.md 6h; that specification,
// restated in tests/drizzle_ref.py, is the contract.  Parity is unpinned.
//
// The reference is a sequential scatter over input pixels in raster order,
// whose running mean is not associative, so the kernel is a gather: one lane
// per output pixel visits a superset of the input pixels that can land on it,
// in raster order, and applies the scatter's rule to itself only.  Every
// arithmetic step is drizzle_host.h's, shared with the host.
//
// One 256-lane workgroup per 22 x 11 output tile (242 lanes carry a pixel),
// frame in blockIdx.z.  Staged path: the tile's candidate box (drz_window on
// the tile's edges) is mapped once -- SQUARE: the four mapped corners, their
// area and the bounds of the drop; TURBO / POINT: the mapped centre -- into LDS
// next to the samples and pixel weights, and every output pixel walks its own
// window there.  Direct path: tiles whose box does not fit DRZ_PATCH pixels
// (strong down-scaling) map every candidate themselves from global memory.
// Both run the same double operations on the same values: identical bits.
//
// Colour-filter-array frames (seqapplyreg -drizzle -cfa=) have a kernel of
// their own, k_drizzle_cfa_frames: the same gather with one (image, weight)
// pair per colour, an input pixel updating its own colour's pair only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "drizzle_host.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

namespace sgpu {

using namespace sgpu_drizzle_host;

constexpr int DRZ_TW = 22, DRZ_TH = 11;              // output tile: 242 pixels on 256 lanes
// staged input pixels: SQUARE 9 doubles + 4 shorts + sample + weight = 88 B each, 53 504 B per
// workgroup, three workgroups per CU (160 KiB); TURBO / POINT 24 B each
constexpr int DRZ_PATCH = 608;
// tile counters striped over cache lines, as the frame warp's (DESIGN.md 6d finding 4)
constexpr int DRZ_STRIPES = 128, DRZ_STRIPE_WORDS = 8;

// bounds of a drop relative to the tile origin, clipped far outside the tile
struct alignas(8) DrzBounds {
    short x0, x1, y0, y1;
};

__device__ __forceinline__ short drz_rel(double v, int origin) {
    return (short)drz_clip(v - (double)origin, -30000, 30000);
}

// CFA frames, SQUARE: the bounds of a drop and the colour of its input pixel in one record.  y1 is
// compared with a tile row (0 .. 10) only, so a byte clipped far outside the tile holds it.
struct alignas(8) DrzBoundsCfa {
    short x0, x1, y0;
    signed char y1;
    unsigned char c;
};

template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void k_drizzle_frames(const T *in, const float *pw, float *out, float *outw, int W,
                                                        int H, int OW, int OH, long long fstride, long long ostride,
                                                        const double *maps, double scale, double pixfrac,
                                                        unsigned long long *counts) {
    constexpr int NQ = KERNEL == SGPU_DRIZZLE_SQUARE ? 9 : 2;
    __shared__ double s_q[NQ * DRZ_PATCH];
    __shared__ DrzBounds s_bb[KERNEL == SGPU_DRIZZLE_SQUARE ? DRZ_PATCH : 1];
    __shared__ float s_d[DRZ_PATCH];
    __shared__ float s_w[DRZ_PATCH];             // 0: the pixel is skipped (its own weight, or a degenerate drop)

    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * DRZ_TW, y0 = blockIdx.y * DRZ_TH;
    const double *A = maps + 18 * (size_t)f, *M = A + 9;
    const T *fin = in + (long long)f * fstride;
    const double grow = drz_grow(KERNEL, scale, pixfrac), widen = drz_widen(KERNEL, pixfrac);
    const double r = 0.5 * pixfrac * scale;      // TURBO half-size

    // ---- the tile's candidate box ----
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    bool ok;
    {
        double u0, u1, v0, v1;
        ok = drz_window(M, scale, (double)x0 - 0.5 - grow, (double)min(x0 + DRZ_TW, OW) - 0.5 + grow,
                        (double)y0 - 0.5 - grow, (double)min(y0 + DRZ_TH, OH) - 0.5 + grow, widen, u0, u1, v0, v1);
        if (ok) {
            drz_window_clip(u0, u1, v0, v1, 0, W - 1, 0, H - 1, bx0, bx1, by0, by1);
            if (bx1 < bx0 || by1 < by0) {        // the whole tile maps outside the frame
                bx0 = by0 = 0;
                bx1 = by1 = -1;
            }
            ok = (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1) <= DRZ_PATCH;
        }
#ifdef SGPU_DRZ_FORCE_DIRECT   // tuning variant: the plain register gather on every tile (same bits)
        ok = false;
#endif
    }
    // every lane computed the same values from the same inputs: make that explicit
    const bool staged = __builtin_amdgcn_readfirstlane((int)ok) != 0;
    bx0 = __builtin_amdgcn_readfirstlane(bx0);
    bx1 = __builtin_amdgcn_readfirstlane(bx1);
    by0 = __builtin_amdgcn_readfirstlane(by0);
    by1 = __builtin_amdgcn_readfirstlane(by1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;

    if (staged) {
        const int n = bw * bh;                   // <= DRZ_PATCH
        for (int idx = tid; idx < n; idx += 256) {
            const int rr = idx / bw, cc = idx - rr * bw;
            const int i = bx0 + cc, j = by0 + rr;
            const long long g = (long long)j * W + i;
            float w = pw ? pw[g] : 1.f;
            s_d[idx] = drz_sample(fin[g]);
            if (KERNEL == SGPU_DRIZZLE_SQUARE) {
                DrzQuad q;
                DrzBounds b = {1, 0, 1, 0};
                if (drz_quad(A, scale, pixfrac, i, j, q)) {
                    double bx_lo, bx_hi, by_lo, by_hi;
                    drz_quad_bounds(q, bx_lo, bx_hi, by_lo, by_hi);
                    b.x0 = drz_rel(bx_lo, x0);
                    b.x1 = drz_rel(bx_hi, x0);
                    b.y0 = drz_rel(by_lo, y0);
                    b.y1 = drz_rel(by_hi, y0);
                } else {
                    w = 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    s_q[k * DRZ_PATCH + idx] = q.qx[k];
                    s_q[(4 + k) * DRZ_PATCH + idx] = q.qy[k];
                }
                s_q[8 * DRZ_PATCH + idx] = q.jaco;
                s_bb[idx] = b;
            } else {
                double xo, yo;
                drz_map(A, scale, (double)i, (double)j, xo, yo);
                if (!drz_finite(xo) || !drz_finite(yo)) w = 0.f;
                s_q[idx] = xo;
                s_q[DRZ_PATCH + idx] = yo;
            }
            s_w[idx] = w;
        }
    }
    if (tid == 0) {
        const unsigned b = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        atomicAdd(&counts[(b % DRZ_STRIPES) * DRZ_STRIPE_WORDS + (staged ? 0 : 1)], 1ULL);
    }
    __syncthreads();

    const int ly = tid / DRZ_TW, lx = tid - ly * DRZ_TW;
    const int X = x0 + lx, Y = y0 + ly;
    if (ly >= DRZ_TH || X >= OW || Y >= OH) return;

    // ---- this pixel's candidate window: inside the tile's box (staged) or the frame (direct) ----
    const int cx0 = staged ? bx0 : 0, cx1 = staged ? bx1 : W - 1, cy0 = staged ? by0 : 0, cy1 = staged ? by1 : H - 1;
    int i0 = cx0, i1 = cx1, j0 = cy0, j1 = cy1;  // an irregular window: every pixel of the box is a candidate
    {
        double u0, u1, v0, v1;
        if (drz_window(M, scale, (double)X - 0.5 - grow, (double)X + 0.5 + grow, (double)Y - 0.5 - grow,
                       (double)Y + 0.5 + grow, widen, u0, u1, v0, v1))
            drz_window_clip(u0, u1, v0, v1, cx0, cx1, cy0, cy1, i0, i1, j0, j1);
    }

    float o = 0.f, vc = 0.f;
    if (!staged) {
        drz_gather_pixel(fin, pw, W, A, scale, pixfrac, KERNEL, i0, i1, j0, j1, X, Y, o, vc);
    } else {
        const double Xd = (double)X, Yd = (double)Y;
        for (int j = j0; j <= j1; j++) {
            const int row = (j - by0) * bw - bx0;
            for (int i = i0; i <= i1; i++) {
                const int p = row + i;
                const float w = s_w[p];
                if (w == 0.f) continue;
                float dow;
                if (KERNEL == SGPU_DRIZZLE_SQUARE) {
                    const DrzBounds b = s_bb[p];
                    if (lx < b.x0 || lx > b.x1 || ly < b.y0 || ly > b.y1) continue;
                    DrzQuad q;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        q.qx[k] = s_q[k * DRZ_PATCH + p];
                        q.qy[k] = s_q[(4 + k) * DRZ_PATCH + p];
                    }
                    q.jaco = s_q[8 * DRZ_PATCH + p];
                    dow = drz_dow_square(q, Xd, Yd, w);
                } else {
                    const double xo = s_q[p], yo = s_q[DRZ_PATCH + p];
                    if (KERNEL == SGPU_DRIZZLE_TURBO) {
                        double tx0, tx1, ty0, ty1;
                        drz_turbo_bounds(xo, yo, r, tx0, tx1, ty0, ty1);
                        if (Xd < tx0 || Xd > tx1 || Yd < ty0 || Yd > ty1) continue;
                        dow = drz_dow_turbo(xo, yo, r, Xd, Yd, w);
                    } else {
                        dow = (Xd == floor(xo + 0.5) && Yd == floor(yo + 0.5)) ? w : 0.f;
                    }
                }
                if (dow > 0.f) drz_update(o, vc, s_d[p], dow);
            }
        }
    }
    const long long op = (long long)f * ostride + (long long)Y * OW + X;
    out[op] = o;
    outw[op] = vc;
}

// k_drizzle_frames of colour-filter-array frames (DESIGN.md 6h "CFA frames"): every output pixel
// holds one (out, vc) pair per colour, and a candidate's dow -- computed once, it does not depend
// on the colour -- updates the pair of that input pixel's colour only.  Tile, staging, the choice
// of path and the counters are k_drizzle_frames'.  The colour of a staged pixel is staged with it:
// TURBO / POINT as a byte beside the weight; SQUARE inside the 8-byte record of the drop's
// bounds (DrzBoundsCfa), so that the workgroup stays at 53 504 B of LDS -- LDS is granted in
// granules of 1280 B here, a byte array more (54 112 B) rounds up to 55 040 B and leaves two
// workgroups per CU instead of three (measured: DESIGN.md 6h).  The three pairs stay in
// registers: the colour selects a pair in and out (drz_update_cfa), it indexes nothing.
// pat: dim * dim bytes; channel c of frame f at f * ostride + c * pstride.
template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void k_drizzle_cfa_frames(const T *in, const float *pw, float *out, float *outw,
                                                            int W, int H, int OW, int OH, long long fstride,
                                                            long long pstride, long long ostride, const double *maps,
                                                            const unsigned char *pat, int dim, double scale,
                                                            double pixfrac, unsigned long long *counts) {
    constexpr int NQ = KERNEL == SGPU_DRIZZLE_SQUARE ? 9 : 2;
    __shared__ double s_q[NQ * DRZ_PATCH];
    __shared__ DrzBoundsCfa s_bb[KERNEL == SGPU_DRIZZLE_SQUARE ? DRZ_PATCH : 1];
    __shared__ float s_d[DRZ_PATCH];
    __shared__ float s_w[DRZ_PATCH];             // 0: the pixel is skipped (its own weight, or a degenerate drop)
    __shared__ unsigned char s_c[KERNEL == SGPU_DRIZZLE_SQUARE ? 1 : DRZ_PATCH];   // TURBO / POINT: the colour

    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * DRZ_TW, y0 = blockIdx.y * DRZ_TH;
    const double *A = maps + 18 * (size_t)f, *M = A + 9;
    const T *fin = in + (long long)f * fstride;
    const double grow = drz_grow(KERNEL, scale, pixfrac), widen = drz_widen(KERNEL, pixfrac);
    const double r = 0.5 * pixfrac * scale;      // TURBO half-size

    // ---- the tile's candidate box ----
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    bool ok;
    {
        double u0, u1, v0, v1;
        ok = drz_window(M, scale, (double)x0 - 0.5 - grow, (double)min(x0 + DRZ_TW, OW) - 0.5 + grow,
                        (double)y0 - 0.5 - grow, (double)min(y0 + DRZ_TH, OH) - 0.5 + grow, widen, u0, u1, v0, v1);
        if (ok) {
            drz_window_clip(u0, u1, v0, v1, 0, W - 1, 0, H - 1, bx0, bx1, by0, by1);
            if (bx1 < bx0 || by1 < by0) {        // the whole tile maps outside the frame
                bx0 = by0 = 0;
                bx1 = by1 = -1;
            }
            ok = (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1) <= DRZ_PATCH;
        }
#ifdef SGPU_DRZ_FORCE_DIRECT   // tuning variant: the plain register gather on every tile (same bits)
        ok = false;
#endif
    }
    // every lane computed the same values from the same inputs: make that explicit
    const bool staged = __builtin_amdgcn_readfirstlane((int)ok) != 0;
    bx0 = __builtin_amdgcn_readfirstlane(bx0);
    bx1 = __builtin_amdgcn_readfirstlane(bx1);
    by0 = __builtin_amdgcn_readfirstlane(by0);
    by1 = __builtin_amdgcn_readfirstlane(by1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;

    if (staged) {
        const int n = bw * bh;                   // <= DRZ_PATCH
        for (int idx = tid; idx < n; idx += 256) {
            const int rr = idx / bw, cc = idx - rr * bw;
            const int i = bx0 + cc, j = by0 + rr;
            const long long g = (long long)j * W + i;
            float w = pw ? pw[g] : 1.f;
            s_d[idx] = drz_sample(fin[g]);
            const unsigned char col = (unsigned char)drz_cfa_colour(pat, dim, i, j);
            if (KERNEL == SGPU_DRIZZLE_SQUARE) {
                DrzQuad q;
                DrzBoundsCfa b = {1, 0, 1, 0, col};
                if (drz_quad(A, scale, pixfrac, i, j, q)) {
                    double bx_lo, bx_hi, by_lo, by_hi;
                    drz_quad_bounds(q, bx_lo, bx_hi, by_lo, by_hi);
                    b.x0 = drz_rel(bx_lo, x0);
                    b.x1 = drz_rel(bx_hi, x0);
                    b.y0 = drz_rel(by_lo, y0);
                    b.y1 = (signed char)drz_clip(by_hi - (double)y0, -100, 100);
                } else {
                    w = 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    s_q[k * DRZ_PATCH + idx] = q.qx[k];
                    s_q[(4 + k) * DRZ_PATCH + idx] = q.qy[k];
                }
                s_q[8 * DRZ_PATCH + idx] = q.jaco;
                s_bb[idx] = b;
            } else {
                double xo, yo;
                drz_map(A, scale, (double)i, (double)j, xo, yo);
                if (!drz_finite(xo) || !drz_finite(yo)) w = 0.f;
                s_q[idx] = xo;
                s_q[DRZ_PATCH + idx] = yo;
                s_c[idx] = col;
            }
            s_w[idx] = w;
        }
    }
    if (tid == 0) {
        const unsigned b = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        atomicAdd(&counts[(b % DRZ_STRIPES) * DRZ_STRIPE_WORDS + (staged ? 0 : 1)], 1ULL);
    }
    __syncthreads();

    const int ly = tid / DRZ_TW, lx = tid - ly * DRZ_TW;
    const int X = x0 + lx, Y = y0 + ly;
    if (ly >= DRZ_TH || X >= OW || Y >= OH) return;

    // ---- this pixel's candidate window: inside the tile's box (staged) or the frame (direct) ----
    const int cx0 = staged ? bx0 : 0, cx1 = staged ? bx1 : W - 1, cy0 = staged ? by0 : 0, cy1 = staged ? by1 : H - 1;
    int i0 = cx0, i1 = cx1, j0 = cy0, j1 = cy1;  // an irregular window: every pixel of the box is a candidate
    {
        double u0, u1, v0, v1;
        if (drz_window(M, scale, (double)X - 0.5 - grow, (double)X + 0.5 + grow, (double)Y - 0.5 - grow,
                       (double)Y + 0.5 + grow, widen, u0, u1, v0, v1))
            drz_window_clip(u0, u1, v0, v1, cx0, cx1, cy0, cy1, i0, i1, j0, j1);
    }

    float o0 = 0.f, v0 = 0.f, o1 = 0.f, v1 = 0.f, o2 = 0.f, v2 = 0.f;
    if (!staged) {
        float o[3], v[3];
        drz_gather_pixel_cfa(fin, pw, pat, dim, W, A, scale, pixfrac, KERNEL, i0, i1, j0, j1, X, Y, o, v);
        o0 = o[0];
        o1 = o[1];
        o2 = o[2];
        v0 = v[0];
        v1 = v[1];
        v2 = v[2];
    } else {
        const double Xd = (double)X, Yd = (double)Y;
        for (int j = j0; j <= j1; j++) {
            const int row = (j - by0) * bw - bx0;
            for (int i = i0; i <= i1; i++) {
                const int p = row + i;
                const float w = s_w[p];
                if (w == 0.f) continue;
                float dow;
                int col;
                if (KERNEL == SGPU_DRIZZLE_SQUARE) {
                    const DrzBoundsCfa b = s_bb[p];
                    col = b.c;
                    if (lx < b.x0 || lx > b.x1 || ly < b.y0 || ly > b.y1) continue;
                    DrzQuad q;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        q.qx[k] = s_q[k * DRZ_PATCH + p];
                        q.qy[k] = s_q[(4 + k) * DRZ_PATCH + p];
                    }
                    q.jaco = s_q[8 * DRZ_PATCH + p];
                    dow = drz_dow_square(q, Xd, Yd, w);
                } else {
                    const double xo = s_q[p], yo = s_q[DRZ_PATCH + p];
                    col = s_c[p];
                    if (KERNEL == SGPU_DRIZZLE_TURBO) {
                        double tx0, tx1, ty0, ty1;
                        drz_turbo_bounds(xo, yo, r, tx0, tx1, ty0, ty1);
                        if (Xd < tx0 || Xd > tx1 || Yd < ty0 || Yd > ty1) continue;
                        dow = drz_dow_turbo(xo, yo, r, Xd, Yd, w);
                    } else {
                        dow = (Xd == floor(xo + 0.5) && Yd == floor(yo + 0.5)) ? w : 0.f;
                    }
                }
                if (dow > 0.f) drz_update_cfa(o0, v0, o1, v1, o2, v2, col, s_d[p], dow);
            }
        }
    }
    const long long op = (long long)f * ostride + (long long)Y * OW + X;
    out[op] = o0;
    out[op + pstride] = o1;
    out[op + 2 * pstride] = o2;
    outw[op] = v0;
    outw[op + pstride] = v1;
    outw[op + 2 * pstride] = v2;
}

}  // namespace sgpu

using sgpu_host::fail;
namespace dh = sgpu_drizzle_host;

namespace {
constexpr int CNT_WORDS = sgpu::DRZ_STRIPES * sgpu::DRZ_STRIPE_WORDS;

template <typename T>
void launch_drizzle(int kernel, dim3 grid, hipStream_t st, const void *in, const float *pw, float *out, float *outw,
                    int W, int H, int OW, int OH, long long fstride, long long ostride, const double *maps,
                    double scale, double pixfrac, unsigned long long *cnt) {
#define SGPU_DRZ_LAUNCH(K)                                                                                      \
    hipLaunchKernelGGL((sgpu::k_drizzle_frames<T, K>), grid, dim3(256), 0, st, (const T *)in, pw, out, outw, W, H, \
                       OW, OH, fstride, ostride, maps, scale, pixfrac, cnt)
    if (kernel == SGPU_DRIZZLE_SQUARE) SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_SQUARE);
    else if (kernel == SGPU_DRIZZLE_TURBO) SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_TURBO);
    else SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_POINT);
#undef SGPU_DRZ_LAUNCH
}

template <typename T>
void launch_drizzle_cfa(int kernel, dim3 grid, hipStream_t st, const void *in, const float *pw, float *out,
                        float *outw, int W, int H, int OW, int OH, long long fstride, long long pstride,
                        long long ostride, const double *maps, const unsigned char *pat, int dim, double scale,
                        double pixfrac, unsigned long long *cnt) {
#define SGPU_DRZ_LAUNCH(K)                                                                                          \
    hipLaunchKernelGGL((sgpu::k_drizzle_cfa_frames<T, K>), grid, dim3(256), 0, st, (const T *)in, pw, out, outw, W, \
                       H, OW, OH, fstride, pstride, ostride, maps, pat, dim, scale, pixfrac, cnt)
    if (kernel == SGPU_DRIZZLE_SQUARE) SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_SQUARE);
    else if (kernel == SGPU_DRIZZLE_TURBO) SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_TURBO);
    else SGPU_DRZ_LAUNCH(SGPU_DRIZZLE_POINT);
#undef SGPU_DRZ_LAUNCH
}
}  // namespace

extern "C" int sgpu_drizzle_output_size(int width, int height, double scale, int *out_w, int *out_h) {
    if (!out_w || !out_h) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (const char *e = dh::drz_output_size(width, height, scale, out_w, out_h)) return fail(SGPU_BAD_ARGUMENT, e);
    return SGPU_OK;
}

extern "C" int sgpu_drizzle_forward_maps(int nframes, const double *H, int ref_index, int height, double *A) {
    if (const char *e = dh::drz_forward_maps(nframes, H, ref_index, height, A)) return fail(SGPU_BAD_ARGUMENT, e);
    return SGPU_OK;
}

extern "C" int sgpu_drizzle_check_maps(int nframes, const double *A, int width, int height,
                                       const sgpu_drizzle_params *params) {
    if (nframes < 1 || !A) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (const char *e = dh::drz_check_params(params)) return fail(SGPU_BAD_ARGUMENT, e);
    int ow = 0, oh = 0;
    if (const char *e = dh::drz_output_size(width, height, params->scale, &ow, &oh)) return fail(SGPU_BAD_ARGUMENT, e);
    for (int f = 0; f < nframes; f++) {
        double M[9];
        if (const char *e = dh::drz_frame_maps(A + 9 * (size_t)f, width, height, ow, oh, params, M))
            return fail(SGPU_BAD_ARGUMENT, e);
    }
    return SGPU_OK;
}

namespace {
// one call's share of the context's device block and its grid
struct DrzCall {
    int ow = 0, oh = 0;
    unsigned long long *dcnt = nullptr;   // striped tile counters, zeroed by the upload
    const double *dmaps = nullptr;        // per frame: A, M = inv3(A)
    const unsigned char *dtail = nullptr; // the caller's bytes behind the maps (the CFA pattern)
    dim3 grid;
};

// What both entries do before their launch: the argument checks (a frame holds nplanes output planes
// out_plane_stride apart), the maps and their refusals, and the upload of the block
// [counters][maps][tail, tail_bytes <= 40] on the context's stream.
int drz_begin(sgpu_context *c, const void *d_in, int elem_size, int nframes, int width, int height, long frame_stride,
              const double *H, int ref_index, const sgpu_drizzle_params *params, const float *d_out,
              const float *d_out_weights, long out_plane_stride, long out_frame_stride, int nplanes,
              const unsigned char *tail, size_t tail_bytes, DrzCall &k) {
    if (!c || !d_in || !d_out || !d_out_weights || !H || nframes < 1 || nframes > 65535 || width < 1 || height < 1 ||
        frame_stride < (long)width * height || ref_index < 0 || ref_index >= nframes)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (const char *e = dh::drz_check_params(params)) return fail(SGPU_BAD_ARGUMENT, e);
    int ow = 0, oh = 0;
    if (const char *e = dh::drz_output_size(width, height, params->scale, &ow, &oh)) return fail(SGPU_BAD_ARGUMENT, e);
    if (out_plane_stride < (long)ow * oh || out_frame_stride / nplanes < out_plane_stride ||
        (oh + sgpu::DRZ_TH - 1) / sgpu::DRZ_TH > 65535 || d_out == d_out_weights || (const void *)d_out == d_in ||
        (const void *)d_out_weights == d_in)
        return fail(SGPU_BAD_ARGUMENT, "drizzle: bad output planes");
    // host image of the device block: [striped tile counters][per frame: A, M = inv3(A)][tail]
    constexpr size_t TAIL_WORDS = 5;
    const size_t nd = CNT_WORDS + 18 * (size_t)nframes + TAIL_WORDS;
    c->h_drz.assign(nd, 0.0);
    double *hmaps = c->h_drz.data() + CNT_WORDS;
    {
        std::vector<double> A(9 * (size_t)nframes);
        if (const char *e = dh::drz_forward_maps(nframes, H, ref_index, height, A.data()))
            return fail(SGPU_BAD_ARGUMENT, e);
        for (int f = 0; f < nframes; f++) {
            double *fa = hmaps + 18 * (size_t)f;
            for (int i = 0; i < 9; i++) fa[i] = A[9 * (size_t)f + i];
            if (const char *e = dh::drz_frame_maps(fa, width, height, ow, oh, params, fa + 9))
                return fail(SGPU_BAD_ARGUMENT, e);
        }
    }
    if (tail_bytes) std::memcpy(hmaps + 18 * (size_t)nframes, tail, tail_bytes);
    HIP_TRY(hipSetDevice(c->device));
    if (int r = c->drz_ws.ensure(nd * sizeof(double))) return r;
    HIP_TRY(hipMemcpyAsync(c->drz_ws.p, c->h_drz.data(), nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
    k.ow = ow;
    k.oh = oh;
    k.dcnt = (unsigned long long *)c->drz_ws.p;
    k.dmaps = (const double *)c->drz_ws.p + CNT_WORDS;
    k.dtail = (const unsigned char *)(k.dmaps + 18 * (size_t)nframes);
    k.grid = dim3((unsigned)((ow + sgpu::DRZ_TW - 1) / sgpu::DRZ_TW), (unsigned)((oh + sgpu::DRZ_TH - 1) / sgpu::DRZ_TH),
                  (unsigned)nframes);
    return SGPU_OK;
}

// After the launch: the counters come back and the call synchronises.
int drz_end(sgpu_context *c, const DrzCall &k) {
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> cnt(CNT_WORDS, 0);   // read back before the synchronise below
    HIP_TRY(hipMemcpyAsync(cnt.data(), k.dcnt, CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream));
    // the host image must outlive the upload, and the counters must have landed
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->drz_tiles[0] = c->drz_tiles[1] = 0;
    for (int s = 0; s < sgpu::DRZ_STRIPES; s++) {
        c->drz_tiles[0] += cnt[s * sgpu::DRZ_STRIPE_WORDS];
        c->drz_tiles[1] += cnt[s * sgpu::DRZ_STRIPE_WORDS + 1];
    }
    return SGPU_OK;
}
}  // namespace

extern "C" int sgpu_drizzle_frames_device(sgpu_context *c, const void *d_in, int elem_size, int nframes, int width,
                                          int height, long frame_stride, const float *d_pixel_weights,
                                          const double *H, int ref_index, const sgpu_drizzle_params *params,
                                          float *d_out, float *d_out_weights, long out_frame_stride) {
    DrzCall k;
    if (int r = drz_begin(c, d_in, elem_size, nframes, width, height, frame_stride, H, ref_index, params, d_out,
                          d_out_weights, out_frame_stride, out_frame_stride, 1, nullptr, 0, k))
        return r;
    if (elem_size == 4)
        launch_drizzle<float>(params->kernel, k.grid, c->stream, d_in, d_pixel_weights, d_out, d_out_weights, width,
                              height, k.ow, k.oh, (long long)frame_stride, (long long)out_frame_stride, k.dmaps,
                              params->scale, params->pixfrac, k.dcnt);
    else
        launch_drizzle<uint16_t>(params->kernel, k.grid, c->stream, d_in, d_pixel_weights, d_out, d_out_weights, width,
                                 height, k.ow, k.oh, (long long)frame_stride, (long long)out_frame_stride, k.dmaps,
                                 params->scale, params->pixfrac, k.dcnt);
    return drz_end(c, k);
}

extern "C" int sgpu_drizzle_cfa_frames_device(sgpu_context *c, const void *d_in, int elem_size, int nframes, int width,
                                              int height, long frame_stride, const float *d_pixel_weights,
                                              const unsigned char *pattern, int pattern_dim, const double *H,
                                              int ref_index, const sgpu_drizzle_params *params, float *d_out,
                                              float *d_out_weights, long out_plane_stride, long out_frame_stride) {
    if (const char *e = dh::drz_check_pattern(pattern, pattern_dim)) return fail(SGPU_BAD_ARGUMENT, e);
    DrzCall k;
    if (int r = drz_begin(c, d_in, elem_size, nframes, width, height, frame_stride, H, ref_index, params, d_out,
                          d_out_weights, out_plane_stride, out_frame_stride, 3, pattern,
                          (size_t)pattern_dim * pattern_dim, k))
        return r;
    if (elem_size == 4)
        launch_drizzle_cfa<float>(params->kernel, k.grid, c->stream, d_in, d_pixel_weights, d_out, d_out_weights,
                                  width, height, k.ow, k.oh, (long long)frame_stride, (long long)out_plane_stride,
                                  (long long)out_frame_stride, k.dmaps, k.dtail, pattern_dim, params->scale,
                                  params->pixfrac, k.dcnt);
    else
        launch_drizzle_cfa<uint16_t>(params->kernel, k.grid, c->stream, d_in, d_pixel_weights, d_out, d_out_weights,
                                     width, height, k.ow, k.oh, (long long)frame_stride, (long long)out_plane_stride,
                                     (long long)out_frame_stride, k.dmaps, k.dtail, pattern_dim, params->scale,
                                     params->pixfrac, k.dcnt);
    return drz_end(c, k);
}

extern "C" int sgpu_drizzle_last_tiles(sgpu_context *c, long counts[2]) {
    if (!c || !counts) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    counts[0] = (long)c->drz_tiles[0];
    counts[1] = (long)c->drz_tiles[1];
    return SGPU_OK;
}

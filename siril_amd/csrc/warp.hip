// warp.hip -- apply_reg with an OpenCV interpolation (the
// resampling half): every frame warped through Href^-1 * Hf at scale 1 with
// FRAMING_CURRENT, as cvTransformImage does (Siril opencv/opencv.cpp:
// warpPerspective(BORDER_TRANSPARENT) onto a zeroed image, then the
// Lanczos / cubic clamp against a second, bilinear warp).
//
// PARITY STATUS: neither Siril's source nor OpenCV was available to check
// against.  The arithmetic is modelled on OpenCV's generic warpPerspective ->
// fixed-point remap path (INTER_BITS = 5, float coefficient tables,
// reflect-101 taps) and is specified in full in DESIGN.md "Frame warp"; that
// specification, restated in tests/warp_ref.py, is the contract.  Parity
// against a real OpenCV build is unpinned.
//
// Arithmetic (all coordinate math double, all sample math float, no FMA):
//   M  = (F * (Href^-1 * Hf) * F)^-1, F the row flip (frames are bottom-up)
//   X = M0*x + (M1*y + M2), Y = M3*x + (M4*y + M5), W = M6*x + (M7*y + M8)
//   w = W ? 32/W : 0;  U = (int)rint(sat(X*w));  sx = U >> 5, fx = U & 31
//   (NEAREST: w = W ? 1/W : 0, sx = (int)rint(sat(X*w))); likewise V, sy, fy
//   (sx, sy) outside the frame: the pixel stays 0.  Otherwise taps from
//   sx - (taps/2 - 1), indices reflected 101-style, 2-D weight wy[i]*wx[j],
//   row partials summed left to right, rows ascending, from 0.f.
//   WORD store: clamp(rint(sum), 0, 65535).
//   clamp: guide = the LINEAR warp; where out < guide * 0.98f (WORD: rounded
//   like a store), the pixel and its 4-neighbours take the guide.
//
// One workgroup per 64 x 16 output tile, frame in blockIdx.z.  Staged path:
// the tile (plus the 1-pixel halo the dilation needs) maps to a convex quad
// while W keeps one sign, so the bounding box of its four mapped corners plus
// the tap halo holds every tap; when that box fits WARP_PATCH floats it is
// loaded once (coalesced rows, WORD -> float and reflection on the way in)
// and the kernel, the guide and the clamp all read LDS.  Direct path: the
// same arithmetic gathering from global memory, for tiles whose W changes
// sign or whose box does not fit.  Both paths run the same float operations
// on the same values: identical bits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sgpu_internal.h"

#pragma clang fp contract(off)

namespace sgpu {

constexpr int WARP_TW = 64, WARP_TH = 16;            // output tile
constexpr int WARP_PW = WARP_TW + 2, WARP_PH = WARP_TH + 2;   // tile + dilation halo
constexpr int WARP_PATCH = 6144;                     // staged source patch, floats (24 KiB)
// tile counters: striped over cache lines (same-address atomics serialise: 47 000 workgroups on
// one pair of counters cost 2 ms); stripe s holds {staged, direct} at counts[8 * s]
constexpr int WARP_STRIPES = 128, WARP_STRIPE_WORDS = 8;

constexpr int K_NEAREST = 0, K_LINEAR = 1, K_CUBIC = 2, K_LANCZOS = 4;
constexpr int warp_taps(int kind) { return kind == K_NEAREST ? 1 : kind == K_LINEAR ? 2 : kind == K_CUBIC ? 4 : 8; }
constexpr int warp_lo(int kind) { return kind == K_NEAREST ? 0 : warp_taps(kind) / 2 - 1; }   // first tap: s - lo

__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

// (int)rint(clamp(v, INT_MIN, INT_MAX)); a NaN goes to INT_MIN
__device__ __forceinline__ int sat_rint(double v) {
    if (!(v >= -2147483648.0)) v = -2147483648.0;
    if (v > 2147483647.0) v = 2147483647.0;
    return (int)rint(v);
}

template <typename T>
__device__ __forceinline__ float round_store(float v);
template <>
__device__ __forceinline__ float round_store<float>(float v) {
    return v;
}
template <>
__device__ __forceinline__ float round_store<uint16_t>(float v) {
    float r = rintf(v);
    if (!(r >= 0.f)) r = 0.f;
    if (r > 65535.f) r = 65535.f;
    return r;
}
template <typename T>
__device__ __forceinline__ T to_sample(float v);
template <>
__device__ __forceinline__ float to_sample<float>(float v) {
    return v;
}
template <>
__device__ __forceinline__ uint16_t to_sample<uint16_t>(float v) {
    return (uint16_t)(int)v;
}

template <int KIND>
__device__ __forceinline__ void warp_map(const double *M, int x, int y, int &sx, int &sy, int &fx, int &fy) {
    const double xd = (double)x, yd = (double)y;
    const double X = M[0] * xd + (M[1] * yd + M[2]);
    const double Y = M[3] * xd + (M[4] * yd + M[5]);
    const double W = M[6] * xd + (M[7] * yd + M[8]);
    if (KIND == K_NEAREST) {
        const double w = W != 0.0 ? 1.0 / W : 0.0;
        sx = sat_rint(X * w);
        sy = sat_rint(Y * w);
        fx = fy = 0;
    } else {
        const double w = W != 0.0 ? 32.0 / W : 0.0;
        const int U = sat_rint(X * w), V = sat_rint(Y * w);
        sx = U >> 5;
        fx = U & 31;
        sy = V >> 5;
        fy = V & 31;
    }
}

// p: the first tap's sample in the staged patch
template <int TAPS>
__device__ __forceinline__ float interp_lds(const float *p, int pitch, const float *wx, const float *wy) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TAPS; i++) {
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < TAPS; j++) part += p[i * pitch + j] * (wy[i] * wx[j]);
        sum += part;
    }
    return sum;
}

// (tx, ty): the first tap's coordinates, possibly outside the frame
template <typename T, int TAPS>
__device__ __forceinline__ float interp_global(const T *in, int W, int H, int tx, int ty, const float *wx,
                                               const float *wy) {
    int xs[TAPS];
#pragma unroll
    for (int j = 0; j < TAPS; j++) xs[j] = reflect101(tx + j, W);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TAPS; i++) {
        const T *row = in + (long long)reflect101(ty + i, H) * W;
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < TAPS; j++) part += (float)row[xs[j]] * (wy[i] * wx[j]);
        sum += part;
    }
    return sum;
}

template <typename T, int KIND, bool CLAMP>
__global__ __launch_bounds__(256) void k_warp_frames(const T *in, T *out, int W, int H, long long fstride,
                                                     const double *Mall, const float *tab, const float *lin,
                                                     unsigned long long *counts) {
    constexpr int TAPS = warp_taps(KIND), LO = warp_lo(KIND), HI = TAPS - 1 - LO;
    constexpr int HALO = CLAMP ? 1 : 0;
    constexpr int TS = TAPS + 1;                     // table row stride: phases on distinct banks
    __shared__ float s_patch[WARP_PATCH];
    __shared__ float s_tab[KIND == K_NEAREST ? 1 : 32 * TS];
    __shared__ float s_lin[CLAMP ? 32 * 3 : 1];
    __shared__ float s_out[CLAMP ? WARP_PW * WARP_PH : 1];
    __shared__ float s_gd[CLAMP ? WARP_PW * WARP_PH : 1];
    __shared__ unsigned char s_mask[CLAMP ? WARP_PW * WARP_PH : 1];

    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * WARP_TW, y0 = blockIdx.y * WARP_TH;
    const double *M = Mall + 9 * (size_t)f;
    const T *fin = in + (long long)f * fstride;
    T *fout = out + (long long)f * fstride;

    if (KIND != K_NEAREST)
        for (int i = tid; i < 32 * TAPS; i += 256) s_tab[(i / TAPS) * TS + i % TAPS] = tab[i];
    if (CLAMP)
        for (int i = tid; i < 64; i += 256) s_lin[(i >> 1) * 3 + (i & 1)] = lin[i];

    // ---- footprint of the whole tile (+ halo): a property of the map, not of the frame size ----
    const int cx[2] = {x0 - HALO, x0 + WARP_TW - 1 + HALO};
    const int cy[2] = {y0 - HALO, y0 + WARP_TH - 1 + HALO};
    constexpr double SC = KIND == K_NEAREST ? 1.0 : 32.0;
    bool ok = true;
    double umin = 0, umax = 0, vmin = 0, vmax = 0;
    int sgn = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double xd = (double)cx[k & 1], yd = (double)cy[k >> 1];
        const double X = M[0] * xd + (M[1] * yd + M[2]);
        const double Y = M[3] * xd + (M[4] * yd + M[5]);
        const double Wc = M[6] * xd + (M[7] * yd + M[8]);
        const int s = Wc > 0.0 ? 1 : (Wc < 0.0 ? -1 : 0);
        if (k == 0) sgn = s;
        if (s == 0 || s != sgn) ok = false;
        const double w = SC / Wc, u = X * w, v = Y * w;
        if (!(fabs(u) < 1e8) || !(fabs(v) < 1e8)) ok = false;      // NaN and infinities too; int box arithmetic
        if (k == 0) {
            umin = umax = u;
            vmin = vmax = v;
        } else {
            umin = fmin(umin, u);
            umax = fmax(umax, u);
            vmin = fmin(vmin, v);
            vmax = fmax(vmax, v);
        }
    }
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1, bw = 0, bh = 0, pitch = 1;
    if (ok) {
        // one pixel of slack for the rounding of U and V
        bx0 = (int)floor(umin * (1.0 / SC)) - LO - 1;
        bx1 = (int)ceil(umax * (1.0 / SC)) + HI + 1;
        by0 = (int)floor(vmin * (1.0 / SC)) - LO - 1;
        by1 = (int)ceil(vmax * (1.0 / SC)) + HI + 1;
        pitch = (bx1 - bx0 + 1) | 1;                 // odd row pitch
        ok = (long long)pitch * (by1 - by0 + 1) <= WARP_PATCH;
        // load only coordinates a tap of an in-frame pixel can ask for
        bx0 = max(bx0, -LO);
        bx1 = min(bx1, W - 1 + HI);
        by0 = max(by0, -LO);
        by1 = min(by1, H - 1 + HI);
        bw = bx1 - bx0 + 1;
        bh = by1 - by0 + 1;
        if (bw <= 0 || bh <= 0) bw = bh = 0;         // the whole tile maps outside the frame
    }
    // every lane computed the same values from the same inputs: make that explicit
    const bool staged = __builtin_amdgcn_readfirstlane((int)ok) != 0;
    bx0 = __builtin_amdgcn_readfirstlane(bx0);
    bx1 = __builtin_amdgcn_readfirstlane(bx1);
    by0 = __builtin_amdgcn_readfirstlane(by0);
    by1 = __builtin_amdgcn_readfirstlane(by1);
    bw = __builtin_amdgcn_readfirstlane(bw);
    bh = __builtin_amdgcn_readfirstlane(bh);
    pitch = __builtin_amdgcn_readfirstlane(pitch);

    if (staged) {
        const int n = bw * bh;
        for (int idx = tid; idx < n; idx += 256) {
            const int r = idx / bw, c = idx - r * bw;
            const int yy = reflect101(by0 + r, H), xx = reflect101(bx0 + c, W);
            s_patch[r * pitch + c] = (float)fin[(long long)yy * W + xx];
        }
    }
    if (tid == 0) {
        const unsigned b = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        atomicAdd(&counts[(b % WARP_STRIPES) * WARP_STRIPE_WORDS + (staged ? 0 : 1)], 1ULL);
    }
    __syncthreads();

    // o: the interpolated sample, g: the bilinear guide (CLAMP), both as stored
    auto eval = [&](int x, int y, float &o, float &g) {
        int sx, sy, fx, fy;
        warp_map<KIND>(M, x, y, sx, sy, fx, fy);
        o = 0.f;
        g = 0.f;
        if (sx < 0 || sx >= W || sy < 0 || sy >= H) return;
        const int tx = sx - LO, ty = sy - LO;
        const bool inbox = staged && tx >= bx0 && tx + TAPS - 1 <= bx1 && ty >= by0 && ty + TAPS - 1 <= by1;
        if (KIND == K_NEAREST) {
            o = inbox ? s_patch[(ty - by0) * pitch + (tx - bx0)] : (float)fin[(long long)sy * W + sx];
            return;
        }
        float wx[TAPS], wy[TAPS], lx[2], ly[2];
#pragma unroll
        for (int j = 0; j < TAPS; j++) {
            wx[j] = s_tab[fx * TS + j];
            wy[j] = s_tab[fy * TS + j];
        }
        if (CLAMP) {
            lx[0] = s_lin[fx * 3];
            lx[1] = s_lin[fx * 3 + 1];
            ly[0] = s_lin[fy * 3];
            ly[1] = s_lin[fy * 3 + 1];
        }
        if (inbox) {
            const float *p = s_patch + (ty - by0) * pitch + (tx - bx0);
            o = interp_lds<TAPS>(p, pitch, wx, wy);
            if (CLAMP) g = interp_lds<2>(p + LO * pitch + LO, pitch, lx, ly);
        } else {
            o = interp_global<T, TAPS>(fin, W, H, tx, ty, wx, wy);
            if (CLAMP) g = interp_global<T, 2>(fin, W, H, sx, sy, lx, ly);
        }
        o = round_store<T>(o);
        g = round_store<T>(g);
    };

    if (!CLAMP) {
#pragma unroll 1
        for (int k = 0; k < WARP_TH / 4; k++) {
            const int x = x0 + (tid & 63), y = y0 + (tid >> 6) + 4 * k;
            if (x < W && y < H) {
                float o, g;
                eval(x, y, o, g);
                fout[(long long)y * W + x] = to_sample<T>(o);
            }
        }
    } else {
#pragma unroll 1
        for (int idx = tid; idx < WARP_PW * WARP_PH; idx += 256) {
            const int py = idx / WARP_PW, px = idx - py * WARP_PW;
            const int x = x0 - 1 + px, y = y0 - 1 + py;
            float o = 0.f, g = 0.f;
            unsigned char m = 0;
            if (x >= 0 && x < W && y >= 0 && y < H) {   // neighbours outside the frame never mark
                eval(x, y, o, g);
                const float thr = round_store<T>(g * 0.98f);
                m = o < thr ? 1 : 0;
            }
            s_out[idx] = o;
            s_gd[idx] = g;
            s_mask[idx] = m;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WARP_TH / 4; k++) {
            const int lx = tid & 63, ly = (tid >> 6) + 4 * k;
            const int x = x0 + lx, y = y0 + ly;
            if (x < W && y < H) {
                const int idx = (ly + 1) * WARP_PW + lx + 1;
                const int m = s_mask[idx] | s_mask[idx - 1] | s_mask[idx + 1] | s_mask[idx - WARP_PW] |
                              s_mask[idx + WARP_PW];
                fout[(long long)y * W + x] = to_sample<T>(m ? s_gd[idx] : s_out[idx]);
            }
        }
    }
}

}  // namespace sgpu

using sgpu_host::fail;

namespace {

// closed-form inverse: adjugate over the determinant, in this operation order
bool inv3(const double *m, double *o) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double A[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g,
                         c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d};
    const double det = (a * A[0] + b * A[3]) + c * A[6];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int k = 0; k < 9; k++) {
        o[k] = A[k] / det;
        if (!std::isfinite(o[k])) return false;
    }
    return true;
}

constexpr int TAB_FLOATS = 32 * 8, LIN_FLOATS = 32 * 2;
constexpr int CNT_WORDS = sgpu::WARP_STRIPES * sgpu::WARP_STRIPE_WORDS;

}  // namespace

extern "C" int sgpu_warp_inverse_maps(int nframes, const double *H, int ref_index, int height, double *M) {
    if (nframes < 1 || !H || !M || ref_index < 0 || ref_index >= nframes || height < 1)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    for (size_t k = 0; k < 9 * (size_t)nframes; k++)
        if (!std::isfinite(H[k])) return fail(SGPU_BAD_ARGUMENT, "warp: non-finite homography entry");
    double R[9];
    if (!inv3(H + 9 * (size_t)ref_index, R)) return fail(SGPU_BAD_ARGUMENT, "warp: singular reference homography");
    const double hm1 = (double)(height - 1);
    for (int fr = 0; fr < nframes; fr++) {
        const double *Hf = H + 9 * (size_t)fr;
        double Hc[9], A[9], Hm[9];
        // cvTransfH: Hc = Href^-1 * Hf
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                Hc[3 * r + c] = (R[3 * r] * Hf[c] + R[3 * r + 1] * Hf[3 + c]) + R[3 * r + 2] * Hf[6 + c];
        // Hm = F * (Hc * F), F = [[1, 0, 0], [0, -1, height - 1], [0, 0, 1]]
        for (int r = 0; r < 3; r++) {
            A[3 * r] = Hc[3 * r];
            A[3 * r + 1] = -Hc[3 * r + 1];
            A[3 * r + 2] = hm1 * Hc[3 * r + 1] + Hc[3 * r + 2];
        }
        for (int c = 0; c < 3; c++) {
            Hm[c] = A[c];
            Hm[3 + c] = -A[3 + c] + hm1 * A[6 + c];
            Hm[6 + c] = A[6 + c];
        }
        if (!inv3(Hm, M + 9 * (size_t)fr)) return fail(SGPU_BAD_ARGUMENT, "warp: singular or non-finite map");
    }
    return SGPU_OK;
}

extern "C" int sgpu_warp_table(int interpolation, float *tab, int *taps) {
    if (!tab || !taps || interpolation < 0 || interpolation > 4)
        return fail(SGPU_BAD_ARGUMENT, "warp table: interpolation OPENCV_NEAREST..LANCZOS4");
    if (interpolation == 0) {
        *taps = 1;
        for (int p = 0; p < 32; p++) tab[p] = 1.f;
    } else if (interpolation == 1 || interpolation == 3) {
        *taps = 2;
        for (int p = 0; p < 32; p++) {
            const float t = (float)p / 32.f;
            tab[2 * p] = 1.f - t;
            tab[2 * p + 1] = t;
        }
    } else if (interpolation == 2) {
        *taps = 4;
        const float A = -0.75f;
        for (int p = 0; p < 32; p++) {
            const float t = (float)p / 32.f, t1 = t + 1.f, u = 1.f - t;
            float *c = tab + 4 * p;
            c[0] = ((A * t1 - 5.f * A) * t1 + 8.f * A) * t1 - 4.f * A;
            c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
            c[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
            c[3] = 1.f - c[0] - c[1] - c[2];
        }
    } else {
        *taps = 8;
        const double PI = 3.1415926535897932384626433832795, s45 = 0.70710678118654752440084436210485;
        const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
        for (int p = 0; p < 32; p++) {
            float *c = tab + 8 * p;
            if (p == 0) {
                for (int i = 0; i < 8; i++) c[i] = i == 3 ? 1.f : 0.f;
                continue;
            }
            const double t = (double)p / 32.0;
            const double y0 = -(t + 3.0) * PI * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
            float sum = 0.f;
            for (int i = 0; i < 8; i++) {
                const double y = -(t + 3.0 - (double)i) * PI * 0.25;
                c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
                sum += c[i];
            }
            sum = 1.f / sum;
            for (int i = 0; i < 8; i++) c[i] *= sum;
        }
    }
    return SGPU_OK;
}

namespace {
template <typename T>
void launch_warp(int kind, bool clamp, dim3 grid, hipStream_t st, const void *in, void *out, int W, int H,
                 long long fstride, const double *M, const float *tab, const float *lin, unsigned long long *cnt) {
#define SGPU_WARP_LAUNCH(KIND, CL)                                                                              \
    hipLaunchKernelGGL((sgpu::k_warp_frames<T, KIND, CL>), grid, dim3(256), 0, st, (const T *)in, (T *)out, W, H, \
                       fstride, M, tab, lin, cnt)
    if (kind == sgpu::K_NEAREST) SGPU_WARP_LAUNCH(sgpu::K_NEAREST, false);
    else if (kind == sgpu::K_LINEAR) SGPU_WARP_LAUNCH(sgpu::K_LINEAR, false);
    else if (kind == sgpu::K_CUBIC && clamp) SGPU_WARP_LAUNCH(sgpu::K_CUBIC, true);
    else if (kind == sgpu::K_CUBIC) SGPU_WARP_LAUNCH(sgpu::K_CUBIC, false);
    else if (clamp) SGPU_WARP_LAUNCH(sgpu::K_LANCZOS, true);
    else SGPU_WARP_LAUNCH(sgpu::K_LANCZOS, false);
#undef SGPU_WARP_LAUNCH
}
}  // namespace

extern "C" int sgpu_warp_frames_device(sgpu_context *c, const void *d_in, void *d_out, int elem_size, int nframes,
                                       int width, int height, long frame_stride, const double *H, int ref_index,
                                       int interpolation, int clamp) {
    if (!c || !d_in || !d_out || !H || nframes < 1 || nframes > 65535 || width < 1 || height < 1 ||
        frame_stride < (long)width * height || ref_index < 0 || ref_index >= nframes ||
        (height + sgpu::WARP_TH - 1) / sgpu::WARP_TH > 65535)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (interpolation < 0 || interpolation > 4)
        return fail(SGPU_BAD_ARGUMENT, "warp: interpolation OPENCV_NEAREST..LANCZOS4 (NONE is sgpu_apply_reg_device)");
    if (d_in == d_out) return fail(SGPU_BAD_ARGUMENT, "in place warp is not supported");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    // host image of the device block: [striped tile counters][9 doubles per frame][table][bilinear table]
    const size_t nd = CNT_WORDS + 9 * (size_t)nframes + (TAB_FLOATS + LIN_FLOATS) / 2;
    c->h_warp.assign(nd, 0.0);
    double *hM = c->h_warp.data() + CNT_WORDS;
    if (int r = sgpu_warp_inverse_maps(nframes, H, ref_index, height, hM)) return r;
    float *htab = (float *)(hM + 9 * (size_t)nframes), *hlin = htab + TAB_FLOATS;
    int taps = 0;
    if (int r = sgpu_warp_table(interpolation, htab, &taps)) return r;
    if (int r = sgpu_warp_table(1, hlin, &taps)) return r;
    const int kind = interpolation == 3 ? sgpu::K_LINEAR : interpolation;   // AREA: the LINEAR table
    HIP_TRY(hipSetDevice(c->device));
    if (int r = c->warp_ws.ensure(nd * sizeof(double))) return r;
    HIP_TRY(hipMemcpyAsync(c->warp_ws.p, c->h_warp.data(), nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
    unsigned long long *dcnt = (unsigned long long *)c->warp_ws.p;
    const double *dM = (const double *)c->warp_ws.p + CNT_WORDS;
    const float *dtab = (const float *)(dM + 9 * (size_t)nframes), *dlin = dtab + TAB_FLOATS;
    dim3 grid((unsigned)((width + sgpu::WARP_TW - 1) / sgpu::WARP_TW),
              (unsigned)((height + sgpu::WARP_TH - 1) / sgpu::WARP_TH), (unsigned)nframes);
    if (elem_size == 4)
        launch_warp<float>(kind, clamp != 0, grid, c->stream, d_in, d_out, width, height, (long long)frame_stride, dM,
                           dtab, dlin, dcnt);
    else
        launch_warp<uint16_t>(kind, clamp != 0, grid, c->stream, d_in, d_out, width, height, (long long)frame_stride,
                              dM, dtab, dlin, dcnt);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> cnt(CNT_WORDS, 0);   // read back before the synchronise below
    HIP_TRY(hipMemcpyAsync(cnt.data(), dcnt, CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream));
    // the host image must outlive the upload, and the counters must have landed
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->warp_tiles[0] = c->warp_tiles[1] = 0;
    for (int s = 0; s < sgpu::WARP_STRIPES; s++) {
        c->warp_tiles[0] += cnt[s * sgpu::WARP_STRIPE_WORDS];
        c->warp_tiles[1] += cnt[s * sgpu::WARP_STRIPE_WORDS + 1];
    }
    return SGPU_OK;
}

extern "C" int sgpu_warp_last_tiles(sgpu_context *c, long counts[2]) {
    if (!c || !counts) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    counts[0] = (long)c->warp_tiles[0];
    counts[1] = (long)c->warp_tiles[1];
    return SGPU_OK;
}

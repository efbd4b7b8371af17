// wavelet_host.h -- the arithmetic of the a trous wavelet transform and its
// weighted reconstruction shared by the kernels
// (wavelet.hip), the C-ABI's host side and a stand-alone program
// (tests/hostsim/wavelet_host_main.cpp): the refusals, the conversion, the
// reflection, one separable smoothing, the detail and the accumulation.  Plain
// C++ unless compiled by hipcc, where the arithmetic is __host__ __device__.
//
// Everything is float; every operation is rounded once and nothing may be
// contracted into a fused multiply-add.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SGPU_WAV_HD __host__ __device__
#else
#define SGPU_WAV_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sgpu_wav_host {

constexpr int WAV_MAX_LAYERS = 6;
constexpr float WAV_INV_USHRT = 1.0f / 65535.0f;      // S1 of 6e

// ---- W0 ----
SGPU_WAV_HD inline float wav_to_float(float v) { return v; }
SGPU_WAV_HD inline float wav_to_float(uint16_t v) { return (float)v * WAV_INV_USHRT; }

// ---- W1 ----
SGPU_WAV_HD inline int wav_refl(int i, int N) { return i < 0 ? -i : (i >= N ? 2 * (N - 1) - i : i); }
// taps on each side of the centre: 2 (B3 spline) or 1 (linear)
SGPU_WAV_HD inline int wav_radius(int type) { return type == 2 ? 2 : 1; }
// the largest offset any tap of an n-layer transform uses
SGPU_WAV_HD inline int wav_reach(int n, int type) { return n <= 1 ? 0 : wav_radius(type) << (n - 2); }

// nullptr, or what is refused
inline const char *wav_check(int W, int H, int n, int type) {
    if (W < 1 || H < 1) return "wavelet: empty plane";
    if (n < 1 || n > WAV_MAX_LAYERS) return "wavelet: nbr_layers must be 1 .. 6";
    if (type < 1 || type > 2) return "wavelet: type must be 1 (linear) or 2 (B3 spline)";
    if (wav_reach(n, type) > (W < H ? W : H) - 1) return "wavelet: the plane is too small for that many layers";
    return nullptr;
}

inline bool wav_finite(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// ---- W2 ----
// one line of the smoothing: the taps at -2s, -s, 0, +s, +2s (type 1 ignores the outer pair)
SGPU_WAV_HD inline float wav_smooth(int type, float m2, float m1, float c, float p1, float p2) {
    if (type == 2) {
        const float outer = (m2 + p2) * (1.0f / 16.0f);
        const float inner = (m1 + p1) * (1.0f / 4.0f);
        const float side = outer + inner;
        const float mid = c * (3.0f / 8.0f);
        return side + mid;
    }
    const float side = (m1 + p1) * (1.0f / 4.0f);
    const float mid = c * (1.0f / 2.0f);
    return side + mid;
}

// ---- W3 ----
SGPU_WAV_HD inline float wav_detail(float c_j, float c_next) { return c_j - c_next; }

// ---- W4 ----
SGPU_WAV_HD inline float wav_first(float k, float v) { return k * v; }
SGPU_WAV_HD inline float wav_add(float acc, float k, float v) {
    const float t = k * v;
    return acc + t;
}

// ---- host restatements of one plane (the stand-alone program) ----

// c_{j+1} of c (W x H) at step s
inline void wav_smooth_plane_host(const float *c, int W, int H, int type, int s, float *tmp, float *next) {
    const bool b3 = type == 2;      // the outer taps of the linear filter are not read: they may lie outside the plane
    for (int y = 0; y < H; y++) {
        const float *r = c + (size_t)y * W;
        for (int x = 0; x < W; x++)
            tmp[(size_t)y * W + x] = wav_smooth(type, b3 ? r[wav_refl(x - 2 * s, W)] : 0.0f, r[wav_refl(x - s, W)], r[x],
                                                r[wav_refl(x + s, W)], b3 ? r[wav_refl(x + 2 * s, W)] : 0.0f);
    }
    for (int y = 0; y < H; y++) {
        const float *m1 = tmp + (size_t)wav_refl(y - s, H) * W, *p1 = tmp + (size_t)wav_refl(y + s, H) * W;
        const float *m2 = b3 ? tmp + (size_t)wav_refl(y - 2 * s, H) * W : m1, *p2 = b3 ? tmp + (size_t)wav_refl(y + 2 * s, H) * W : p1;
        for (int x = 0; x < W; x++)
            next[(size_t)y * W + x] = wav_smooth(type, m2[x], m1[x], tmp[(size_t)y * W + x], p1[x], p2[x]);
    }
}

// W3: planes[k * W*H ..], k < n
template <typename T>
inline void wav_transform_host(const T *in, int W, int H, int n, int type, float *planes) {
    const size_t np = (size_t)W * H;
    std::vector<float> c(np), tmp(np), next(np);
    for (size_t i = 0; i < np; i++) c[i] = wav_to_float(in[i]);
    for (int j = 0; j + 1 < n; j++) {
        wav_smooth_plane_host(c.data(), W, H, type, 1 << j, tmp.data(), next.data());
        for (size_t i = 0; i < np; i++) planes[(size_t)j * np + i] = wav_detail(c[i], next[i]);
        c.swap(next);
    }
    for (size_t i = 0; i < np; i++) planes[(size_t)(n - 1) * np + i] = c[i];
}

// W4
inline void wav_reconstruct_host(const float *planes, size_t np, int n, const float *coef, float *out) {
    for (size_t i = 0; i < np; i++) {
        float acc = wav_first(coef[0], planes[i]);
        for (int k = 1; k < n; k++) acc = wav_add(acc, coef[k], planes[(size_t)k * np + i]);
        out[i] = acc;
    }
}

}  // namespace sgpu_wav_host

// epf_host.h -- the edge-preserving filter (`epf -guided`: the guided filter;
// DESIGN.md 6n, E0-E7) as it is shared by the kernels (epf.hip), the C-ABI's
// host side and a stand-alone program (tests/hostsim/epf_host_main.cpp): the
// refusals, the window rule, the guided filter's coefficients, and a host
// reference of whole planes.  Plain C++ unless compiled by hipcc, where the
// arithmetic is __host__ __device__.  The bilateral filter (mode 0) is
// specified in 6n but not built: it is refused.
//
// The widening is str_widen of stretch_host.h, the reflection is wav_refl of
// wavelet_host.h, the modulation is med_modulate of median_host.h; nothing of
// them is restated here.  Everything between the samples and the one rounding
// to float is double, every operation is rounded once and nothing may be
// contracted into a fused multiply-add.  The order in which an expression is
// written below is the specification; tests/epf_ref.py follows it literally.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "median_host.h"
#include "stretch_host.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define SGPU_EPF_HD SGPU_STR_HD

namespace sgpu_epf_host {

using sgpu_med_host::med_modulate;
using sgpu_str_host::str_widen;
using sgpu_wav_host::wav_refl;

constexpr int EPF_MIN_D = 3, EPF_MAX_D = 25, EPF_MAX_R = (EPF_MAX_D - 1) / 2;

inline bool epf_finite(double v) { return (sgpu_str_host::rbf_bits(v) >> 52 & 0x7FFu) != 0x7FFu; }

// ---- E1: the window; d = 0 asks for OpenCV's rule ----
inline int epf_window(int d, double ss) {
    if (d != 0) return d;
    double rd = __builtin_floor(1.5 * ss + 0.5);        // round half away from zero, ss > 0
    rd = rd > (double)EPF_MAX_R ? (double)EPF_MAX_R : rd;
    rd = rd < 1.0 ? 1.0 : rd;
    return 2 * (int)rd + 1;
}

// ---- E6: nullptr, or what is refused ----
inline const char *epf_check(int W, int H, int mode, int d, double si, double ss, float modulation) {
    if (W < 1 || H < 1) return "epf: empty plane";
    if (W > 65535 || H > 65535) return "epf: the plane is too large";
    if (mode == SGPU_EPF_BILATERAL) return "epf: the bilateral filter is not built; mode must be 1 (guided)";
    if (mode != SGPU_EPF_GUIDED) return "epf: mode must be 1 (guided)";
    if (!epf_finite(si) || !(si > 0.0)) return "epf: si must be finite and above 0";
    if (d == 0 && (!epf_finite(ss) || !(ss > 0.0))) return "epf: ss must be finite and above 0";
    if (d != 0 && (d < EPF_MIN_D || d > EPF_MAX_D || d % 2 == 0)) return "epf: d must be 0, or odd in 3 .. 25";
    if ((epf_window(d, ss) - 1) / 2 > (W < H ? W : H) - 1) return "epf: the plane is too small for that window";
    if (!sgpu_wav_host::wav_finite(modulation) || !(modulation >= 0.0f && modulation <= 1.0f))
        return "epf: modulation must be in [0, 1]";
    return nullptr;
}

// ---- E3: a and b from the four box means ----
SGPU_EPF_HD inline void epf_coeffs(double mI, double mp, double cII, double cIp, double eps, float *a, float *b) {
    const double var = cII - mI * mI;
    const double cov = cIp - mI * mp;
    const double ad = cov / (var + eps);
    const double bd = mp - ad * mI;
    *a = (float)ad;
    *b = (float)bd;
}
SGPU_EPF_HD inline float epf_guided_out(double ma, double mb, double I) { return (float)(ma * I + mb); }

// ---- E4: x is the sample the result replaces, rounded to float once ----
SGPU_EPF_HD inline float epf_centre(float v) { return v; }
SGPU_EPF_HD inline float epf_centre(uint16_t v) { return (float)str_widen(v); }

// ---- host restatement of whole planes (the stand-alone program) ----

// box(f) at (x, y): the row sums left to right, the rows top to bottom, times 1 / (d d)
template <class F>
inline double epf_box_ref(F f, int W, int H, int x, int y, int r, double inv_n) {
    double col = 0.0;
    for (int dy = -r; dy <= r; dy++) {
        const int yy = wav_refl(y + dy, H);
        double row = f(wav_refl(x - r, W), yy);
        for (int dx = -r + 1; dx <= r; dx++) row = row + f(wav_refl(x + dx, W), yy);
        col = dy == -r ? row : col + row;
    }
    return col * inv_n;
}

// E0-E4 of one plane; guide is nullptr for the self-guided filter
template <typename T, typename G>
inline void epf_filter_host(const T *in, const G *guide, int W, int H, int d, double si, double ss, float modulation,
                            float *out) {
    d = epf_window(d, ss);
    const int r = (d - 1) / 2;
    const size_t np = (size_t)W * H;
    const double eps = si * si, inv_n = 1.0 / (double)(d * d);
    auto P = [&](int x, int y) { return str_widen(in[(size_t)y * W + x]); };
    auto I = [&](int x, int y) { return guide ? str_widen(guide[(size_t)y * W + x]) : P(x, y); };
    std::vector<float> a(np), b(np);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double mI = epf_box_ref(I, W, H, x, y, r, inv_n), mp = epf_box_ref(P, W, H, x, y, r, inv_n);
            const double cII = epf_box_ref([&](int u, int v) { return I(u, v) * I(u, v); }, W, H, x, y, r, inv_n);
            const double cIp = epf_box_ref([&](int u, int v) { return I(u, v) * P(u, v); }, W, H, x, y, r, inv_n);
            epf_coeffs(mI, mp, cII, cIp, eps, &a[(size_t)y * W + x], &b[(size_t)y * W + x]);
        }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double ma = epf_box_ref([&](int u, int v) { return (double)a[(size_t)v * W + u]; }, W, H, x, y, r, inv_n);
            const double mb = epf_box_ref([&](int u, int v) { return (double)b[(size_t)v * W + u]; }, W, H, x, y, r, inv_n);
            out[(size_t)y * W + x] =
                med_modulate(modulation, epf_guided_out(ma, mb, I(x, y)), epf_centre(in[(size_t)y * W + x]));
        }
}

}  // namespace sgpu_epf_host

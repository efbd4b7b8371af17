// bkg_host.h -- the arithmetic of the polynomial background extraction
//  shared by the kernels (background.hip), the C-ABI's
// host side and a stand-alone program (tests/hostsim/bkg_host_main.cpp): the
// sample grid and its refusals, the parameter checks, the term table, the
// ordered key of the box median, the selection threshold, the normal sums, the
// Cholesky solve, the closed-form mean of the model, the Horner evaluation and
// the correction.  Plain C++ unless compiled by hipcc, where the arithmetic is
// __host__ __device__.
//
// Samples and medians are float, everything from the selection on is double,
// every operation is rounded once and nothing may be contracted into a fused
// multiply-add.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sirilgpu.h"

#if defined(__HIPCC__)
#define SGPU_BKG_HD __host__ __device__
#else
#define SGPU_BKG_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sgpu_bkg_host {

constexpr int BKG_BOX = 25, BKG_R = 12, BKG_NS = BKG_BOX * BKG_BOX, BKG_RANK = 312;
constexpr int BKG_MAX_K = 8192, BKG_NCOEF = 15, BKG_NPAIR = 120;     // pairs q <= p of 15 terms
constexpr float BKG_INV_USHRT = 1.0f / 65535.0f;                     // S1 of 6e

// ---- B1 ----
struct BkgGrid {
    int nx, ny, dist, startx, starty, K;
};

// nullptr and *g filled, or what is refused
inline const char *bkg_grid(int W, int H, int S, BkgGrid *g) {
    if (W < BKG_BOX || H < BKG_BOX) return "subsky: the frame is smaller than one 25 x 25 sample box";
    if (S < 1) return "subsky: samples < 1";
    const int dist = W / S;
    if (dist < 1) return "subsky: more samples per line than pixels";
    const long long nx = (W - BKG_BOX) / dist + 1, ny = (H - BKG_BOX) / dist + 1;
    if (nx * ny > BKG_MAX_K) return "subsky: more than 8192 sample boxes";
    g->dist = dist;
    g->startx = ((W - BKG_BOX) % dist) / 2;
    g->starty = ((H - BKG_BOX) % dist) / 2;
    g->nx = (int)nx;
    g->ny = (int)ny;
    g->K = (int)(nx * ny);
    return nullptr;
}

SGPU_BKG_HD inline int bkg_cx(const BkgGrid &g, int i) { return BKG_R + g.startx + i * g.dist; }
SGPU_BKG_HD inline int bkg_cy(const BkgGrid &g, int j) { return BKG_R + g.starty + j * g.dist; }

inline const char *bkg_check_params(const sgpu_bkg_params *p) {
    if (!p) return "subsky: no parameters";
    if (p->degree < 1 || p->degree > 4) return "subsky: degree must be 1 .. 4";
    if (!(p->tolerance >= 0.0) || !(p->tolerance <= 1.7976931348623157e308))
        return "subsky: tolerance must be finite and >= 0";
    return nullptr;
}

SGPU_BKG_HD inline int bkg_ncoef(int d) { return (d + 1) * (d + 2) / 2; }

// ---- the term table: (i, j) of u^i v^j by total degree, then by j ----
SGPU_BKG_HD inline int bkg_ti(int p) {
    constexpr int t[BKG_NCOEF] = {0, 1, 0, 2, 1, 0, 3, 2, 1, 0, 4, 3, 2, 1, 0};
    return t[p];
}
SGPU_BKG_HD inline int bkg_tj(int p) {
    constexpr int t[BKG_NCOEF] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4};
    return t[p];
}
SGPU_BKG_HD inline int bkg_term(int i, int j) { return (i + j) * (i + j + 1) / 2 + j; }
// pair s < 120 -> (p, q), q <= p, rows of the lower triangle one after the other
SGPU_BKG_HD inline void bkg_pair(int s, int &p, int &q) {
    p = 0;
    while ((p + 1) * (p + 2) / 2 <= s) p++;
    q = s - p * (p + 1) / 2;
}

// ---- B0, B2 ----
SGPU_BKG_HD inline float bkg_to_float(float v) { return v; }
SGPU_BKG_HD inline float bkg_to_float(uint16_t v) { return (float)v * BKG_INV_USHRT; }

SGPU_BKG_HD inline uint32_t bkg_float_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
SGPU_BKG_HD inline float bkg_bits_float(uint32_t b) {
    float v;
    memcpy(&v, &b, 4);
    return v;
}
// -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
SGPU_BKG_HD inline uint32_t bkg_key(float v) {
    const uint32_t b = bkg_float_bits(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
SGPU_BKG_HD inline float bkg_unkey(uint32_t k) {
    return bkg_bits_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
// the median as it is stored: a non-finite one becomes 0
SGPU_BKG_HD inline float bkg_median_of_key(uint32_t k) {
    const float m = bkg_unkey(k);
    return (bkg_float_bits(m) & 0x7F800000u) == 0x7F800000u ? 0.0f : m;
}

// ---- B3 ----
SGPU_BKG_HD inline bool bkg_keep(float med, double T) {
    const double m = (double)med;
    return m > 0.0 && m <= T;
}

// ---- B4 ----
// the normalised coordinate of pixel c of an axis of n: u = ((double)c - x0) * ax
struct BkgAxis {
    double x0, ax;
};
SGPU_BKG_HD inline BkgAxis bkg_axis(int n) {
    BkgAxis a;
    a.x0 = (double)(n - 1) * 0.5;
    a.ax = 1.0 / a.x0;
    return a;
}
SGPU_BKG_HD inline double bkg_coord(int c, const BkgAxis &a) { return ((double)c - a.x0) * a.ax; }
SGPU_BKG_HD inline double bkg_coord(int c, int n) { return bkg_coord(c, bkg_axis(n)); }
// u^i by repeated multiplication: 1, u, u*u, (u*u)*u, ((u*u)*u)*u
SGPU_BKG_HD inline double bkg_pow(double u, int i) {
    if (i == 0) return 1.0;
    double w = u;
    for (int t = 1; t < i; t++) w = w * u;
    return w;
}

// One of the 135 sums over the kept boxes in ascending k: A[p][q] (q >= 0) or g[p] (q < 0).
SGPU_BKG_HD inline double bkg_normal_sum(int p, int q, const float *med, const uint8_t *keep, const BkgGrid &g,
                                         int W, int H) {
    const int ip = bkg_ti(p), jp = bkg_tj(p), iq = q < 0 ? 0 : bkg_ti(q), jq = q < 0 ? 0 : bkg_tj(q);
    const BkgAxis xa = bkg_axis(W), ya = bkg_axis(H);
    double acc = 0.0;
    int k = 0;
    for (int j = 0; j < g.ny; j++) {
        const double v = bkg_coord(bkg_cy(g, j), ya);
        const double vpp = bkg_pow(v, jp), vpq = bkg_pow(v, jq);
        for (int i = 0; i < g.nx; i++, k++) {
            if (!keep[k]) continue;
            const double u = bkg_coord(bkg_cx(g, i), xa);
            const double fp = bkg_pow(u, ip) * vpp;
            const double t = q < 0 ? fp * (double)med[k] : fp * (bkg_pow(u, iq) * vpq);
            acc += t;
        }
    }
    return acc;
}

// Cholesky (j outer) of the n x n normal matrix A (row stride 15), then the two
// triangular solves; 0, or 2 when a pivot is not positive.  c[n .. 14] = +0.
// L (15 x 15) and y (15) are the caller's workspace (LDS in the kernel).
SGPU_BKG_HD inline int bkg_solve(int n, const double *A, const double *g, double *c, double *L, double *y) {
    for (int p = 0; p < BKG_NCOEF; p++) c[p] = 0.0;
    for (int j = 0; j < n; j++) {
        double s = A[j * BKG_NCOEF + j];
        for (int k = 0; k < j; k++) {
            const double t = L[j * BKG_NCOEF + k] * L[j * BKG_NCOEF + k];
            s = s - t;
        }
        if (!(s > 0.0)) return 2;
        const double d = sqrt(s);
        L[j * BKG_NCOEF + j] = d;
        for (int i = j + 1; i < n; i++) {
            double a = A[i * BKG_NCOEF + j];
            for (int k = 0; k < j; k++) {
                const double t = L[i * BKG_NCOEF + k] * L[j * BKG_NCOEF + k];
                a = a - t;
            }
            L[i * BKG_NCOEF + j] = a / d;
        }
    }
    for (int i = 0; i < n; i++) {
        double a = g[i];
        for (int k = 0; k < i; k++) {
            const double t = L[i * BKG_NCOEF + k] * y[k];
            a = a - t;
        }
        y[i] = a / L[i * BKG_NCOEF + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double a = y[i];
        for (int k = i + 1; k < n; k++) {
            const double t = L[k * BKG_NCOEF + i] * c[k];
            a = a - t;
        }
        c[i] = a / L[i * BKG_NCOEF + i];
    }
    return 0;
}

// ---- B5 ----
// (sum over x = 0 .. n-1 of u(x)^i) / n, i = 1 .. 4
SGPU_BKG_HD inline double bkg_axis_moment(int n, int i) {
    const BkgAxis a = bkg_axis(n);
    double s = 0.0;
    for (int x = 0; x < n; x++) {
        s += bkg_pow(bkg_coord(x, a), i);
    }
    return s / (double)n;
}
SGPU_BKG_HD inline double bkg_model_mean(const double *c, const double *Mx, const double *My) {
    double s = 0.0;
    for (int p = 0; p < BKG_NCOEF; p++) {
        const double t = c[p] * (Mx[bkg_ti(p)] * My[bkg_tj(p)]);
        s += t;
    }
    return s;
}

// ---- B6 ----
// C[i][j] (row stride 5): the coefficient of u^i v^j, +0 past the total degree 4
SGPU_BKG_HD inline void bkg_full_table(const double *c, double *C) {
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) C[i * 5 + j] = i + j <= 4 ? c[bkg_term(i, j)] : 0.0;
}
SGPU_BKG_HD inline void bkg_row_poly(const double *C, double v, double *r) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 5; k++) {
        double a = C[k * 5 + 4] * v;
        a = a + C[k * 5 + 3];
        a = a * v;
        a = a + C[k * 5 + 2];
        a = a * v;
        a = a + C[k * 5 + 1];
        a = a * v;
        r[k] = a + C[k * 5];
    }
}
SGPU_BKG_HD inline double bkg_eval(const double *r, double u) {
    double b = r[4] * u;
    b = b + r[3];
    b = b * u;
    b = b + r[2];
    b = b * u;
    b = b + r[1];
    b = b * u;
    return b + r[0];
}

// ---- B7 ----
SGPU_BKG_HD inline float bkg_correct(float x, double b, double mean, int divide) {
    if (divide) {
        if (b == 0.0) return 0.0f;
        const double t = (double)x / b;
        return (float)(t * mean);
    }
    const double t = (double)x - b;
    return (float)(t + mean);
}

// ---- host restatements of one plane (the stand-alone program) ----

template <typename T>
inline float bkg_box_median_host(const T *plane, int W, const BkgGrid &g, int k) {
    const int cx = bkg_cx(g, k % g.nx), cy = bkg_cy(g, k / g.nx);
    std::vector<uint32_t> keys;
    keys.reserve(BKG_NS);
    for (int dy = -BKG_R; dy <= BKG_R; dy++)
        for (int dx = -BKG_R; dx <= BKG_R; dx++)
            keys.push_back(bkg_key(bkg_to_float(plane[(size_t)(cy + dy) * W + (cx + dx)])));
    std::nth_element(keys.begin(), keys.begin() + BKG_RANK, keys.end());
    return bkg_median_of_key(keys[BKG_RANK]);
}

inline double bkg_median_sorted(std::vector<double> a) {
    std::sort(a.begin(), a.end());
    const size_t K = a.size();
    return (K & 1) ? a[K / 2] : (a[K / 2 - 1] + a[K / 2]) * 0.5;
}

// B3: keep mask and the number kept
inline int bkg_select_host(const float *med, int K, double tol, uint8_t *keep) {
    std::vector<double> a((size_t)K);
    for (int k = 0; k < K; k++) a[(size_t)k] = (double)med[k];
    const double m = bkg_median_sorted(a);
    for (int k = 0; k < K; k++) a[(size_t)k] = fabs((double)med[k] - m);
    const double mad = bkg_median_sorted(a);
    const double T = m + tol * mad;
    int kept = 0;
    for (int k = 0; k < K; k++) kept += (keep[k] = bkg_keep(med[k], T) ? 1 : 0);
    return kept;
}

// B4 + B5: status 0 / 1 / 2; c[15] and *mean are +0 unless the status is 0
inline int bkg_fit_host(const float *med, const uint8_t *keep, int kept, const BkgGrid &g, int W, int H, int degree,
                        double *c, double *mean) {
    const int n = bkg_ncoef(degree);
    for (int p = 0; p < BKG_NCOEF; p++) c[p] = 0.0;
    *mean = 0.0;
    if (kept < n) return 1;
    double A[BKG_NCOEF * BKG_NCOEF] = {0.0}, rhs[BKG_NCOEF] = {0.0};
    for (int p = 0; p < n; p++) {
        for (int q = 0; q <= p; q++)
            A[p * BKG_NCOEF + q] = A[q * BKG_NCOEF + p] = bkg_normal_sum(p, q, med, keep, g, W, H);
        rhs[p] = bkg_normal_sum(p, -1, med, keep, g, W, H);
    }
    double L[BKG_NCOEF * BKG_NCOEF], y[BKG_NCOEF];
    if (int st = bkg_solve(n, A, rhs, c, L, y)) {
        for (int p = 0; p < BKG_NCOEF; p++) c[p] = 0.0;
        return st;
    }
    double Mx[5] = {1.0}, My[5] = {1.0};
    for (int i = 1; i <= 4; i++) {
        Mx[i] = bkg_axis_moment(W, i);
        My[i] = bkg_axis_moment(H, i);
    }
    *mean = bkg_model_mean(c, Mx, My);
    return 0;
}

}  // namespace sgpu_bkg_host

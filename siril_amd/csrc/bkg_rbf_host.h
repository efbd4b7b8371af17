// bkg_rbf_host.h -- the arithmetic of the thin-plate-spline background
// extraction shared by the kernels (background_rbf.hip),
// the C-ABI's host side and a stand-alone program
// (tests/hostsim/bkg_rbf_host_main.cpp): the refusals, the one-scale
// coordinates, a logarithm built from + - * / and bit operations (the same
// bits on the host, on the device and in numpy), the radial kernel, the
// smoothing weight, the pivot order of the LU, and host restatements of the
// system, the solve, the mean and the background of one plane.  B0-B3 and B7
// are bkg_host.h's.  Plain C++ unless compiled by hipcc, where the arithmetic
// is __host__ __device__.
//
// Everything from the selection on is double, every operation is rounded once
// and nothing may be contracted into a fused multiply-add.
#pragma once
#include "bkg_host.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sgpu_bkg_host {

constexpr int RBF_MAX_SAMPLES = SGPU_BKG_RBF_MAX_SAMPLES;       // boxes of the grid, so samples too
constexpr int RBF_MAX_ORDER = RBF_MAX_SAMPLES + 1;

// ---- R0 ----
inline const char *rbf_check(int W, int H, int S, double tol, double smooth, BkgGrid *g) {
    if (const char *why = bkg_grid(W, H, S, g)) return why;
    if (g->K > RBF_MAX_SAMPLES) return "subsky -rbf: more than 1024 sample boxes";
    if (!(tol >= 0.0) || !(tol <= 1.7976931348623157e308)) return "subsky: tolerance must be finite and >= 0";
    if (!(smooth >= 0.0) || !(smooth <= 1.0)) return "subsky -rbf: smooth must be in [0, 1]";
    return nullptr;
}

// ---- R1 ----
struct RbfAxes {
    double x0, y0, a;       // u = ((double)x - x0) * a, v = ((double)y - y0) * a
};
SGPU_BKG_HD inline RbfAxes rbf_axes(int W, int H) {
    RbfAxes ax;
    ax.x0 = (double)(W - 1) * 0.5;
    ax.y0 = (double)(H - 1) * 0.5;
    ax.a = 1.0 / (ax.x0 > ax.y0 ? ax.x0 : ax.y0);
    return ax;
}
SGPU_BKG_HD inline double rbf_u(int x, const RbfAxes &ax) { return ((double)x - ax.x0) * ax.a; }
SGPU_BKG_HD inline double rbf_v(int y, const RbfAxes &ax) { return ((double)y - ax.y0) * ax.a; }

// ---- R2 ----
SGPU_BKG_HD inline uint64_t rbf_bits(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
SGPU_BKG_HD inline double rbf_from_bits(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// log(s) of a positive normal s: s = 2^e m with m in (sqrt(1/2), sqrt(2)],
// z = (m - 1) / (m + 1), log m = 2 z sum_{k < 10} z^(2k) / (2k + 1) by Horner
// in z^2, and e ln 2 added in two parts.
SGPU_BKG_HD inline double rbf_log(double s) {
    constexpr double SQRT2 = 1.4142135623730951;
    constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const uint64_t b = rbf_bits(s);
    int e = (int)((b >> 52) & 0x7FFu) - 1023;
    double m = rbf_from_bits((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m > SQRT2) {
        m = m * 0.5;
        e = e + 1;
    }
    const double z = (m - 1.0) / (m + 1.0);
    const double z2 = z * z;
    double p = 1.0 / 19.0;
    p = p * z2;
    p = p + 1.0 / 17.0;
    p = p * z2;
    p = p + 1.0 / 15.0;
    p = p * z2;
    p = p + 1.0 / 13.0;
    p = p * z2;
    p = p + 1.0 / 11.0;
    p = p * z2;
    p = p + 1.0 / 9.0;
    p = p * z2;
    p = p + 1.0 / 7.0;
    p = p * z2;
    p = p + 1.0 / 5.0;
    p = p * z2;
    p = p + 1.0 / 3.0;
    p = p * z2;
    p = p + 1.0;
    const double r = (2.0 * z) * p;
    const double ed = (double)e;
    const double lo = ed * LN2_LO;
    const double t = lo + r;
    const double hi = ed * LN2_HI;
    return t + hi;
}

// phi(s) = r^2 log r of s = r^2
SGPU_BKG_HD inline double rbf_phi(double s) {
    const double h = 0.5 * s;
    const double l = rbf_log(s);
    return s == 0.0 ? 0.0 : h * l;
}
SGPU_BKG_HD inline double rbf_phi(double du, double dv) {
    const double a = du * du, b = dv * dv;
    return rbf_phi(a + b);
}

// ---- R3 ----
// host only (libm's pow): the kernel and the restatement are handed this double
inline double rbf_lam_rel(double smooth) { return 1e-4 * pow(10.0, 3.0 * (smooth - 0.5)); }

// ---- R4 ----
// The pivot of a column is the entry of the largest key, the lowest row among
// equals: |a| as its bit pattern, which puts a NaN above everything.
SGPU_BKG_HD inline uint64_t rbf_pivot_key(double a) { return rbf_bits(a) & 0x7FFFFFFFFFFFFFFFull; }
// a pivot that is 0 or not finite
SGPU_BKG_HD inline bool rbf_pivot_bad(double a) {
    const uint64_t k = rbf_pivot_key(a);
    return k == 0 || k >= 0x7FF0000000000000ull;
}

// ---- host restatements (the stand-alone program) ----

// [A | rhs] of order N, row stride N + 1, overwritten; x[N]; 0, or 2 with x = +0
inline int rbf_lu_solve_host(int N, double *aug, double *x) {
    const size_t ld = (size_t)N + 1;
    for (int i = 0; i < N; i++) x[i] = 0.0;
    for (int k = 0; k < N; k++) {
        int p = k;
        uint64_t best = rbf_pivot_key(aug[k * ld + k]);
        for (int i = k + 1; i < N; i++) {
            const uint64_t key = rbf_pivot_key(aug[i * ld + k]);
            if (key > best) {
                best = key;
                p = i;
            }
        }
        if (rbf_pivot_bad(aug[p * ld + k])) return 2;
        if (p != k)
            for (int j = k; j <= N; j++) std::swap(aug[k * ld + j], aug[p * ld + j]);
        for (int i = k + 1; i < N; i++) {
            const double l = aug[i * ld + k] / aug[k * ld + k];
            for (int j = k + 1; j <= N; j++) {
                const double t = l * aug[k * ld + j];
                aug[i * ld + j] = aug[i * ld + j] - t;
            }
        }
    }
    for (int i = N - 1; i >= 0; i--) {
        const double xi = aug[i * ld + N] / aug[i * ld + i];
        x[i] = xi;
        for (int j = 0; j < i; j++) {
            const double t = aug[j * ld + i] * xi;
            aug[j * ld + N] = aug[j * ld + N] - t;
        }
    }
    return 0;
}

struct RbfFit {
    int n = 0, status = 0;
    double mean_abs = 0.0, lambda = 0.0, mean = 0.0;
    std::vector<double> u, v, z, x;     // the samples, and the weights followed by the constant
};

// R0 - R5 of one plane from its medians and mask; weights, constant and mean are +0 unless the status is 0
inline RbfFit rbf_fit_host(const float *med, const uint8_t *keep, const BkgGrid &g, int W, int H, double lam_rel) {
    RbfFit f;
    const RbfAxes ax = rbf_axes(W, H);
    for (int k = 0; k < g.K; k++) {
        if (!keep[k]) continue;
        f.u.push_back(rbf_u(bkg_cx(g, k % g.nx), ax));
        f.v.push_back(rbf_v(bkg_cy(g, k / g.nx), ax));
        f.z.push_back((double)med[k]);
    }
    const int n = f.n = (int)f.z.size();
    f.x.assign((size_t)n + 1, 0.0);
    if (n == 0) {
        f.status = 1;
        return f;
    }
    const int N = n + 1;
    const size_t ld = (size_t)N + 1;
    std::vector<double> aug((size_t)N * ld, 0.0);
    double sum = 0.0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const double p = rbf_phi(f.u[(size_t)i] - f.u[(size_t)j], f.v[(size_t)i] - f.v[(size_t)j]);
            aug[i * ld + j] = p;
            sum = sum + fabs(p);
        }
    f.mean_abs = sum / ((double)n * (double)n);
    f.lambda = lam_rel * f.mean_abs;
    for (int i = 0; i < n; i++) {
        aug[i * ld + i] = aug[i * ld + i] + f.lambda;
        aug[i * ld + n] = 1.0;
        aug[n * ld + i] = 1.0;
        aug[i * ld + N] = f.z[(size_t)i];
    }
    f.status = rbf_lu_solve_host(N, aug.data(), f.x.data());
    if (f.status) return f;
    double s = 0.0;
    for (int i = 0; i < n; i++) s = s + f.z[(size_t)i];
    f.mean = s / (double)n;
    return f;
}

// R6 at one pixel
inline double rbf_background_host(const RbfFit &f, int x, int y, const RbfAxes &ax) {
    const double u = rbf_u(x, ax), v = rbf_v(y, ax);
    double acc = 0.0;
    for (int i = 0; i < f.n; i++) {
        const double t = f.x[(size_t)i] * rbf_phi(u - f.u[(size_t)i], v - f.v[(size_t)i]);
        acc = acc + t;
    }
    return acc + f.x[(size_t)f.n];
}

}  // namespace sgpu_bkg_host

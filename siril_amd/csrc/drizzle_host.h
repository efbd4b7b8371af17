// drizzle_host.h -- the arithmetic of the drizzle shared by the
// kernel (drizzle.hip), the C-ABI's host side and a stand-alone program
// (tests/hostsim/drizzle_host_main.cpp): the forward map, sgarea / boxer, the
// three drops, the running-mean update, the candidate window of the gather,
// and the argument checks, size rule and refusals.  Plain C++ unless compiled
// by hipcc, where the arithmetic is __host__ __device__.
//
// Coordinates and areas are double, samples / weights / the mean are float,
// and nothing may be contracted into a fused multiply-add.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/sirilgpu.h"

#if defined(__HIPCC__)
#define SGPU_DRZ_HD __host__ __device__
#else
#define SGPU_DRZ_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sgpu_drizzle_host {

constexpr double DRZ_SCALE_MIN = 0.1, DRZ_SCALE_MAX = 4.0;

SGPU_DRZ_HD inline bool drz_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for a NaN
SGPU_DRZ_HD inline double drz_min(double a, double b) { return b < a ? b : a; }
SGPU_DRZ_HD inline double drz_max(double a, double b) { return b > a ? b : a; }
// (int)v clipped to lo .. hi; v is finite
SGPU_DRZ_HD inline int drz_clip(double v, int lo, int hi) {
    return v < (double)lo ? lo : (v > (double)hi ? hi : (int)v);
}

// input point (u, v), pixel centres at integers -> output coordinates
SGPU_DRZ_HD inline void drz_map(const double *A, double scale, double u, double v, double &x, double &y) {
    const double X = A[0] * u + (A[1] * v + A[2]);
    const double Y = A[3] * u + (A[4] * v + A[5]);
    const double W = A[6] * u + (A[7] * v + A[8]);
    x = scale * (X / W + 0.5) - 0.5;
    y = scale * (Y / W + 0.5) - 0.5;
}

SGPU_DRZ_HD inline double drz_sgarea(double x1, double y1, double x2, double y2) {
    const double dx = x2 - x1, dy = y2 - y1;
    if (dx == 0.0) return 0.0;
    double xlo, xhi;
    if (dx < 0.0) {
        xlo = x2;
        xhi = x1;
    } else {
        xlo = x1;
        xhi = x2;
    }
    if (xlo >= 1.0 || xhi <= 0.0) return 0.0;
    xlo = drz_max(xlo, 0.0);
    xhi = drz_min(xhi, 1.0);
    const double m = dy / dx, c = y1 - m * x1;
    double ylo = m * xlo + c, yhi = m * xhi + c;
    if (ylo <= 0.0 && yhi <= 0.0) return 0.0;
    const double s = dx < 0.0 ? -1.0 : 1.0;
    if (ylo >= 1.0 && yhi >= 1.0) return s * (xhi - xlo);
    const double det = x1 * y2 - y1 * x2;
    if (ylo < 0.0) {
        ylo = 0.0;
        xlo = det / dy;
    }
    if (yhi < 0.0) {
        yhi = 0.0;
        xhi = det / dy;
    }
    if (ylo <= 1.0) {
        if (yhi <= 1.0) return s * 0.5 * (xhi - xlo) * (yhi + ylo);
        const double xtop = (dx + det) / dy;
        return s * (0.5 * (xtop - xlo) * (1.0 + ylo) + xhi - xtop);
    }
    const double xtop = (dx + det) / dy;
    return s * (0.5 * (xhi - xtop) * (1.0 + yhi) + xtop - xlo);
}

// the drop of one input pixel, SQUARE: mapped corners (in boxer's order), their area
struct DrzQuad {
    double qx[4], qy[4], jaco;
};

// area of the quad inside output pixel (X, Y)
SGPU_DRZ_HD inline double drz_boxer(double X, double Y, const DrzQuad &q) {
    double px[4], py[4];
    for (int k = 0; k < 4; k++) {
        px[k] = q.qx[k] - (X - 0.5);
        py[k] = q.qy[k] - (Y - 0.5);
    }
    double a = 0.0;
    for (int k = 0; k < 4; k++) a += drz_sgarea(px[k], py[k], px[(k + 1) & 3], py[(k + 1) & 3]);
    return a;
}

// false: the pixel is skipped (degenerate or non-finite quad)
SGPU_DRZ_HD inline bool drz_quad(const double *A, double scale, double pixfrac, int i, int j, DrzQuad &q) {
    const double dh = 0.5 * pixfrac, u = (double)i, v = (double)j;
    drz_map(A, scale, u - dh, v + dh, q.qx[0], q.qy[0]);
    drz_map(A, scale, u + dh, v + dh, q.qx[1], q.qy[1]);
    drz_map(A, scale, u + dh, v - dh, q.qx[2], q.qy[2]);
    drz_map(A, scale, u - dh, v - dh, q.qx[3], q.qy[3]);
    double jaco = 0.5 * ((q.qx[1] - q.qx[3]) * (q.qy[0] - q.qy[2]) - (q.qx[0] - q.qx[2]) * (q.qy[1] - q.qy[3]));
    if (jaco < 0.0) {   // a mirrored map
        jaco = -jaco;
        double t = q.qx[1];
        q.qx[1] = q.qx[3];
        q.qx[3] = t;
        t = q.qy[1];
        q.qy[1] = q.qy[3];
        q.qy[3] = t;
    }
    q.jaco = jaco;
    bool ok = jaco > 0.0;
    for (int k = 0; k < 4; k++) ok = ok && drz_finite(q.qx[k]) && drz_finite(q.qy[k]);
    return ok;
}

// output pixels the quad may touch: floor(min + 0.5) .. floor(max + 0.5), as doubles
SGPU_DRZ_HD inline void drz_quad_bounds(const DrzQuad &q, double &x0, double &x1, double &y0, double &y1) {
    double xl = q.qx[0], xh = q.qx[0], yl = q.qy[0], yh = q.qy[0];
    for (int k = 1; k < 4; k++) {
        xl = drz_min(xl, q.qx[k]);
        xh = drz_max(xh, q.qx[k]);
        yl = drz_min(yl, q.qy[k]);
        yh = drz_max(yh, q.qy[k]);
    }
    x0 = floor(xl + 0.5);
    x1 = floor(xh + 0.5);
    y0 = floor(yl + 0.5);
    y1 = floor(yh + 0.5);
}

// dow of a SQUARE drop on (X, Y), which lies inside the quad's bounds; 0: nothing lands
SGPU_DRZ_HD inline float drz_dow_square(const DrzQuad &q, double X, double Y, float w) {
    const double a = drz_boxer(X, Y, q);
    if (!(a > 0.0)) return 0.f;
    return (float)(a / q.jaco) * w;
}

// TURBO: centre (xo, yo), half-size r = 0.5 * pixfrac * scale
SGPU_DRZ_HD inline void drz_turbo_bounds(double xo, double yo, double r, double &x0, double &x1, double &y0,
                                         double &y1) {
    x0 = floor(xo - r + 0.5);
    x1 = floor(xo + r + 0.5);
    y0 = floor(yo - r + 0.5);
    y1 = floor(yo + r + 0.5);
}
SGPU_DRZ_HD inline float drz_dow_turbo(double xo, double yo, double r, double X, double Y, float w) {
    const double ox = drz_min(xo + r, X + 0.5) - drz_max(xo - r, X - 0.5);
    const double oy = drz_min(yo + r, Y + 0.5) - drz_max(yo - r, Y - 0.5);
    if (!(ox > 0.0 && oy > 0.0)) return 0.f;
    const double a = ox * oy;
    return (float)(a / ((2.0 * r) * (2.0 * r))) * w;
}

SGPU_DRZ_HD inline void drz_update(float &out, float &vc, float d, float dow) {
    const float vn = vc + dow;
    out = vc == 0.f ? d : ((out * vc) + (dow * d)) / vn;
    vc = vn;
}

// dow of input pixel (i, j) on output pixel (X, Y), maps computed here; 0: nothing lands
SGPU_DRZ_HD inline float drz_dow_pixel(const double *A, double scale, double pixfrac, int kernel, int i, int j,
                                       double X, double Y, float w) {
    if (kernel == SGPU_DRIZZLE_SQUARE) {
        DrzQuad q;
        if (!drz_quad(A, scale, pixfrac, i, j, q)) return 0.f;
        double x0, x1, y0, y1;
        drz_quad_bounds(q, x0, x1, y0, y1);
        if (X < x0 || X > x1 || Y < y0 || Y > y1) return 0.f;
        return drz_dow_square(q, X, Y, w);
    }
    double xo, yo;
    drz_map(A, scale, (double)i, (double)j, xo, yo);
    if (!drz_finite(xo) || !drz_finite(yo)) return 0.f;
    if (kernel == SGPU_DRIZZLE_TURBO) {
        const double r = 0.5 * pixfrac * scale;
        double x0, x1, y0, y1;
        drz_turbo_bounds(xo, yo, r, x0, x1, y0, y1);
        if (X < x0 || X > x1 || Y < y0 || Y > y1) return 0.f;
        return drz_dow_turbo(xo, yo, r, X, Y, w);
    }
    return (X == floor(xo + 0.5) && Y == floor(yo + 0.5)) ? w : 0.f;
}

// ---- the gather's candidate window ----
// An input pixel can land on an output rectangle only if its drop meets it.
// SQUARE: the shrunk square (half-size pixfrac / 2) meets the rectangle's
// preimage.  TURBO: the centre lies in the preimage of the rectangle grown by
// r.  POINT: the centre lies in the preimage.  So: grow the rectangle by
// drz_grow() in the output, take its four corners back through the scaling and
// M, and widen their bounding box by drz_widen() input pixels (one of them slack
// for the rounding of M, which is only inv3(A)).
SGPU_DRZ_HD inline double drz_grow(int kernel, double scale, double pixfrac) {
    return kernel == SGPU_DRIZZLE_TURBO ? 0.5 * pixfrac * scale : 0.0;
}
SGPU_DRZ_HD inline double drz_widen(int kernel, double pixfrac) {
    return kernel == SGPU_DRIZZLE_SQUARE ? 0.5 * pixfrac + 1.0 : 1.0;
}

// Output rectangle with edges xl .. xh, yl .. yh (pixel (X, Y) spans X - 0.5 .. X + 0.5) -> the box
// u0 .. u1, v0 .. v1 of input coordinates, already widened.  false: W of M is zero or changes sign
// over the corners, or a bound is not finite (the host's refusals rule this out inside the output).
SGPU_DRZ_HD inline bool drz_window(const double *M, double scale, double xl, double xh, double yl, double yh,
                                   double widen, double &u0, double &u1, double &v0, double &v1) {
    bool ok = true;
    int sgn = 0;
    for (int k = 0; k < 4; k++) {
        const double x = ((k & 1 ? xh : xl) + 0.5) / scale - 0.5, y = ((k >> 1 ? yh : yl) + 0.5) / scale - 0.5;
        const double U = M[0] * x + (M[1] * y + M[2]);
        const double V = M[3] * x + (M[4] * y + M[5]);
        const double Wd = M[6] * x + (M[7] * y + M[8]);
        const int s = Wd > 0.0 ? 1 : (Wd < 0.0 ? -1 : 0);
        if (k == 0) sgn = s;
        if (s == 0 || s != sgn) ok = false;
        const double iw = 1.0 / Wd, u = U * iw, v = V * iw;   // bounds only: one division, not two
        if (k == 0) {
            u0 = u1 = u;
            v0 = v1 = v;
        } else {
            u0 = drz_min(u0, u);
            u1 = drz_max(u1, u);
            v0 = drz_min(v0, v);
            v1 = drz_max(v1, v);
        }
    }
    u0 -= widen;
    u1 += widen;
    v0 -= widen;
    v1 += widen;
    return ok && drz_finite(u0) && drz_finite(u1) && drz_finite(v0) && drz_finite(v1);
}

// the window as pixel indices clipped to lo .. hi per axis; empty when i1 < i0 or j1 < j0
SGPU_DRZ_HD inline void drz_window_clip(double u0, double u1, double v0, double v1, int ilo, int ihi, int jlo, int jhi,
                                        int &i0, int &i1, int &j0, int &j1) {
    i0 = drz_clip(floor(u0), ilo, ihi + 1);
    i1 = drz_clip(ceil(u1), ilo - 1, ihi);
    j0 = drz_clip(floor(v0), jlo, jhi + 1);
    j1 = drz_clip(ceil(v1), jlo - 1, jhi);
}

template <typename T>
SGPU_DRZ_HD inline float drz_sample(T v) {
    return (float)v;
}

// One output pixel from global memory: candidates i0 .. i1 x j0 .. j1 in input raster order.
template <typename T>
SGPU_DRZ_HD inline void drz_gather_pixel(const T *in, const float *pw, int W, const double *A, double scale,
                                         double pixfrac, int kernel, int i0, int i1, int j0, int j1, int X, int Y,
                                         float &out, float &vc) {
    out = 0.f;
    vc = 0.f;
    for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
            const float w = pw ? pw[(long long)j * W + i] : 1.f;
            if (w == 0.f) continue;
            const float dow = drz_dow_pixel(A, scale, pixfrac, kernel, i, j, (double)X, (double)Y, w);
            if (dow > 0.f) drz_update(out, vc, drz_sample(in[(long long)j * W + i]), dow);
        }
}

// ---- CFA frames: one (out, vc) pair per colour, an input pixel updates its own colour's only ----

// colour (0 R, 1 G, 2 B) of memory-order input pixel (i, j); pattern holds dim * dim entries
SGPU_DRZ_HD inline int drz_cfa_colour(const unsigned char *pattern, int dim, int i, int j) {
    return pattern[(j % dim) * dim + (i % dim)];
}

// drz_update on the pair of colour c.  The pair is selected in and out: c is a run-time value and
// must not index registers.
SGPU_DRZ_HD inline void drz_update_cfa(float &o0, float &v0, float &o1, float &v1, float &o2, float &v2, int c,
                                       float d, float dow) {
    float o = c == 0 ? o0 : (c == 1 ? o1 : o2), v = c == 0 ? v0 : (c == 1 ? v1 : v2);
    drz_update(o, v, d, dow);
    o0 = c == 0 ? o : o0;
    v0 = c == 0 ? v : v0;
    o1 = c == 1 ? o : o1;
    v1 = c == 1 ? v : v1;
    o2 = c == 2 ? o : o2;
    v2 = c == 2 ? v : v2;
}

// drz_gather_pixel of a CFA frame: out[c], vc[c] of the three colours
template <typename T>
SGPU_DRZ_HD inline void drz_gather_pixel_cfa(const T *in, const float *pw, const unsigned char *pattern, int dim,
                                             int W, const double *A, double scale, double pixfrac, int kernel,
                                             int i0, int i1, int j0, int j1, int X, int Y, float out[3],
                                             float vc[3]) {
    float o0 = 0.f, v0 = 0.f, o1 = 0.f, v1 = 0.f, o2 = 0.f, v2 = 0.f;
    for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
            const float w = pw ? pw[(long long)j * W + i] : 1.f;
            if (w == 0.f) continue;
            const float dow = drz_dow_pixel(A, scale, pixfrac, kernel, i, j, (double)X, (double)Y, w);
            if (dow > 0.f)
                drz_update_cfa(o0, v0, o1, v1, o2, v2, drz_cfa_colour(pattern, dim, i, j),
                               drz_sample(in[(long long)j * W + i]), dow);
        }
    out[0] = o0;
    out[1] = o1;
    out[2] = o2;
    vc[0] = v0;
    vc[1] = v1;
    vc[2] = v2;
}

// ---- host side: checks, size rule, maps, refusals ----

// nullptr when the pattern is a Bayer (dim 2) or X-Trans (dim 6) one of entries 0 .. 2, else what is wrong
inline const char *drz_check_pattern(const unsigned char *pattern, int dim) {
    if (!pattern) return "drizzle: no CFA pattern";
    if (dim != 2 && dim != 6) return "drizzle: the CFA pattern is 2 x 2 (Bayer) or 6 x 6 (X-Trans)";
    for (int k = 0; k < dim * dim; k++)
        if (pattern[k] > 2) return "drizzle: CFA pattern entries are 0 (R), 1 (G) or 2 (B)";
    return nullptr;
}

// nullptr when the parameters are in range, else what is wrong
inline const char *drz_check_params(const sgpu_drizzle_params *p) {
    if (!p) return "drizzle: no parameters";
    if (!(p->scale >= DRZ_SCALE_MIN && p->scale <= DRZ_SCALE_MAX)) return "drizzle: 0.1 <= scale <= 4";
    if (!(p->pixfrac > 0.0 && p->pixfrac <= 1.0)) return "drizzle: 0 < pixfrac <= 1";
    if (p->kernel != SGPU_DRIZZLE_POINT && p->kernel != SGPU_DRIZZLE_TURBO && p->kernel != SGPU_DRIZZLE_SQUARE)
        return "drizzle: unknown kernel (point, turbo, square)";
    return nullptr;
}

inline const char *drz_output_size(int width, int height, double scale, int *out_w, int *out_h) {
    if (width < 1 || height < 1) return "drizzle: bad frame size";
    if (!(scale >= DRZ_SCALE_MIN && scale <= DRZ_SCALE_MAX)) return "drizzle: 0.1 <= scale <= 4";
    const double w = floor((double)width * scale + 0.5), h = floor((double)height * scale + 0.5);
    if (w < 1.0 || h < 1.0 || w > 2147483647.0 || h > 2147483647.0) return "drizzle: output size out of range";
    *out_w = (int)w;
    *out_h = (int)h;
    return nullptr;
}

// closed-form inverse: adjugate over the determinant, in the operation order of the frame warp (6d)
inline bool drz_inv3(const double *m, double *o) {
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

// A[f] = F * ((Href^-1 * Hf) * F), F = [[1, 0, 0], [0, -1, height - 1], [0, 0, 1]]: the forward
// memory-order map of the frame warp before its inversion
inline const char *drz_forward_maps(int nframes, const double *H, int ref_index, int height, double *A) {
    if (nframes < 1 || !H || !A || ref_index < 0 || ref_index >= nframes || height < 1) return "bad argument";
    for (size_t k = 0; k < 9 * (size_t)nframes; k++)
        if (!std::isfinite(H[k])) return "drizzle: non-finite homography entry";
    double R[9];
    if (!drz_inv3(H + 9 * (size_t)ref_index, R)) return "drizzle: singular reference homography";
    const double hm1 = (double)(height - 1);
    for (int fr = 0; fr < nframes; fr++) {
        const double *Hf = H + 9 * (size_t)fr;
        double Hc[9], B[9], *Hm = A + 9 * (size_t)fr, inv[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                Hc[3 * r + c] = (R[3 * r] * Hf[c] + R[3 * r + 1] * Hf[3 + c]) + R[3 * r + 2] * Hf[6 + c];
        for (int r = 0; r < 3; r++) {
            B[3 * r] = Hc[3 * r];
            B[3 * r + 1] = -Hc[3 * r + 1];
            B[3 * r + 2] = hm1 * Hc[3 * r + 1] + Hc[3 * r + 2];
        }
        for (int c = 0; c < 3; c++) {
            Hm[c] = B[c];
            Hm[3 + c] = -B[3 + c] + hm1 * B[6 + c];
            Hm[6 + c] = B[6 + c];
        }
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(Hm[k])) return "drizzle: singular or non-finite map";
        if (!drz_inv3(Hm, inv)) return "drizzle: singular or non-finite map";
    }
    return nullptr;
}

// does the third row of a map keep one non-zero sign over the corners xl / xh x yl / yh
inline bool drz_w_regular(const double *P, double xl, double xh, double yl, double yh) {
    int sgn = 0;
    for (int k = 0; k < 4; k++) {
        const double x = k & 1 ? xh : xl, y = k >> 1 ? yh : yl;
        const double Wd = P[6] * x + (P[7] * y + P[8]);
        const int s = Wd > 0.0 ? 1 : (Wd < 0.0 ? -1 : 0);
        if (k == 0) sgn = s;
        if (s == 0 || s != sgn) return false;
    }
    return true;
}

// One frame's maps: M = inv3(A), and both regular on their domains.  The input frame is taken at
// (-1, -1) .. (width, height); the output frame at its pixel edges grown by drz_grow() (the reach
// of a TURBO drop), mapped back to scale 1.
inline const char *drz_frame_maps(const double *A, int width, int height, int out_w, int out_h,
                                  const sgpu_drizzle_params *p, double *M) {
    if (!drz_inv3(A, M)) return "drizzle: singular or non-finite map";
    if (!drz_w_regular(A, -1.0, (double)width, -1.0, (double)height))
        return "drizzle: the map's denominator vanishes or changes sign inside the frame";
    const double g = drz_grow(p->kernel, p->scale, p->pixfrac);
    const double xl = (-0.5 - g + 0.5) / p->scale - 0.5, xh = ((double)out_w - 0.5 + g + 0.5) / p->scale - 0.5;
    const double yl = (-0.5 - g + 0.5) / p->scale - 0.5, yh = ((double)out_h - 0.5 + g + 0.5) / p->scale - 0.5;
    if (!drz_w_regular(M, xl, xh, yl, yh))
        return "drizzle: the inverse map's denominator vanishes or changes sign inside the output";
    return nullptr;
}

// ---- host restatements of one frame (the stand-alone program; the kernel's reference) ----

// the sequential scatter: the order of the contract
template <typename T>
inline void drz_scatter_frame(const T *in, const float *pw, int W, int H, const double *A,
                              const sgpu_drizzle_params *p, int OW, int OH, float *out, float *vc) {
    for (size_t k = 0; k < (size_t)OW * (size_t)OH; k++) out[k] = vc[k] = 0.f;
    const double r = 0.5 * p->pixfrac * p->scale;
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            const float w = pw ? pw[(size_t)j * W + i] : 1.f;
            if (w == 0.f) continue;
            const float d = drz_sample(in[(size_t)j * W + i]);
            double x0, x1, y0, y1;
            DrzQuad q;
            double xo = 0.0, yo = 0.0;
            if (p->kernel == SGPU_DRIZZLE_SQUARE) {
                if (!drz_quad(A, p->scale, p->pixfrac, i, j, q)) continue;
                drz_quad_bounds(q, x0, x1, y0, y1);
            } else {
                drz_map(A, p->scale, (double)i, (double)j, xo, yo);
                if (!drz_finite(xo) || !drz_finite(yo)) continue;
                if (p->kernel == SGPU_DRIZZLE_TURBO) drz_turbo_bounds(xo, yo, r, x0, x1, y0, y1);
                else {
                    x0 = x1 = floor(xo + 0.5);
                    y0 = y1 = floor(yo + 0.5);
                }
            }
            const int X0 = drz_clip(x0, 0, OW), X1 = drz_clip(x1, -1, OW - 1);
            const int Y0 = drz_clip(y0, 0, OH), Y1 = drz_clip(y1, -1, OH - 1);
            for (int Y = Y0; Y <= Y1; Y++)
                for (int X = X0; X <= X1; X++) {
                    float dow;
                    if (p->kernel == SGPU_DRIZZLE_SQUARE) dow = drz_dow_square(q, (double)X, (double)Y, w);
                    else if (p->kernel == SGPU_DRIZZLE_TURBO) dow = drz_dow_turbo(xo, yo, r, (double)X, (double)Y, w);
                    else dow = w;
                    if (dow > 0.f) drz_update(out[(size_t)Y * OW + X], vc[(size_t)Y * OW + X], d, dow);
                }
        }
}

// the gather, one output pixel after the other, as the kernel's direct path runs it
template <typename T>
inline void drz_gather_frame(const T *in, const float *pw, int W, int H, const double *A, const double *M,
                             const sgpu_drizzle_params *p, int OW, int OH, float *out, float *vc) {
    const double g = drz_grow(p->kernel, p->scale, p->pixfrac), wd = drz_widen(p->kernel, p->pixfrac);
    for (int Y = 0; Y < OH; Y++)
        for (int X = 0; X < OW; X++) {
            double u0, u1, v0, v1;
            int i0 = 0, i1 = W - 1, j0 = 0, j1 = H - 1;   // an irregular window: every pixel is a candidate
            if (drz_window(M, p->scale, X - 0.5 - g, X + 0.5 + g, Y - 0.5 - g, Y + 0.5 + g, wd, u0, u1, v0, v1))
                drz_window_clip(u0, u1, v0, v1, 0, W - 1, 0, H - 1, i0, i1, j0, j1);
            drz_gather_pixel(in, pw, W, A, p->scale, p->pixfrac, p->kernel, i0, i1, j0, j1, X, Y,
                             out[(size_t)Y * OW + X], vc[(size_t)Y * OW + X]);
        }
}

// drz_scatter_frame of a CFA frame: planes out[c * plane + Y * OW + X], plane >= OW * OH, of the
// three colours; the pixel of colour c updates plane c only
template <typename T>
SGPU_DRZ_HD inline void drz_scatter_frame_cfa(const T *in, const float *pw, const unsigned char *pattern, int dim,
                                              int W, int H, const double *A, const sgpu_drizzle_params *p, int OW,
                                              int OH, size_t plane, float *out, float *vc) {
    for (int c = 0; c < 3; c++)
        for (size_t k = 0; k < (size_t)OW * (size_t)OH; k++) out[c * plane + k] = vc[c * plane + k] = 0.f;
    const double r = 0.5 * p->pixfrac * p->scale;
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            const float w = pw ? pw[(size_t)j * W + i] : 1.f;
            if (w == 0.f) continue;
            const float d = drz_sample(in[(size_t)j * W + i]);
            const size_t base = (size_t)drz_cfa_colour(pattern, dim, i, j) * plane;
            double x0, x1, y0, y1;
            DrzQuad q;
            double xo = 0.0, yo = 0.0;
            if (p->kernel == SGPU_DRIZZLE_SQUARE) {
                if (!drz_quad(A, p->scale, p->pixfrac, i, j, q)) continue;
                drz_quad_bounds(q, x0, x1, y0, y1);
            } else {
                drz_map(A, p->scale, (double)i, (double)j, xo, yo);
                if (!drz_finite(xo) || !drz_finite(yo)) continue;
                if (p->kernel == SGPU_DRIZZLE_TURBO) drz_turbo_bounds(xo, yo, r, x0, x1, y0, y1);
                else {
                    x0 = x1 = floor(xo + 0.5);
                    y0 = y1 = floor(yo + 0.5);
                }
            }
            const int X0 = drz_clip(x0, 0, OW), X1 = drz_clip(x1, -1, OW - 1);
            const int Y0 = drz_clip(y0, 0, OH), Y1 = drz_clip(y1, -1, OH - 1);
            for (int Y = Y0; Y <= Y1; Y++)
                for (int X = X0; X <= X1; X++) {
                    float dow;
                    if (p->kernel == SGPU_DRIZZLE_SQUARE) dow = drz_dow_square(q, (double)X, (double)Y, w);
                    else if (p->kernel == SGPU_DRIZZLE_TURBO) dow = drz_dow_turbo(xo, yo, r, (double)X, (double)Y, w);
                    else dow = w;
                    if (dow > 0.f) drz_update(out[base + (size_t)Y * OW + X], vc[base + (size_t)Y * OW + X], d, dow);
                }
        }
}

// drz_gather_frame of a CFA frame, planes as drz_scatter_frame_cfa lays them out
template <typename T>
inline void drz_gather_frame_cfa(const T *in, const float *pw, const unsigned char *pattern, int dim, int W, int H,
                                 const double *A, const double *M, const sgpu_drizzle_params *p, int OW, int OH,
                                 size_t plane, float *out, float *vc) {
    const double g = drz_grow(p->kernel, p->scale, p->pixfrac), wd = drz_widen(p->kernel, p->pixfrac);
    for (int Y = 0; Y < OH; Y++)
        for (int X = 0; X < OW; X++) {
            double u0, u1, v0, v1;
            int i0 = 0, i1 = W - 1, j0 = 0, j1 = H - 1;   // an irregular window: every pixel is a candidate
            if (drz_window(M, p->scale, X - 0.5 - g, X + 0.5 + g, Y - 0.5 - g, Y + 0.5 + g, wd, u0, u1, v0, v1))
                drz_window_clip(u0, u1, v0, v1, 0, W - 1, 0, H - 1, i0, i1, j0, j1);
            float o[3], v[3];
            drz_gather_pixel_cfa(in, pw, pattern, dim, W, A, p->scale, p->pixfrac, p->kernel, i0, i1, j0, j1, X, Y, o,
                                 v);
            for (int c = 0; c < 3; c++) {
                out[c * plane + (size_t)Y * OW + X] = o[c];
                vc[c * plane + (size_t)Y * OW + X] = v[c];
            }
        }
}

}  // namespace sgpu_drizzle_host

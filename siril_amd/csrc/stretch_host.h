// stretch_host.h -- the arithmetic of the stretches
// shared by the kernel (stretch.hip), the C-ABI's host side and a stand-alone
// program (tests/hostsim/stretch_host_main.cpp): the refusals, the input
// conversion, exp / pow / asinh built on 6k's logarithm from + - * /, sqrt and
// bit operations (the same bits on the host, on the device and in numpy), the
// midtones transfer function and the autostretch parameters, the linear and
// the asinh stretch, the generalised hyperbolic stretch with its coefficient
// block and its closed-form inverse, and the colour models.  Plain C++ unless
// compiled by hipcc, where the arithmetic is __host__ __device__.
//
// Everything between the input and the one rounding to float is double, every
// operation is rounded once and nothing may be contracted into a fused
// multiply-add.  The order of operations below is the specification;
// tests/stretch_ref.py follows it literally.
#pragma once
#include "bkg_rbf_host.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define SGPU_STR_HD SGPU_BKG_HD

namespace sgpu_str_host {

using sgpu_bkg_host::rbf_bits;
using sgpu_bkg_host::rbf_from_bits;
using sgpu_bkg_host::rbf_log;

constexpr double STR_TINY = 2.2250738585072014e-308;        // 2^-1022, the floor of T8's log and pow arguments
constexpr double STR_EXP_MIN = -708.0, STR_EXP_MAX = 708.0;
constexpr double STR_MAD_SIGMA = 1.4826;
constexpr double STR_HUMAN_R = 0.2126, STR_HUMAN_G = 0.7152, STR_HUMAN_B = 0.0722;
constexpr double STR_THIRD = 1.0 / 3.0;

// what a coefficient block holds, by function (T6)
enum { C_LO = 0, C_M = 1, C_HI = 2, C_RANGE = 3, C_M1 = 4, C_M2 = 5 };                       // mtf
enum { C_BP = 0, C_BPD = 1 };                                                                 // linstretch
enum { C_BETA = 0, C_OFF = 1, C_OFFD = 2, C_AB = 3 };                                         // asinh
enum { G_D = 0, G_B = 1, G_AB = 2, G_LP = 3, G_SP = 4, G_HP = 5, G_A1 = 6, G_S1 = 7, G_A2 = 8, G_S2 = 9,
       G_S0 = 10, G_SPAN = 11, G_INV = 12, G_P1 = 13, G_P2 = 14, G_BD = 15 };                 // ght family
// the form of q (T5)
enum { Q_LOG = 0, Q_NEG = 1, Q_EXP = 2, Q_POS = 3, Q_ASINH = 4, Q_IDENTITY = 5 };

struct StrCoef {
    double c[SGPU_STRETCH_NCOEF];
    int fn, regime, model, clipmode, mask;
};

// ---- T0: input ----
SGPU_STR_HD inline double str_widen(float v) { return (double)v; }
SGPU_STR_HD inline double str_widen(uint16_t v) { return (double)v / 65535.0; }
SGPU_STR_HD inline double str_clip01(double v) {
    v = v < 0.0 ? 0.0 : v;
    return v > 1.0 ? 1.0 : v;
}

// ---- T1: transcendentals ----
SGPU_STR_HD inline double str_log(double s) {
    const double r = rbf_log(s);
    return s != s ? s : r;
}
SGPU_STR_HD inline double str_floor_arg(double s) { return s < STR_TINY ? STR_TINY : s; }

// exp(x), total: x is clamped to [-708, 708]; n = floor(x / ln 2 + 1/2), r = (x - n LN2_HI) - n LN2_LO,
// exp r = sum_{k <= 13} r^k / k! by Horner, scaled by 2^n put together from bits
SGPU_STR_HD inline double str_exp(double x) {
    constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    constexpr double INV_LN2 = 1.4426950408889634;
    double xc = x < STR_EXP_MIN ? STR_EXP_MIN : x;
    xc = xc > STR_EXP_MAX ? STR_EXP_MAX : xc;
    xc = x != x ? 0.0 : xc;
    const double tn = xc * INV_LN2;
    const double nd = __builtin_floor(tn + 0.5);
    const double hi = nd * LN2_HI;
    const double lo = nd * LN2_LO;
    const double r = (xc - hi) - lo;
    double p = 1.0 / 6227020800.0;
    p = p * r;
    p = p + 1.0 / 479001600.0;
    p = p * r;
    p = p + 1.0 / 39916800.0;
    p = p * r;
    p = p + 1.0 / 3628800.0;
    p = p * r;
    p = p + 1.0 / 362880.0;
    p = p * r;
    p = p + 1.0 / 40320.0;
    p = p * r;
    p = p + 1.0 / 5040.0;
    p = p * r;
    p = p + 1.0 / 720.0;
    p = p * r;
    p = p + 1.0 / 120.0;
    p = p * r;
    p = p + 1.0 / 24.0;
    p = p * r;
    p = p + 1.0 / 6.0;
    p = p * r;
    p = p + 0.5;
    p = p * r;
    p = p + 1.0;
    p = p * r;
    p = p + 1.0;
    const int n = (int)nd;
    const double scale = rbf_from_bits((uint64_t)(n + 1023) << 52);
    const double res = p * scale;
    return x != x ? x : res;
}
SGPU_STR_HD inline double str_pow(double a, double p) {
    const double l = str_log(a);
    return str_exp(p * l);
}
SGPU_STR_HD inline double str_asinh(double v) {
    const double s = __builtin_sqrt(v * v + 1.0);
    return str_log(v + s);
}

// ---- T2: the midtones transfer function of xp in [0, 1] ----
SGPU_STR_HD inline double str_mtf01(double xp, double m, double m1, double m2) {
    const double num = m1 * xp;
    const double den = m2 * xp - m;
    const double r = num / den;
    return xp == 0.0 ? 0.0 : (xp == 1.0 ? 1.0 : r);
}
SGPU_STR_HD inline double str_mtf01(double xp, double m) { return str_mtf01(xp, m, m - 1.0, 2.0 * m - 1.0); }
SGPU_STR_HD inline double str_mtf(const double *c, double x) {
    const double xp = str_clip01((x - c[C_LO]) / c[C_RANGE]);
    return str_mtf01(xp, c[C_M], c[C_M1], c[C_M2]);
}

// ---- T3: the autostretch parameters (host) ----
// nullptr and out[3*p + 0..2] = lo, m, hi, or what is refused
inline const char *str_autostretch(const double *stats, const int *status, int nimages, int nch, double unit,
                                   int linked, double clip, double target, double *out) {
    if (!stats || !status || !out) return "autostretch: null argument";
    if (nimages < 0 || nch < 1) return "autostretch: bad number of planes";
    if (!(unit == 1.0 || unit == 65535.0)) return "autostretch: the unit must be 1 or 65535";
    if (!(clip <= 0.0) || !(clip >= -1.7976931348623157e308)) return "autostretch: the shadows clip must be finite and <= 0";
    if (!(target > 0.0) || !(target < 1.0)) return "autostretch: the target background must be inside (0, 1)";
    auto finish = [&](double med, double edge, bool inv, double *o) -> const char * {
        const double lo = inv ? 0.0 : edge, hi = inv ? edge : 1.0;
        if (!(hi > lo)) return "autostretch: the plane has no spread";
        const double xm = str_clip01((inv ? hi - med : med - lo) / (hi - lo));
        const double t = str_mtf01(xm, target);
        const double m = inv ? 1.0 - t : t;
        if (!(m > 0.0) || !(m < 1.0)) return "autostretch: the plane has no spread";
        o[0] = lo, o[1] = m, o[2] = hi;
        return nullptr;
    };
    for (int i = 0; i < nimages; i++) {
        int ninv = 0;
        for (int c = 0; c < nch; c++) {
            const size_t p = (size_t)i * nch + c;
            if (status[p] != 0) return "autostretch: a plane has no statistics (status != 0)";
            ninv += stats[4 * p] / unit > 0.5;
        }
        const bool inv_all = 2 * ninv > nch;
        double sum_med = 0.0, sum_edge = 0.0;
        for (int c = 0; c < nch; c++) {
            const size_t p = (size_t)i * nch + c;
            const double med = stats[4 * p] / unit, mad = stats[4 * p + 1] / unit;
            const double sig = STR_MAD_SIGMA * mad;
            const double cs = clip * sig;
            const bool inv = linked ? inv_all : med > 0.5;
            const double edge = str_clip01(inv ? med - cs : med + cs);
            if (!linked) {
                if (const char *why = finish(med, edge, inv, out + 3 * p)) return why;
            }
            sum_med = sum_med + med;
            sum_edge = sum_edge + edge;
        }
        if (linked) {
            double o[3];
            if (const char *why = finish(sum_med / (double)nch, sum_edge / (double)nch, inv_all, o)) return why;
            for (int c = 0; c < nch; c++)
                for (int k = 0; k < 3; k++) out[3 * ((size_t)i * nch + c) + k] = o[k];
        }
    }
    return nullptr;
}

// ---- T4: linstretch and asinh ----
SGPU_STR_HD inline double str_lin(const double *c, double x) {
    const double v = (x - c[C_BP]) / c[C_BPD];
    return v < 0.0 ? 0.0 : v;
}
SGPU_STR_HD inline double str_asinh_pre(const double *c, double x) {
    double v = x - c[C_OFF];
    v = v < 0.0 ? 0.0 : v;
    return v / c[C_OFFD];
}
SGPU_STR_HD inline double str_asinh_k(const double *c, double v) {
    const double num = str_asinh(c[C_BETA] * v);
    const double den = v * c[C_AB];
    const double k = num / den;
    return v == 0.0 ? 1.0 : k;
}
SGPU_STR_HD inline double str_min1(double v) { return v > 1.0 ? 1.0 : v; }

// ---- T5: q, q' and the inverse of q, u and v >= 0 ----
SGPU_STR_HD inline double str_q(const double *c, int regime, double u) {
    const double du = c[G_D] * u;
    const double w = 1.0 + c[G_BD] * u;
    switch (regime) {
        case Q_LOG: return str_log(1.0 + du);
        case Q_NEG: return (1.0 - str_pow(w, c[G_P1])) / (1.0 - c[G_AB]);
        case Q_EXP: return 1.0 - str_exp(-du);
        case Q_POS: return 1.0 - str_pow(w, c[G_P1]);
        default: return str_asinh(du);
    }
}
SGPU_STR_HD inline double str_dq(const double *c, int regime, double u) {
    const double du = c[G_D] * u;
    const double w = 1.0 + c[G_BD] * u;
    switch (regime) {
        case Q_LOG: return c[G_D] / (1.0 + du);
        case Q_NEG: return c[G_D] * str_pow(w, -1.0 / c[G_AB]);
        case Q_EXP: return c[G_D] * str_exp(-du);
        case Q_POS: return c[G_D] * str_pow(w, -(1.0 + c[G_B]) / c[G_B]);
        default: return c[G_D] / __builtin_sqrt(1.0 + du * du);
    }
}
SGPU_STR_HD inline double str_qinv(const double *c, int regime, double v) {
    switch (regime) {
        case Q_LOG: return (str_exp(v) - 1.0) / c[G_D];
        case Q_NEG: {
            const double base = 1.0 - v * (1.0 - c[G_AB]);
            return (str_pow(str_floor_arg(base), c[G_P2]) - 1.0) / c[G_BD];
        }
        case Q_EXP: return -str_log(str_floor_arg(1.0 - v)) / c[G_D];
        case Q_POS: return (str_pow(str_floor_arg(1.0 - v), c[G_P2]) - 1.0) / c[G_BD];
        default: {
            const double e1 = str_exp(v), e2 = str_exp(-v);
            return ((e1 - e2) * 0.5) / c[G_D];
        }
    }
}

// ---- T7: S, T and the inverse of T.  One q per sample whatever the piece: t = clip(x, LP, HP), u = |t - SP|,
// the sign of t - SP, and a linear term whose slope is q' at the lower end, at the upper end, or 0. ----
SGPU_STR_HD inline double str_S(const double *c, int regime, double x) {
    double t = x < c[G_LP] ? c[G_LP] : x;
    t = t > c[G_HP] ? c[G_HP] : t;
    const double d = t - c[G_SP];
    const double u = d < 0.0 ? -d : d;
    const double qv = str_q(c, regime, u);
    const double sq = d < 0.0 ? -qv : qv;
    const double slope = x < c[G_LP] ? c[G_S1] : (x > c[G_HP] ? c[G_S2] : 0.0);
    const double lin = slope * (x - t);
    return sq + lin;
}
SGPU_STR_HD inline double str_T(const double *c, int regime, double x) {
    if (regime == Q_IDENTITY) return x;
    const double s = str_S(c, regime, x);
    return str_clip01((s - c[G_S0]) * c[G_INV]);
}
SGPU_STR_HD inline double str_Tinv(const double *c, int regime, double y) {
    if (regime == Q_IDENTITY) return y;
    const double s = c[G_S0] + y * c[G_SPAN];
    const double lo = -c[G_A1];
    double sc = s < lo ? lo : s;
    sc = sc > c[G_A2] ? c[G_A2] : sc;
    const double v = sc < 0.0 ? -sc : sc;
    const double u = str_qinv(c, regime, v);
    const double xq = sc < 0.0 ? c[G_SP] - u : c[G_SP] + u;
    const double slope = s < lo ? c[G_S1] : (s > c[G_A2] ? c[G_S2] : 1.0);
    const double lin = (s - sc) / str_floor_arg(slope);
    return str_clip01(xq + lin);
}
SGPU_STR_HD inline bool str_is_inverse(int fn) { return fn == SGPU_STRETCH_INVGHT || fn == SGPU_STRETCH_INVMODASINH; }
// the transfer of the ght family, forward or inverse, of x in [0, 1]
SGPU_STR_HD inline double str_transfer(const StrCoef &k, double x) {
    return str_is_inverse(k.fn) ? str_Tinv(k.c, k.regime, x) : str_T(k.c, k.regime, x);
}

// ---- refusals (T9) and the coefficient block (T6), host ----
inline const char *str_check(const sgpu_stretch_params &p) {
    auto in01 = [](double v) { return v >= 0.0 && v <= 1.0; };
    if (p.function < SGPU_STRETCH_MTF || p.function > SGPU_STRETCH_INVMODASINH) return "stretch: unknown function";
    if (p.model < SGPU_STRETCH_INDEPENDENT || p.model > SGPU_STRETCH_EVEN) return "stretch: unknown colour model";
    if (p.clipmode < SGPU_STRETCH_CLIP || p.clipmode > SGPU_STRETCH_RGBBLEND) return "stretch: unknown clip mode";
    if (p.mask < 1 || p.mask > 7) return "stretch: the channel mask must be 1 .. 7";
    switch (p.function) {
        case SGPU_STRETCH_MTF:
            if (!in01(p.lo) || !in01(p.hi)) return "mtf: low and high must be in [0, 1]";
            if (!(p.hi > p.lo)) return "mtf: high must be above low";
            if (!(p.m > 0.0) || !(p.m < 1.0)) return "mtf: the midtones balance must be inside (0, 1)";
            return nullptr;
        case SGPU_STRETCH_LINEAR:
            if (!(p.BP >= 0.0) || !(p.BP < 1.0)) return "linstretch: BP must be in [0, 1)";
            return nullptr;
        case SGPU_STRETCH_ASINH:
            if (!(p.beta >= 1.0) || !(p.beta <= 1000.0)) return "asinh: the stretch must be in [1, 1000]";
            if (!(p.offset >= 0.0) || !(p.offset < 1.0)) return "asinh: the offset must be in [0, 1)";
            return nullptr;
        default:
            if (!(p.D >= 0.0) || !(p.D <= 10.0)) return "ght: D must be in [0, 10]";
            if ((p.function == SGPU_STRETCH_GHT || p.function == SGPU_STRETCH_INVGHT) &&
                (!(p.B >= -5.0) || !(p.B <= 15.0)))
                return "ght: B must be in [-5, 15]";
            if (!in01(p.LP) || !in01(p.SP) || !in01(p.HP) || !(p.LP <= p.SP) || !(p.SP <= p.HP))
                return "ght: 0 <= LP <= SP <= HP <= 1 must hold";
            return nullptr;
    }
}

// nullptr and *k filled, or what is refused
inline const char *str_coeffs(const sgpu_stretch_params &p, StrCoef *k) {
    if (const char *why = str_check(p)) return why;
    *k = StrCoef();
    k->fn = p.function, k->model = p.model, k->clipmode = p.clipmode, k->mask = p.mask;
    double *c = k->c;
    switch (p.function) {
        case SGPU_STRETCH_MTF:
            c[C_LO] = p.lo, c[C_M] = p.m, c[C_HI] = p.hi;
            c[C_RANGE] = p.hi - p.lo;
            c[C_M1] = p.m - 1.0;
            c[C_M2] = 2.0 * p.m - 1.0;
            return nullptr;
        case SGPU_STRETCH_LINEAR:
            c[C_BP] = p.BP;
            c[C_BPD] = 1.0 - p.BP;
            return nullptr;
        case SGPU_STRETCH_ASINH:
            c[C_BETA] = p.beta, c[C_OFF] = p.offset;
            c[C_OFFD] = 1.0 - p.offset;
            c[C_AB] = str_asinh(p.beta);
            return nullptr;
        default: break;
    }
    const bool modasinh = p.function == SGPU_STRETCH_MODASINH || p.function == SGPU_STRETCH_INVMODASINH;
    const double B = modasinh ? 0.0 : p.B, b = B < 0.0 ? -B : B;
    const double D = str_exp(p.D) - 1.0;
    c[G_D] = D, c[G_B] = B, c[G_AB] = b, c[G_LP] = p.LP, c[G_SP] = p.SP, c[G_HP] = p.HP;
    if (p.D == 0.0) {
        k->regime = Q_IDENTITY;
        return nullptr;
    }
    c[G_BD] = b * D;
    if (modasinh) {
        k->regime = Q_ASINH;
    } else if (B == -1.0) {
        k->regime = Q_LOG;
    } else if (B < 0.0) {
        k->regime = Q_NEG;
        c[G_P1] = (b - 1.0) / b;
        c[G_P2] = b / (b - 1.0);
    } else if (B == 0.0) {
        k->regime = Q_EXP;
    } else {
        k->regime = Q_POS;
        c[G_P1] = -1.0 / B;
        c[G_P2] = -B;
    }
    const double ul = p.SP - p.LP, uh = p.HP - p.SP;
    c[G_A1] = str_q(c, k->regime, ul);
    c[G_S1] = str_dq(c, k->regime, ul);
    c[G_A2] = str_q(c, k->regime, uh);
    c[G_S2] = str_dq(c, k->regime, uh);
    c[G_S0] = str_S(c, k->regime, 0.0);
    c[G_SPAN] = str_S(c, k->regime, 1.0) - c[G_S0];
    c[G_INV] = 1.0 / c[G_SPAN];
    return nullptr;
}

// ---- T8: one sample and one pixel ----
// three planes of an image go through str_pixel3 together
SGPU_STR_HD inline bool str_joint(const StrCoef &k, int nch) {
    return nch == 3 && (k.fn == SGPU_STRETCH_ASINH || (k.fn >= SGPU_STRETCH_GHT && k.model != SGPU_STRETCH_INDEPENDENT));
}
// x is the widened sample; the result is rounded to float by the caller
SGPU_STR_HD inline double str_sample(const StrCoef &k, double x) {
    x = str_clip01(x);
    switch (k.fn) {
        case SGPU_STRETCH_MTF: return str_mtf(k.c, x);
        case SGPU_STRETCH_LINEAR: return str_lin(k.c, x);
        case SGPU_STRETCH_ASINH: {
            const double v = str_asinh_pre(k.c, x);
            return str_min1(v * str_asinh_k(k.c, v));
        }
        default: return str_transfer(k, x);
    }
}
SGPU_STR_HD inline double str_lum(const StrCoef &k, const double *x) {
    if (k.model == SGPU_STRETCH_HUMAN) return (STR_HUMAN_R * x[0] + STR_HUMAN_G * x[1]) + STR_HUMAN_B * x[2];
    return (STR_THIRD * x[0] + STR_THIRD * x[1]) + STR_THIRD * x[2];
}
// x[3] are the widened samples of one pixel; o[3] the results before the rounding to float
SGPU_STR_HD inline void str_pixel3(const StrCoef &k, const double *xw, double *o) {
    double x[3];
    if (k.fn == SGPU_STRETCH_ASINH) {
        for (int c = 0; c < 3; c++) x[c] = str_asinh_pre(k.c, str_clip01(xw[c]));
        const double kk = str_asinh_k(k.c, str_lum(k, x));
        for (int c = 0; c < 3; c++) o[c] = str_min1(x[c] * kk);
        return;
    }
    for (int c = 0; c < 3; c++) x[c] = str_clip01(xw[c]);
    const double L = str_lum(k, x);
    const double tl = str_transfer(k, L);
    const double q = tl / L;
    const double kk = L == 0.0 ? 0.0 : q;
    double s[3];
    for (int c = 0; c < 3; c++) s[c] = x[c] * kk;
    if (k.clipmode == SGPU_STRETCH_CLIP) {
        for (int c = 0; c < 3; c++) o[c] = str_min1(s[c]);
    } else if (k.clipmode == SGPU_STRETCH_RESCALE) {
        double mx = s[0];
        mx = s[1] > mx ? s[1] : mx;
        mx = s[2] > mx ? s[2] : mx;
        for (int c = 0; c < 3; c++) {
            const double r = s[c] / mx;
            o[c] = mx > 1.0 ? r : s[c];
        }
    } else {
        for (int c = 0; c < 3; c++) o[c] = s[c];
        if (s[0] > 1.0 || s[1] > 1.0 || s[2] > 1.0) {       // the per-channel transfer only where a channel clips
            double t[3], kb = 1.0;
            for (int c = 0; c < 3; c++) {
                t[c] = str_transfer(k, x[c]);
                const double r = (1.0 - t[c]) / (s[c] - t[c]);
                kb = (s[c] > 1.0 && r < kb) ? r : kb;
            }
            const double kt = 1.0 - kb;
            for (int c = 0; c < 3; c++) o[c] = str_min1(kb * s[c] + kt * t[c]);
        }
    }
}

// host restatement of a whole call's planes with one coefficient block (the stand-alone program)
template <typename T>
inline void str_planes_host(const StrCoef &k, const T *in, int nimages, int nch, size_t npix, float *out) {
    const bool masked = nch == 3;
    if (str_joint(k, nch)) {
        for (int i = 0; i < nimages; i++)
            for (size_t j = 0; j < npix; j++) {
                double x[3], o[3];
                for (int c = 0; c < 3; c++) x[c] = str_widen(in[((size_t)i * 3 + c) * npix + j]);
                str_pixel3(k, x, o);
                for (int c = 0; c < 3; c++)
                    out[((size_t)i * 3 + c) * npix + j] = (k.mask >> c & 1) ? (float)o[c] : (float)x[c];
            }
        return;
    }
    for (size_t p = 0; p < (size_t)nimages * nch; p++) {
        const bool sel = !masked || (k.mask >> (int)(p % 3) & 1);
        for (size_t j = 0; j < npix; j++) {
            const double x = str_widen(in[p * npix + j]);
            out[p * npix + j] = sel ? (float)str_sample(k, x) : (float)x;
        }
    }
}

}  // namespace sgpu_str_host

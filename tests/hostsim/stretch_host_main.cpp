// stretch_host_main.cpp -- stand-alone driver of the stretches' shared code
// (siril_amd/csrc/stretch_host.h: refusals, conversion, exp / pow / asinh, the
// midtones transfer function, the autostretch parameters, the generalised
// hyperbolic stretch with its coefficient block and inverse, the colour
// models), for a sanitizer build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       stretch_host_main.cpp -o stretch_host_main
// Prints, per case, the parameters, the coefficient block and every output
// sample in hex (tests/test_stretch_host.py compares them with
// tests/stretch_ref.py bit for bit), then the autostretch cases, and checks the
// refusals and a few identities itself.
// Exit status 0 and "stretch host ok" when every check of its own holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../siril_amd/csrc/stretch_host.h"

using namespace sgpu_str_host;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);  \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static uint32_t fbits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}
static unsigned long long dbits(double v) { return (unsigned long long)rbf_bits(v); }

// the scene of tests/test_stretch_host.py: plane p of w x h
static int scene_v(int p, int x, int y) { return (x * 37 + y * 101 + 13 * p + (x * y) % 29 * 31) % 997; }
static void scene_word(int np, int w, int h, std::vector<uint16_t> &s) {
    s.assign((size_t)np * w * h, 0);
    for (int p = 0; p < np; p++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) s[((size_t)p * h + y) * w + x] = (uint16_t)(scene_v(p, x, y) * 65);
    for (int p = 0; p < np; p++) {
        s[(size_t)p * w * h] = 0;
        if (w * h > 1) s[(size_t)p * w * h + 1] = 65535;
        if (w * h > 5) s[(size_t)p * w * h + 5] = 0;
    }
}
static void scene_float(int np, int w, int h, std::vector<float> &s) {
    s.assign((size_t)np * w * h, 0.0f);
    const float k = (float)(1.0 / 900.0);
    for (int p = 0; p < np; p++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) s[((size_t)p * h + y) * w + x] = (float)scene_v(p, x, y) * k - 0.05f;
    for (int p = 0; p < np; p++) {
        s[(size_t)p * w * h] = 0.0f;
        if (w * h > 1) s[(size_t)p * w * h + 1] = 1.0f;
        if (w * h > 5) s[(size_t)p * w * h + 5] = 0.0f;
    }
    if (np > 1 && w * h > 3) s[(size_t)w * h + 3] = std::numeric_limits<float>::quiet_NaN();
}

static sgpu_stretch_params P(int fn) {
    sgpu_stretch_params p = {};
    p.function = fn, p.model = SGPU_STRETCH_INDEPENDENT, p.clipmode = SGPU_STRETCH_RGBBLEND, p.mask = 7;
    p.m = 0.5, p.hi = 1.0, p.HP = 1.0, p.beta = 1.0;
    return p;
}
static sgpu_stretch_params ght(int fn, double D, double B, double LP, double SP, double HP, int model = 0,
                               int clipmode = SGPU_STRETCH_RGBBLEND, int mask = 7) {
    sgpu_stretch_params p = P(fn);
    p.D = D, p.B = B, p.LP = LP, p.SP = SP, p.HP = HP, p.model = model, p.clipmode = clipmode, p.mask = mask;
    return p;
}

static void run_case(const sgpu_stretch_params &p, int nimages, int nch, int w, int h, int word) {
    StrCoef k;
    const char *why = str_coeffs(p, &k);
    CHECK(why == nullptr);
    if (why) return;
    std::printf("case %d %d %d %d %d %d %d %d %d", p.function, p.model, p.clipmode, p.mask, nimages, nch, w, h, word);
    for (double d : {p.lo, p.m, p.hi, p.D, p.B, p.LP, p.SP, p.HP, p.beta, p.offset, p.BP}) std::printf(" %016llx", dbits(d));
    std::printf("\ncoef %d", k.regime);
    for (double d : k.c) std::printf(" %016llx", dbits(d));
    const size_t npix = (size_t)w * h, n = (size_t)nimages * nch * npix;
    std::vector<float> out(n);
    if (word) {
        std::vector<uint16_t> s;
        scene_word(nimages * nch, w, h, s);
        str_planes_host(k, s.data(), nimages, nch, npix, out.data());
    } else {
        std::vector<float> s;
        scene_float(nimages * nch, w, h, s);
        str_planes_host(k, s.data(), nimages, nch, npix, out.data());
    }
    std::printf("\nout");
    for (float v : out) std::printf(" %08x", fbits(v));
    std::printf("\n");
    for (float v : out) CHECK(v != v || (v >= 0.0f && v <= 1.0f) || p.mask != 7);
}

static void run_auto(const std::vector<double> &stats, int nimages, int nch, double unit, int linked, double clip,
                     double target) {
    const size_t np = (size_t)nimages * nch;
    std::vector<int> status(np, 0);
    std::vector<double> out(3 * np);
    const char *why = str_autostretch(stats.data(), status.data(), nimages, nch, unit, linked, clip, target, out.data());
    CHECK(why == nullptr);
    std::printf("auto %d %d %d %016llx %016llx %016llx", nimages, nch, linked, dbits(unit), dbits(clip), dbits(target));
    for (double d : stats) std::printf(" %016llx", dbits(d));
    std::printf("\nparams");
    for (double d : out) std::printf(" %016llx", dbits(d));
    std::printf("\n");
}

int main() {
    // refusals
    {
        sgpu_stretch_params p = P(SGPU_STRETCH_MTF);
        CHECK(str_check(p) == nullptr);
        p.hi = 0.0;
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_MTF), p.m = 0.0;
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_MTF), p.m = std::nan("");
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_MTF), p.lo = -0.1;
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_LINEAR), p.BP = 1.0;
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_ASINH), p.beta = 0.5;
        CHECK(str_check(p) != nullptr);
        p = P(SGPU_STRETCH_ASINH), p.offset = 1.0;
        CHECK(str_check(p) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 10.5, 0, 0, 0, 1)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, -5.5, 0, 0, 1)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 15.5, 0, 0, 1)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_MODASINH, 1, 99, 0, 0, 1)) == nullptr);     // modasinh has no B
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 0, 0.5, 0.4, 1)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 0, 0, 0.4, 0.3)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 0, 0, 0, 1, 3)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 0, 0, 0, 1, 0, 3)) != nullptr);
        CHECK(str_check(ght(SGPU_STRETCH_GHT, 1, 0, 0, 0, 1, 0, 0, 0)) != nullptr);
        p = P(7);
        CHECK(str_check(p) != nullptr);
    }
    // exp is total, log and exp keep a NaN, T(0) = 0 and T(1) = 1
    CHECK(str_exp(-22026.0) > 0.0 && str_exp(-22026.0) < 1e-300);
    CHECK(str_exp(1e9) < 1e308);
    CHECK(str_exp(0.0) == 1.0 && str_log(1.0) == 0.0);
    CHECK(str_exp(std::nan("")) != str_exp(std::nan("")) && str_log(std::nan("")) != str_log(std::nan("")));
    CHECK(std::fabs(str_exp(1.0) - 2.718281828459045) < 1e-15);
    CHECK(str_mtf01(0.3, 0.3) == 0.5);
    for (double B : {-5.0, -1.5, -1.0, -0.5, 0.0, 0.5, 3.0, 15.0})
        for (double D : {0.1, 10.0}) {
            StrCoef k;
            CHECK(str_coeffs(ght(SGPU_STRETCH_GHT, D, B, 0.02, 0.1, 0.8), &k) == nullptr);
            CHECK(str_T(k.c, k.regime, 0.0) == 0.0);
            CHECK(std::fabs(str_T(k.c, k.regime, 1.0) - 1.0) <= 1e-14);
        }

    // every B regime, forward and inverse, at a small and at the largest D; float and WORD; mono and three planes
    for (double B : {-5.0, -1.5, -1.0, -0.5, 0.0, 0.5, 3.0, 15.0}) {
        run_case(ght(SGPU_STRETCH_GHT, 1.0, B, 0.02, 0.1, 0.8), 2, 1, 7, 5, 0);
        run_case(ght(SGPU_STRETCH_GHT, 10.0, B, 0.0, 0.0, 1.0), 1, 3, 7, 5, 1);
        run_case(ght(SGPU_STRETCH_INVGHT, 3.0, B, 0.1, 0.5, 0.9), 1, 3, 7, 5, 0);
    }
    run_case(ght(SGPU_STRETCH_INVGHT, 10.0, 0.0, 0.0, 0.0, 1.0), 1, 1, 7, 5, 0);
    run_case(ght(SGPU_STRETCH_GHT, 0.0, 3.0, 0.0, 0.2, 1.0), 1, 1, 7, 5, 0);                     // D = 0: the identity
    run_case(ght(SGPU_STRETCH_GHT, 4.0, 2.0, 0.5, 0.5, 0.5), 1, 1, 7, 5, 1);
    run_case(ght(SGPU_STRETCH_MODASINH, 5.0, 0.0, 0.02, 0.1, 0.8), 1, 1, 7, 5, 0);
    run_case(ght(SGPU_STRETCH_MODASINH, 5.0, 0.0, 0.02, 0.1, 0.8), 1, 3, 7, 5, 1);
    run_case(ght(SGPU_STRETCH_INVMODASINH, 5.0, 0.0, 0.02, 0.1, 0.8), 2, 1, 7, 5, 0);
    // every colour model and clip mode, and a channel mask
    for (int model : {SGPU_STRETCH_HUMAN, SGPU_STRETCH_EVEN})
        for (int mode : {SGPU_STRETCH_CLIP, SGPU_STRETCH_RESCALE, SGPU_STRETCH_RGBBLEND}) {
            run_case(ght(SGPU_STRETCH_GHT, 6.0, 3.0, 0.0, 0.05, 1.0, model, mode), 2, 3, 7, 5, 0);
            run_case(ght(SGPU_STRETCH_MODASINH, 6.0, 0.0, 0.0, 0.05, 1.0, model, mode), 1, 3, 7, 5, 1);
        }
    run_case(ght(SGPU_STRETCH_INVGHT, 2.0, -1.5, 0.0, 0.05, 1.0, SGPU_STRETCH_HUMAN, SGPU_STRETCH_RGBBLEND), 1, 3, 7, 5, 0);
    run_case(ght(SGPU_STRETCH_GHT, 6.0, 3.0, 0.0, 0.05, 1.0, SGPU_STRETCH_HUMAN, SGPU_STRETCH_RGBBLEND, 5), 1, 3, 7, 5, 0);
    run_case(ght(SGPU_STRETCH_GHT, 6.0, 3.0, 0.0, 0.05, 1.0, SGPU_STRETCH_INDEPENDENT, SGPU_STRETCH_RGBBLEND, 2), 1, 3, 7, 5, 1);
    // asinh mono and colour, mtf, linstretch
    {
        sgpu_stretch_params p = P(SGPU_STRETCH_ASINH);
        p.beta = 100.0, p.offset = 0.03;
        run_case(p, 1, 1, 7, 5, 0);
        run_case(p, 1, 1, 7, 5, 1);
        run_case(p, 1, 3, 7, 5, 0);
        p.model = SGPU_STRETCH_HUMAN, p.beta = 1000.0;
        run_case(p, 2, 3, 7, 5, 1);
        p = P(SGPU_STRETCH_MTF);
        p.lo = 0.05, p.m = 0.2, p.hi = 0.9;
        run_case(p, 1, 1, 7, 5, 0);
        p.mask = 6;
        run_case(p, 1, 3, 7, 5, 1);
        p = P(SGPU_STRETCH_LINEAR);
        p.BP = 0.1;
        run_case(p, 1, 3, 7, 5, 0);
        run_case(p, 1, 1, 3, 1, 1);
    }
    // autostretch: unlinked and linked, a plane above 0.5 (inverted), WORD units
    run_auto({0.1, 0.01, 0, 0, 0.12, 0.02, 0, 0, 0.7, 0.03, 0, 0}, 1, 3, 1.0, 0, -2.8, 0.25);
    run_auto({0.1, 0.01, 0, 0, 0.12, 0.02, 0, 0, 0.7, 0.03, 0, 0}, 1, 3, 1.0, 1, -2.8, 0.25);
    run_auto({0.8, 0.01, 0, 0, 0.9, 0.02, 0, 0, 0.2, 0.03, 0, 0}, 1, 3, 1.0, 1, -1.5, 0.3);
    run_auto({6000.0, 400.0, 0, 0, 50000.0, 900.0, 0, 0}, 2, 1, 65535.0, 0, -2.8, 0.25);
    {
        const double st[4] = {0.1, 0.01, 0, 0};
        int bad = 1, good = 0;
        double o[3];
        CHECK(str_autostretch(st, &bad, 1, 1, 1.0, 0, -2.8, 0.25, o) != nullptr);
        CHECK(str_autostretch(st, &good, 1, 1, 1.0, 0, 2.8, 0.25, o) != nullptr);
        CHECK(str_autostretch(st, &good, 1, 1, 1.0, 0, -2.8, 1.0, o) != nullptr);
        const double flat[4] = {0.1, 0.0, 0, 0};
        CHECK(str_autostretch(flat, &good, 1, 1, 1.0, 0, -2.8, 0.25, o) != nullptr);
        CHECK(str_autostretch(st, &good, 1, 1, 1.0, 0, -2.8, 0.25, o) == nullptr);
    }
    if (failures) return 1;
    std::printf("stretch host ok\n");
    return 0;
}

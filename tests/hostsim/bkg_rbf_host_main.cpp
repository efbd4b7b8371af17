// bkg_rbf_host_main.cpp -- stand-alone driver of the thin-plate-spline
// background's host side (siril_amd/csrc/bkg_rbf_host.h: the refusals, the
// one-scale coordinates, the logarithm, the radial kernel, the system, the LU,
// the mean, the background; bkg_host.h's medians, selection and correction),
// for a sanitizer build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       bkg_rbf_host_main.cpp -o bkg_rbf_host_main
// Prints the logarithm of a fixed set of arguments, the solutions of a few
// hand-made systems and, per case, the first row of Phi, the mean of |Phi|,
// lambda, the weights, the mean and a few background and output values, all
// in hex (tests/test_bkg_rbf_host.py compares them with tests/bkg_rbf_ref.py).
// Exit status 0 and "bkg rbf host ok" when every check of its own holds.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/bkg_rbf_host.h"

using namespace sgpu_bkg_host;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);  \
            failures++;                                                   \
        }                                                                 \
    } while (0)

// the scene of tests/test_bkg_rbf_host.py: a gradient, a texture and raised 13 x 13 cells, in ADU
static int scene(int c, int x, int y) {
    const int raised = ((x / 13 + 2 * (y / 13) + c) % 7 == 0) ? 13000 : 0;
    return 3000 + 7 * x * (c + 1) + 5 * y + ((x * 37 + y * 101 + 13 * c) % 97) * 3 + raised;
}

static void print_solve(const char *name, int N, std::vector<double> aug) {
    std::vector<double> x((size_t)N);
    const int st = rbf_lu_solve_host(N, aug.data(), x.data());
    std::printf("solve %s %d", name, st);
    for (int i = 0; i < N; i++) std::printf(" %016" PRIx64, rbf_bits(x[(size_t)i]));
    std::printf("\n");
}

template <typename T>
static void run_case(int c, int W, int H, int S, double tol, double smooth, const std::vector<T> &plane) {
    BkgGrid g;
    CHECK(rbf_check(W, H, S, tol, smooth, &g) == nullptr);
    std::vector<float> med((size_t)g.K);
    for (int k = 0; k < g.K; k++) med[(size_t)k] = bkg_box_median_host(plane.data(), W, g, k);
    std::vector<uint8_t> keep((size_t)g.K);
    const int kept = bkg_select_host(med.data(), g.K, tol, keep.data());
    const double lam_rel = rbf_lam_rel(smooth);
    const RbfFit f = rbf_fit_host(med.data(), keep.data(), g, W, H, lam_rel);
    CHECK(f.n == kept);
    std::printf("case %d %d %d %d %.17g %d %016" PRIx64 "\n", c, W, H, S, tol, (int)(sizeof(T) == 2), rbf_bits(lam_rel));
    std::printf("fit %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", f.n, f.status, rbf_bits(f.mean_abs),
                rbf_bits(f.lambda), rbf_bits(f.mean));
    std::printf("phi");
    for (int j = 0; j < f.n; j++)
        std::printf(" %016" PRIx64, rbf_bits(rbf_phi(f.u[0] - f.u[(size_t)j], f.v[0] - f.v[(size_t)j])));
    std::printf("\nx");
    for (int i = 0; i <= f.n; i++) std::printf(" %016" PRIx64, rbf_bits(f.x[(size_t)i]));
    const RbfAxes ax = rbf_axes(W, H);
    // the first kept box's centre is a pixel: s == 0 there
    int k0 = 0;
    while (!keep[(size_t)k0]) k0++;
    const int px[6] = {0, W - 1, W / 2, 3, W - 1, bkg_cx(g, k0 % g.nx)};
    const int py[6] = {0, 0, H / 2, H - 1, H - 1, bkg_cy(g, k0 / g.nx)};
    CHECK(rbf_u(px[5], ax) - f.u[0] == 0.0 && rbf_v(py[5], ax) - f.v[0] == 0.0);
    std::printf("\nbkg");
    for (int k = 0; k < 6; k++) {
        const double b = rbf_background_host(f, px[k], py[k], ax);
        const float x = bkg_to_float(plane[(size_t)py[k] * W + px[k]]);
        std::printf(" %016" PRIx64 " %08x %08x", rbf_bits(b), bkg_float_bits(bkg_correct(x, b, f.mean, 0)),
                    bkg_float_bits(bkg_correct(x, b, f.mean, 1)));
    }
    std::printf("\n");
}

int main() {
    // R0: the cap and the parameters
    BkgGrid g;
    CHECK(rbf_check(57, 55, 57, 1e9, 0.5, &g) == nullptr && g.K == 1023);
    CHECK(rbf_check(57, 56, 57, 1e9, 0.5, &g) != nullptr);         // K = 1056
    CHECK(rbf_check(6000, 4000, 38, 1.0, 0.5, &g) == nullptr && g.K <= RBF_MAX_SAMPLES);
    CHECK(rbf_check(40, 30, 1, 1.0, 0.0, &g) == nullptr && g.K == 1);
    CHECK(rbf_check(40, 30, 1, 1.0, 1.0, &g) == nullptr);
    CHECK(rbf_check(40, 30, 1, 1.0, -0.1, &g) != nullptr);
    CHECK(rbf_check(40, 30, 1, 1.0, 1.5, &g) != nullptr);
    CHECK(rbf_check(40, 30, 1, 1.0, NAN, &g) != nullptr);
    CHECK(rbf_check(40, 30, 1, -1.0, 0.5, &g) != nullptr);
    CHECK(rbf_check(40, 30, 1, INFINITY, 0.5, &g) != nullptr);
    CHECK(rbf_check(24, 30, 1, 1.0, 0.5, &g) != nullptr);
    // R1: one scale, the longer axis ends at -1 and 1
    const RbfAxes ax = rbf_axes(131, 77);
    CHECK(rbf_u(0, ax) == -1.0 && rbf_u(130, ax) == 1.0 && rbf_u(65, ax) == 0.0 && rbf_v(38, ax) == 0.0);
    CHECK(rbf_v(0, ax) == -38.0 * ax.a);
    // R2: the kernel at 0 is +0, and the logarithm of 1 is 0
    CHECK(rbf_bits(rbf_phi(0.0)) == 0 && rbf_log(1.0) == 0.0 && rbf_phi(1.0) == 0.0);
    CHECK(fabs(rbf_log(8.0) - log(8.0)) <= 7e-16 * log(8.0));
    CHECK(fabs(rbf_log(1e-8) - log(1e-8)) <= 7e-16 * -log(1e-8));
    std::printf("log");
    for (int k = 0; k < 256; k++)
        std::printf(" %016" PRIx64, rbf_bits(rbf_log((double)(k + 1) * (double)(k + 1) * 1.220703125e-4)));
    const double extra[8] = {1.0, 1.4142135623730951, 1.4142135623730954, 0.5, 2.0, 8.0, 1e-8, 0.70710678118654757};
    for (double s : extra) std::printf(" %016" PRIx64, rbf_bits(rbf_log(s)));
    std::printf("\n");
    // R4 on hand-made systems: order 1 and 2, equal maxima in a pivot column, a singular one, one with a NaN
    print_solve("order1", 1, {2.0, 3.0});
    print_solve("order2", 2, {0.1, 0.2, 0.3, 0.3, 0.4, 0.5});
    print_solve("tie", 3, {0.3, 0.7, 0.1, 0.1, -0.9, 0.2, 0.5, 0.2, 0.9, 0.4, 0.6, 0.3});
    print_solve("singular", 2, {1.0, 2.0, 1.0, 2.0, 4.0, 2.0});
    print_solve("nan", 2, {1.0, NAN, 1.0, 2.0, 3.0, 1.0});
    CHECK(rbf_pivot_bad(0.0) && rbf_pivot_bad(-0.0) && rbf_pivot_bad(NAN) && rbf_pivot_bad(-INFINITY) && !rbf_pivot_bad(-1e-300));
    CHECK(rbf_pivot_key(-4.0) == rbf_pivot_key(4.0) && rbf_pivot_key(NAN) > rbf_pivot_key(INFINITY));
    // no box kept: status 1, everything +0
    {
        const int W = 60, H = 50;
        CHECK(rbf_check(W, H, 4, 1.0, 0.5, &g) == nullptr);
        std::vector<float> med((size_t)g.K, 0.0f);
        std::vector<uint8_t> keep((size_t)g.K, 0);
        const RbfFit f = rbf_fit_host(med.data(), keep.data(), g, W, H, rbf_lam_rel(0.5));
        CHECK(f.status == 1 && f.n == 0 && f.x.size() == 1 && f.x[0] == 0.0 && f.mean == 0.0);
    }
    // one box: weight +0, the constant is the median
    {
        const int W = 40, H = 30;
        CHECK(rbf_check(W, H, 1, 1.0, 0.5, &g) == nullptr);
        const float med[1] = {0.25f};
        const uint8_t keep[1] = {1};
        const RbfFit f = rbf_fit_host(med, keep, g, W, H, rbf_lam_rel(0.5));
        CHECK(f.status == 0 && f.n == 1 && rbf_bits(f.x[0]) == 0 && f.x[1] == 0.25 && f.mean == 0.25);
    }
    // the cases
    const int cases[3][3] = {{131, 77, 10}, {131, 77, 10}, {200, 150, 20}};
    const double tols[3] = {1.0, 3.0, 1.0}, smooths[3] = {0.5, 0.0, 1.0};
    for (int c = 0; c < 3; c++) {
        const int W = cases[c][0], H = cases[c][1];
        if (c & 1) {
            std::vector<uint16_t> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (uint16_t)scene(c, x, y);
            run_case(c, W, H, cases[c][2], tols[c], smooths[c], pl);
        } else {
            std::vector<float> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (float)scene(c, x, y) * (1.0f / 65536.0f);
            run_case(c, W, H, cases[c][2], tols[c], smooths[c], pl);
        }
    }
    if (failures) return 1;
    std::printf("bkg rbf host ok\n");
    return 0;
}

// drizzle_host_main.cpp -- stand-alone driver of the drizzle's shared
// arithmetic (siril_amd/csrc/drizzle_host.h), for a sanitizer build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       drizzle_host_main.cpp -o drizzle_host_main
// Runs the sequential scatter and the gather (one output pixel after the
// other, candidate windows as the kernel takes them) on fixed cases, compares
// them bit for bit, checks the host-side refusals, and prints every case with
// its image and weight plane as hexadecimal float words for the test to compare
// with tests/drizzle_ref.py.  Exit status 0 and a last line "drizzle host ok"
// when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/drizzle_host.h"

using namespace sgpu_drizzle_host;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);  \
            failures++;                                                   \
        }                                                                 \
    } while (0)

struct Case {
    int W, H;
    double Hm[9];   // the frame's homography (top-down coordinates); the reference is the identity
    double scale, pixfrac;
    int kernel, word, pw;
};

static const double C15 = 0.99965732497555726, S15 = 0.026176948307873153;   // cos, sin of 1.5 degrees

static const Case CASES[] = {
    {13, 7, {1, 0, 0, 0, 1, 0, 0, 0, 1}, 2.0, 1.0, SGPU_DRIZZLE_SQUARE, 0, 0},
    {13, 7, {1, 0, 0.25, 0, 1, 0.25, 0, 0, 1}, 2.0, 0.5, SGPU_DRIZZLE_SQUARE, 1, 0},
    {13, 7, {C15, -S15, 0.8, S15, C15, -0.6, 0, 0, 1}, 1.5, 0.7, SGPU_DRIZZLE_SQUARE, 0, 1},
    {13, 7, {1.01, 0.02, -1.2, -0.015, 0.99, 0.8, 2e-4, -1e-4, 1}, 1.0, 1.0, SGPU_DRIZZLE_SQUARE, 1, 1},
    {13, 7, {-1, 0, 11.75, 0, 1, 0.5, 0, 0, 1}, 2.0, 0.7, SGPU_DRIZZLE_SQUARE, 0, 0},
    {13, 7, {C15, -S15, 0.8, S15, C15, -0.6, 0, 0, 1}, 0.5, 1.0, SGPU_DRIZZLE_SQUARE, 0, 0},
    {13, 7, {1, 0, 500, 0, 1, 300, 0, 0, 1}, 2.0, 1.0, SGPU_DRIZZLE_SQUARE, 0, 0},
    {13, 7, {C15, -S15, 0.8, S15, C15, -0.6, 0, 0, 1}, 2.0, 0.7, SGPU_DRIZZLE_TURBO, 0, 1},
    {13, 7, {0.45, 0, 1.3, 0, 0.45, 0.7, 0, 0, 1}, 2.0, 1.0, SGPU_DRIZZLE_TURBO, 1, 0},
    {13, 7, {-1, 0, 11.75, 0, 1, 0.5, 0, 0, 1}, 0.5, 0.5, SGPU_DRIZZLE_TURBO, 0, 0},
    {13, 7, {1.01, 0.02, -1.2, -0.015, 0.99, 0.8, 2e-4, -1e-4, 1}, 1.5, 1.0, SGPU_DRIZZLE_POINT, 0, 1},
    {17, 1, {1, 0, -1.4, 0, 1, 0.3, 0, 0, 1}, 2.0, 1.0, SGPU_DRIZZLE_SQUARE, 1, 0},
    {31, 9, {C15, -S15, 0.8, S15, C15, -0.6, 0, 0, 1}, 0.25, 1.0, SGPU_DRIZZLE_SQUARE, 0, 0},
};

static float sample(int c, int i, int j, int word) {
    const int base = (i * 37 + j * 101 + 13 * c) % 1000;
    return word ? (float)(base * 60 + 5) : (float)(base * 60 + 5) + 0.25f;
}
static float pixel_weight(int i, int j) { return (i + 2 * j) % 5 == 0 ? 0.f : 0.25f * (float)((i * 3 + j) % 8 + 1); }

static void print_plane(const char *tag, const std::vector<float> &v) {
    std::printf("%s", tag);
    for (float f : v) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        std::printf(" %08x", u);
    }
    std::printf("\n");
}

template <typename T>
static void run(int c, const Case &cs, const double *A, const double *M, const sgpu_drizzle_params &p, int ow, int oh) {
    std::vector<T> in((size_t)cs.W * cs.H);
    std::vector<float> pw((size_t)cs.W * cs.H);
    for (int j = 0; j < cs.H; j++)
        for (int i = 0; i < cs.W; i++) {
            in[(size_t)j * cs.W + i] = (T)sample(c, i, j, cs.word);
            pw[(size_t)j * cs.W + i] = pixel_weight(i, j);
        }
    const float *w = cs.pw ? pw.data() : nullptr;
    const size_t n = (size_t)ow * oh;
    std::vector<float> so(n), sw(n), go(n, -1.f), gw(n, -1.f);
    drz_scatter_frame(in.data(), w, cs.W, cs.H, A, &p, ow, oh, so.data(), sw.data());
    drz_gather_frame(in.data(), w, cs.W, cs.H, A, M, &p, ow, oh, go.data(), gw.data());
    CHECK(std::memcmp(so.data(), go.data(), n * sizeof(float)) == 0);
    CHECK(std::memcmp(sw.data(), gw.data(), n * sizeof(float)) == 0);
    print_plane("img", so);
    print_plane("wts", sw);
}

int main() {
    // ---- parameter and size refusals ----
    sgpu_drizzle_params p = {2.0, 1.0, SGPU_DRIZZLE_SQUARE, 0};
    CHECK(drz_check_params(&p) == nullptr);
    p.scale = 0.05;
    CHECK(drz_check_params(&p) != nullptr);
    p.scale = 4.5;
    CHECK(drz_check_params(&p) != nullptr);
    p.scale = NAN;
    CHECK(drz_check_params(&p) != nullptr);
    p.scale = 2.0;
    p.pixfrac = 0.0;
    CHECK(drz_check_params(&p) != nullptr);
    p.pixfrac = 1.25;
    CHECK(drz_check_params(&p) != nullptr);
    p.pixfrac = 1.0;
    p.kernel = 3;
    CHECK(drz_check_params(&p) != nullptr);
    p.kernel = SGPU_DRIZZLE_SQUARE;
    int ow = 0, oh = 0;
    CHECK(drz_output_size(45, 23, 1.5, &ow, &oh) == nullptr && ow == 68 && oh == 35);
    CHECK(drz_output_size(45, 23, 0.5, &ow, &oh) == nullptr && ow == 23 && oh == 12);
    CHECK(drz_output_size(4, 4, 0.1, &ow, &oh) != nullptr);   // 0.4 + 0.5 floors to 0
    CHECK(drz_output_size(0, 4, 1.0, &ow, &oh) != nullptr);

    // ---- maps: exact integer translation, singular H, W changing sign ----
    {
        const double H2[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 3, 0, 1, -2, 0, 0, 1};
        double A[18];
        CHECK(drz_forward_maps(2, H2, 0, 23, A) == nullptr);
        const double want[9] = {1, 0, 3, 0, 1, 2, 0, 0, 1};
        for (int k = 0; k < 9; k++) CHECK(A[9 + k] == want[k]);
        double Hs[18];
        std::memcpy(Hs, H2, sizeof Hs);
        Hs[9] = 0;
        Hs[12] = 0;   // first column zero
        CHECK(drz_forward_maps(2, Hs, 0, 23, A) != nullptr);
        CHECK(drz_forward_maps(2, Hs, 1, 23, A) != nullptr);
        CHECK(drz_forward_maps(2, H2, 2, 23, A) != nullptr);
        // W = 1 - 0.05 x vanishes at x = 20, inside a 45-wide frame
        const double Hw[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, -0.05, 0, 1};
        CHECK(drz_forward_maps(2, Hw, 0, 23, A) == nullptr);
        double M[9];
        CHECK(drz_frame_maps(A + 9, 45, 23, 90, 46, &p, M) != nullptr);
        CHECK(drz_frame_maps(A + 9, 10, 23, 20, 46, &p, M) == nullptr);   // the pole lies outside a 10-wide frame
        CHECK(drz_frame_maps(A, 45, 23, 90, 46, &p, M) == nullptr);
    }

    // ---- scatter == gather, printed for the comparison with the Python restatement ----
    const int ncases = (int)(sizeof CASES / sizeof CASES[0]);
    for (int c = 0; c < ncases; c++) {
        const Case &cs = CASES[c];
        sgpu_drizzle_params q = {cs.scale, cs.pixfrac, cs.kernel, 0};
        double H2[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, A[18], M[9];
        std::memcpy(H2 + 9, cs.Hm, sizeof cs.Hm);
        CHECK(drz_check_params(&q) == nullptr);
        CHECK(drz_output_size(cs.W, cs.H, cs.scale, &ow, &oh) == nullptr);
        CHECK(drz_forward_maps(2, H2, 0, cs.H, A) == nullptr);
        CHECK(drz_frame_maps(A + 9, cs.W, cs.H, ow, oh, &q, M) == nullptr);
        if (failures) break;
        std::printf("case %d %d %d %.17g %.17g %d %d %d\nH", c, cs.W, cs.H, cs.scale, cs.pixfrac, cs.kernel, cs.word,
                    cs.pw);
        for (int k = 0; k < 9; k++) std::printf(" %.17g", cs.Hm[k]);
        std::printf("\nsize %d %d\n", ow, oh);
        if (cs.word) run<uint16_t>(c, cs, A + 9, M, q, ow, oh);
        else run<float>(c, cs, A + 9, M, q, ow, oh);
    }
    if (failures) return 1;
    std::printf("drizzle host ok\n");
    return 0;
}

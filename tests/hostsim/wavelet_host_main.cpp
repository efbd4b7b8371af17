// wavelet_host_main.cpp -- stand-alone driver of the a trous wavelet
// arithmetic (siril_amd/csrc/wavelet_host.h: refusals, conversion, reflection,
// the separable smoothing, details, weighted reconstruction), for a sanitizer
// build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       wavelet_host_main.cpp -o wavelet_host_main
// Prints, per case, every sample of the n planes and of the reconstruction in
// hex (tests/test_wavelet_host.py compares them with tests/wavelet_ref.py).
// Exit status 0 and "wavelet host ok" when every check of its own holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/wavelet_host.h"

using namespace sgpu_wav_host;

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

// the scene of tests/test_wavelet_host.py, an integer below 997
static int scene(int c, int x, int y) { return (x * 37 + y * 101 + 13 * c + (x * y) % 29 * 31) % 997; }

template <typename T>
static void run_case(int c, int W, int H, int n, int type, const std::vector<T> &plane) {
    const size_t np = (size_t)W * H;
    CHECK(wav_check(W, H, n, type) == nullptr);
    std::vector<float> planes((size_t)n * np), out(np);
    wav_transform_host(plane.data(), W, H, n, type, planes.data());
    const float coef[WAV_MAX_LAYERS] = {3.0f, 2.0f, 1.5f, 1.0f, -0.5f, 1.25f};
    wav_reconstruct_host(planes.data(), np, n, coef, out.data());
    std::printf("case %d %d %d %d %d %d\nplanes", c, W, H, n, type, (int)(sizeof(T) == 2));
    for (float v : planes) std::printf(" %08x", fbits(v));
    std::printf("\nrecon");
    for (float v : out) std::printf(" %08x", fbits(v));
    std::printf("\n");
}

int main() {
    // W1: reach, refusals and their exact boundary
    CHECK(wav_reach(1, 2) == 0 && wav_reach(2, 2) == 2 && wav_reach(6, 2) == 32 && wav_reach(2, 1) == 1 &&
          wav_reach(6, 1) == 16);
    CHECK(wav_check(33, 33, 6, 2) == nullptr);
    CHECK(wav_check(32, 40, 6, 2) != nullptr && wav_check(40, 32, 6, 2) != nullptr);
    CHECK(wav_check(32, 40, 6, 1) == nullptr && wav_check(17, 17, 6, 1) == nullptr && wav_check(16, 17, 6, 1) != nullptr);
    CHECK(wav_check(17, 17, 5, 2) == nullptr && wav_check(17, 17, 6, 2) != nullptr);
    CHECK(wav_check(1, 1, 1, 2) == nullptr && wav_check(1, 1, 2, 1) != nullptr && wav_check(2, 2, 2, 1) == nullptr);
    CHECK(wav_check(100, 100, 0, 2) != nullptr && wav_check(100, 100, 7, 2) != nullptr);
    CHECK(wav_check(100, 100, 3, 0) != nullptr && wav_check(100, 100, 3, 3) != nullptr);
    CHECK(wav_check(0, 100, 1, 2) != nullptr);
    CHECK(wav_refl(-3, 10) == 3 && wav_refl(0, 10) == 0 && wav_refl(9, 10) == 9 && wav_refl(10, 10) == 8 &&
          wav_refl(12, 10) == 6);
    CHECK(wav_finite(0.0f) && wav_finite(-3.5f) && !wav_finite(INFINITY) && !wav_finite(-INFINITY) && !wav_finite(NAN));
    CHECK(fbits(wav_to_float((uint16_t)65535)) == fbits(65535.0f * (1.0f / 65535.0f)));
    // a constant plane: details exactly 0, residual exactly the constant
    for (int type = 1; type <= 2; type++) {
        const int W = 33, H = 35, n = 6;
        std::vector<float> pl((size_t)W * H, 0.25f), planes((size_t)n * W * H);
        wav_transform_host(pl.data(), W, H, n, type, planes.data());
        for (size_t i = 0; i < planes.size(); i++)
            CHECK(fbits(planes[i]) == fbits(i < (size_t)(n - 1) * W * H ? 0.0f : 0.25f));
    }
    // the cases
    const int cases[5][4] = {{33, 33, 6, 2}, {40, 37, 6, 1}, {71, 53, 4, 2}, {17, 17, 6, 1}, {9, 5, 1, 2}};
    for (int c = 0; c < 5; c++) {
        const int W = cases[c][0], H = cases[c][1];
        if (c & 1) {
            std::vector<uint16_t> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (uint16_t)(scene(c, x, y) * 61);
            run_case(c, W, H, cases[c][2], cases[c][3], pl);
        } else {
            std::vector<float> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (float)scene(c, x, y) * (1.0f / 1024.0f);
            run_case(c, W, H, cases[c][2], cases[c][3], pl);
        }
    }
    if (failures) return 1;
    std::printf("wavelet host ok\n");
    return 0;
}

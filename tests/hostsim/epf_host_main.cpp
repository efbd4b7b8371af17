// epf_host_main.cpp -- stand-alone driver of the guided filter's shared code
// (siril_amd/csrc/epf_host.h: refusals, the window rule, the coefficients, the
// host reference of whole planes), for a sanitizer build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       epf_host_main.cpp -o epf_host_main
// Prints, per case, every output sample in hex (tests/test_epf_host.py compares
// them with tests/epf_ref.py bit for bit).  Exit status 0 and "epf host ok"
// when every check of its own holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/epf_host.h"

using namespace sgpu_epf_host;

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
static unsigned long long dbits(double v) {
    unsigned long long b;
    std::memcpy(&b, &v, 8);
    return b;
}

// the scene of tests/test_epf_host.py, an integer below 997
static int scene(int c, int x, int y) { return (x * 37 + y * 101 + 13 * c + (x * y) % 29 * 31) % 997; }

template <typename T>
static std::vector<T> plane(int c, int W, int H) {
    std::vector<T> pl((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            if (sizeof(T) == 2)
                pl[(size_t)y * W + x] = (T)(scene(c, x, y) * 61);
            else
                pl[(size_t)y * W + x] = (T)((float)scene(c, x, y) * (1.0f / 1024.0f));
        }
    return pl;
}

struct Case {
    int W, H, d;
    double si, ss;
    float mod;
    int word, guide;        // guide: -1 none, 0 float, 1 WORD
};

template <typename T, typename G>
static void run_case(int c, const Case &k) {
    CHECK(epf_check(k.W, k.H, 1, k.d, k.si, k.ss, k.mod) == nullptr);
    const std::vector<T> in = plane<T>(c, k.W, k.H);
    const std::vector<G> gd = plane<G>(c + 7, k.W, k.H);
    std::vector<float> out((size_t)k.W * k.H);
    epf_filter_host<T, G>(in.data(), k.guide >= 0 ? gd.data() : nullptr, k.W, k.H, k.d, k.si, k.ss, k.mod,
                          out.data());
    std::printf("case %d %d %d %d %016llx %016llx %08x %d %d\nout", c, k.W, k.H, k.d, dbits(k.si),
                dbits(k.ss), fbits(k.mod), k.word, k.guide);
    for (float v : out) std::printf(" %08x", fbits(v));
    std::printf("\n");
}

int main() {
    const float one = 1.0f;
    // E6 at its exact boundaries
    CHECK(epf_check(13, 13, 1, 25, 0.1, 3.0, one) == nullptr);
    CHECK(epf_check(12, 13, 1, 25, 0.1, 3.0, one) != nullptr && epf_check(13, 12, 1, 25, 0.1, 3.0, one) != nullptr);
    CHECK(epf_check(2, 2, 1, 3, 0.1, 3.0, one) == nullptr && epf_check(1, 5, 1, 3, 0.1, 3.0, one) != nullptr);
    CHECK(epf_check(50, 50, 1, 1, 0.1, 3.0, one) != nullptr && epf_check(50, 50, 1, 4, 0.1, 3.0, one) != nullptr &&
          epf_check(50, 50, 1, 27, 0.1, 3.0, one) != nullptr && epf_check(50, 50, 1, -3, 0.1, 3.0, one) != nullptr &&
          epf_check(50, 50, 1, 0, 0.1, 3.0, one) == nullptr);
    // the bilateral filter is not built
    CHECK(epf_check(50, 50, 2, 3, 0.1, 3.0, one) != nullptr && epf_check(50, 50, -1, 3, 0.1, 3.0, one) != nullptr &&
          epf_check(50, 50, 0, 3, 0.1, 3.0, one) != nullptr && epf_check(50, 50, 1, 3, 0.1, 3.0, one) == nullptr);
    CHECK(epf_check(50, 50, 1, 3, 0.0, 3.0, one) != nullptr && epf_check(50, 50, 1, 3, NAN, 3.0, one) != nullptr &&
          epf_check(50, 50, 1, 3, INFINITY, 3.0, one) != nullptr && epf_check(50, 50, 1, 3, 5e-324, 3.0, one) == nullptr);
    CHECK(epf_check(50, 50, 1, 0, 0.1, 0.0, one) != nullptr && epf_check(50, 50, 1, 0, 0.1, NAN, one) != nullptr &&
          epf_check(50, 50, 1, 3, 0.1, 0.0, one) == nullptr);
    CHECK(epf_check(50, 50, 1, 3, 0.1, 3.0, -0.001f) != nullptr && epf_check(50, 50, 1, 3, 0.1, 3.0, 1.001f) != nullptr &&
          epf_check(50, 50, 1, 3, 0.1, 3.0, NAN) != nullptr && epf_check(50, 50, 1, 3, 0.1, 3.0, 0.0f) == nullptr);
    CHECK(epf_check(65535, 20, 1, 3, 0.1, 3.0, one) == nullptr && epf_check(65536, 20, 1, 3, 0.1, 3.0, one) != nullptr &&
          epf_check(20, 65536, 1, 3, 0.1, 3.0, one) != nullptr && epf_check(0, 20, 1, 3, 0.1, 3.0, one) != nullptr);
    // the d = 0 window decides what is too small: ss = 9 asks for 25
    CHECK(epf_check(12, 12, 1, 0, 0.1, 9.0, one) != nullptr && epf_check(13, 13, 1, 0, 0.1, 9.0, one) == nullptr);
    // E1
    CHECK(epf_window(0, 0.3) == 3 && epf_window(0, 1.0) == 5 && epf_window(0, 3.0) == 11 && epf_window(0, 9.0) == 25 &&
          epf_window(0, 1e300) == 25 && epf_window(7, 9.0) == 7);
    // E3: a flat window has no variance and no covariance
    {
        float a, b;
        epf_coeffs(0.5, 0.25, 0.25, 0.125, 0.01, &a, &b);
        CHECK(a == 0.0f && b == 0.25f);
        CHECK(fbits(epf_guided_out(0.5, 0.25, 2.0)) == fbits(1.25f));
    }
    CHECK(epf_finite(1.0) && !epf_finite(NAN) && !epf_finite(-INFINITY) && epf_finite(-0.0));
    CHECK(fbits(epf_centre((uint16_t)16384)) == fbits((float)(16384.0 / 65535.0)));
    // the cases
    const Case cases[] = {
        {13, 13, 25, 0.1, 5.0, 1.0f, 0, -1},        // every tap reflects
        {13, 13, 25, 0.2, 5.0, 0.3f, 1, 0},
        {23, 17, 3, 0.05, 1.0, 1.0f, 1, -1},
        {23, 17, 9, 0.2, 3.0, 0.3f, 0, 1},
        {19, 26, 9, 0.1, 3.0, 1.0f, 1, 1},
        {19, 26, 3, 0.1, 3.0, 0.3f, 0, 0},
        {19, 26, 0, 0.1, 1.0, 0.3f, 0, -1},         // d = 0: 5
    };
    int c = 0;
    for (const Case &k : cases) {
        if (k.word && k.guide == 1) run_case<uint16_t, uint16_t>(c, k);
        else if (k.word) run_case<uint16_t, float>(c, k);
        else if (k.guide == 1) run_case<float, uint16_t>(c, k);
        else run_case<float, float>(c, k);
        c++;
    }
    if (failures) return 1;
    std::printf("epf host ok\n");
    return 0;
}

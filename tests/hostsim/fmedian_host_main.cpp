// fmedian_host_main.cpp -- stand-alone driver of the median filter's shared
// code (siril_amd/csrc/median_host.h: refusals, conversion, the reference
// median of a window, modulation, the selection networks), for a sanitizer
// build:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       fmedian_host_main.cpp -o fmedian_host_main
// Prints, per case, every output sample in hex (tests/test_fmedian_host.py
// compares them with tests/median_ref.py), and proves the 9- and 25-input
// networks by the 0-1 principle: on uint64_t words, AND as the low half of a
// compare-exchange and OR as the high half, 64 zero-one inputs per word, all
// 2^9 and all 2^25 inputs, the output bit against "more than half are 1".
// The 49-input network takes 10^6 random zero-one inputs of every weight and
// 10^5 random key vectors against nth_element.
// Exit status 0 and "fmedian host ok" when every check of its own holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/median_host.h"

using namespace sgpu_med_host;

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
static float bfloat(uint32_t b) {
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

struct BitOp {
    static uint64_t lo(uint64_t a, uint64_t b) { return a & b; }
    static uint64_t hi(uint64_t a, uint64_t b) { return a | b; }
};

// every zero-one input of an N = K*K network: input i of vector number n is bit i of n; 64 vectors per word
template <int K>
static void zero_one() {
    constexpr int N = K * K;
    const uint64_t total = 1ULL << N;
    uint64_t bad = 0;
    for (uint64_t base = 0; base < total; base += 64) {
        uint64_t v[N], more = 0;
        // base is a multiple of 64: inputs 0 .. 5 vary with the lane, the others are the same in all 64
        const uint64_t lane[6] = {0xAAAAAAAAAAAAAAAAULL, 0xCCCCCCCCCCCCCCCCULL, 0xF0F0F0F0F0F0F0F0ULL,
                                  0xFF00FF00FF00FF00ULL, 0xFFFF0000FFFF0000ULL, 0xFFFFFFFF00000000ULL};
        for (int i = 0; i < N; i++) v[i] = i < 6 ? lane[i] : ((base >> i) & 1ULL ? ~0ULL : 0ULL);
        for (uint64_t l = 0; l < 64; l++) more |= (uint64_t)(__builtin_popcountll(base + l) > N / 2) << l;
        bad += med_network<BitOp, K>(v) != more;
    }
    if (bad) std::printf("the %d-input network fails on %llu words of zero-one inputs\n", N, (unsigned long long)bad);
    failures += bad != 0;
}

// The 49-input network: 10^6 random zero-one inputs, vector n of weight n % 50 (every weight 0 .. 49), 64 per word,
// and 10^5 random key vectors (one in three from eight values only) against nth_element.
static void sample_49() {
    constexpr int N = 49;
    uint32_t s = 2463534242u;
    auto next = [&s]() { return s ^= s << 13, s ^= s >> 17, s ^= s << 5; };
    uint64_t bad = 0;
    for (int word = 0; word < 1000000 / 64; word++) {
        uint64_t v[N] = {}, more = 0;
        for (int l = 0; l < 64; l++) {
            const int weight = (word * 64 + l) % 50;
            int place[N];
            for (int i = 0; i < N; i++) place[i] = i;
            for (int i = 0; i < weight; i++) {          // the first `weight` places of a random permutation are 1
                const int j = i + (int)(next() % (uint32_t)(N - i)), t = place[i];
                place[i] = place[j], place[j] = t;
                v[place[i]] |= 1ULL << l;
            }
            more |= (uint64_t)(weight > N / 2) << l;
        }
        bad += med_network<BitOp, 7>(v) != more;
    }
    std::vector<uint32_t> keys;
    for (int t = 0; t < 100000; t++) {
        uint32_t k[N];
        for (int i = 0; i < N; i++) k[i] = t % 3 == 0 ? next() >> 29 : next();
        keys.assign(k, k + N);
        std::nth_element(keys.begin(), keys.begin() + N / 2, keys.end());
        bad += med_network<MedKeyOp, 7>(k) != keys[N / 2];
    }
    if (bad) std::printf("the 49-input network fails on %llu samples\n", (unsigned long long)bad);
    failures += bad != 0;
}

// the scene of tests/test_fmedian_host.py, an integer below 997
static int scene(int c, int x, int y) { return (x * 37 + y * 101 + 13 * c + (x * y) % 29 * 31) % 997; }

template <typename T>
static void run_case(int c, int W, int H, int ksize, float mod, int iter, const std::vector<T> &plane) {
    CHECK(med_check(W, H, ksize, mod, iter) == nullptr);
    std::vector<float> out((size_t)W * H);
    med_filter_host(plane.data(), W, H, ksize, mod, iter, out.data());
    std::printf("case %d %d %d %d %08x %d %d\nout", c, W, H, ksize, fbits(mod), iter, (int)(sizeof(T) == 2));
    for (float v : out) std::printf(" %08x", fbits(v));
    std::printf("\n");
}

int main() {
    // M5 at its exact boundaries
    CHECK(med_check(8, 8, 15, 1.0f, 1) == nullptr);
    CHECK(med_check(7, 9, 15, 1.0f, 1) != nullptr && med_check(9, 7, 15, 1.0f, 1) != nullptr);
    CHECK(med_check(2, 2, 3, 1.0f, 1) == nullptr && med_check(1, 5, 3, 1.0f, 1) != nullptr);
    CHECK(med_check(50, 50, 1, 1.0f, 1) != nullptr && med_check(50, 50, 4, 1.0f, 1) != nullptr &&
          med_check(50, 50, 17, 1.0f, 1) != nullptr && med_check(50, 50, 16, 1.0f, 1) != nullptr);
    CHECK(med_check(50, 50, 3, 0.0f, 1) == nullptr && med_check(50, 50, 3, -0.0f, 1) == nullptr);
    CHECK(med_check(50, 50, 3, -0.001f, 1) != nullptr && med_check(50, 50, 3, 1.001f, 1) != nullptr &&
          med_check(50, 50, 3, NAN, 1) != nullptr && med_check(50, 50, 3, INFINITY, 1) != nullptr);
    CHECK(med_check(50, 50, 3, 1.0f, 0) != nullptr && med_check(50, 50, 3, 1.0f, 9) != nullptr &&
          med_check(50, 50, 3, 1.0f, 8) == nullptr);
    CHECK(med_check(65535, 20, 3, 1.0f, 1) == nullptr && med_check(65536, 20, 3, 1.0f, 1) != nullptr &&
          med_check(20, 65536, 3, 1.0f, 1) != nullptr && med_check(0, 20, 3, 1.0f, 1) != nullptr);
    CHECK(med_radius(3) == 1 && med_radius(15) == 7 && med_rank(3) == 4 && med_rank(15) == 112);
    // M2: the order -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN, and the way back
    {
        const uint32_t order[8] = {0xFFC00001u, 0xFF800000u, 0xBF800000u, 0x80000000u,
                                   0x00000000u, 0x3F800000u, 0x7F800000u, 0x7FC00001u};
        for (int i = 0; i + 1 < 8; i++) CHECK(med_key(bfloat(order[i])) < med_key(bfloat(order[i + 1])));
        for (int i = 0; i < 8; i++) CHECK(fbits(med_unkey(med_key(bfloat(order[i])))) == order[i]);
    }
    // M3
    CHECK(fbits(med_modulate(1.0f, bfloat(0x7FC00123u), 0.5f)) == 0x7FC00123u);
    CHECK(fbits(med_modulate(0.5f, 0.25f, 3.0f)) == fbits(0.5f * 0.25f + 0.5f * 3.0f));
    CHECK(fbits(med_modulate(0.0f, 0.25f, 3.0f)) == fbits(3.0f));
    CHECK(med_ncandidates(3) == 3 && med_ncandidates(5) == 13);
    // the networks
    zero_one<3>();
    zero_one<5>();
    sample_49();
    // ... and on keys against nth_element, duplicates included
    {
        uint32_t s = 12345u;
        std::vector<uint32_t> keys;
        for (int t = 0; t < 20000; t++) {
            uint32_t v9[9], v25[25];
            for (int i = 0; i < 25; i++) {
                s = s * 1664525u + 1013904223u;
                v25[i] = t % 3 == 0 ? (s >> 29) : s;        // one in three draws from eight values only
                if (i < 9) v9[i] = v25[i];
            }
            keys.assign(v9, v9 + 9);
            std::nth_element(keys.begin(), keys.begin() + 4, keys.end());
            CHECK((med_network<MedKeyOp, 3>(v9)) == keys[4]);
            keys.assign(v25, v25 + 25);
            std::nth_element(keys.begin(), keys.begin() + 12, keys.end());
            CHECK((med_network<MedKeyOp, 5>(v25)) == keys[12]);
        }
    }
    // the cases: width, height, ksize, modulation, iterations
    const struct {
        int W, H, ksize;
        float mod;
        int iter;
    } cases[6] = {{33, 21, 3, 1.0f, 1}, {40, 37, 7, 0.3f, 1}, {23, 19, 15, 1.0f, 2},
                  {8, 8, 15, 0.3f, 1}, {17, 30, 3, 0.3f, 2}, {29, 16, 7, 1.0f, 1}};
    for (int c = 0; c < 6; c++) {
        const int W = cases[c].W, H = cases[c].H;
        if (c & 1) {
            std::vector<uint16_t> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (uint16_t)(scene(c, x, y) * 61);
            run_case(c, W, H, cases[c].ksize, cases[c].mod, cases[c].iter, pl);
        } else {
            std::vector<float> pl((size_t)W * H);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) pl[(size_t)y * W + x] = (float)scene(c, x, y) * (1.0f / 1024.0f);
            run_case(c, W, H, cases[c].ksize, cases[c].mod, cases[c].iter, pl);
        }
    }
    if (failures) return 1;
    std::printf("fmedian host ok\n");
    return 0;
}

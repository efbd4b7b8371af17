// tests/hostsim/wz_split_main.cpp -- TEST BUILD: the split rounds of the
// WINSORIZED moment path (stack_wz.h: k_stack_wz_rounds_lds with a rounds cap,
// then k_stack_wz_tail twice) restated on the host, one column at a time, and
// compared with the one-call wz_finish.
//
// For caps 1, 2 and 3 every column runs the decomposition exactly as the
// kernels do: wz_finish_cap (the head), the WzState copied out through memory,
// WzConst rebuilt with wz_consts, `cap` more rounds (tail pass 1), a second
// deferral through memory, then every remaining round (tail pass 2).  Any
// difference in route, result bits, rl, rh, nkept, pmin or pmax fails; so do
// column families that do not exercise the resume (see the exercise checks in
// main).  Stand-alone: built for the host with the address and undefined-
// behaviour sanitizers and run as its own process (tests/test_wz_split_host.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "stack_wz.h"

using namespace sgpu;

namespace {

constexpr int NP = 128;
using RS = RankStore<NP, 1>;

// splitmix64 / Box-Muller: seeded, the same columns on every machine
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }
    double normal() {
        const double u = uni() + 0x1p-54, v = uni();
        return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
    }
};

enum Kind { RECIPE, ZEROS, TIES, CONSTANT, HEAVY };

// one column of n samples (0 = missing, as in the frames)
void make_column(Rng &r, Kind kind, int n, float *col) {
    const double level = 0.05 + 0.02 * r.uni();
    for (int f = 0; f < n; f++) {
        double x = level + 0.005 * r.normal();
        if (kind == HEAVY) {                       // Cauchy tails
            x = level + 0.002 * std::tan(3.141592653589793 * (r.uni() - 0.5));
        } else {
            if (r.uni() < 0.01) x += 0.2 + 0.4 * r.uni();      // cosmic ray
            if (r.uni() < 0.001) x *= 0.1;                     // cold pixel
        }
        if (kind == TIES) x = std::round(x * 512.0) / 512.0;
        if (kind == CONSTANT) x = level;
        x = x < 1e-6 ? 1e-6 : (x > 1.0 ? 1.0 : x);
        col[f] = (float)x;
        if (kind == ZEROS && r.uni() < 0.2) col[f] = 0.f;
    }
    if (kind == CONSTANT && r.uni() < 0.5) col[(int)(r.uni() * n)] += 0.25f;   // one outlier on a flat column
}

struct Result {
    int route;
    PixOut o;
};

bool same(const Result &a, const Result &b) {
    if (a.route != b.route) return false;
    if (a.route != 0) return true;
    return std::memcmp(&a.o.res, &b.o.res, sizeof a.o.res) == 0 && a.o.rl == b.o.rl && a.o.rh == b.o.rh &&
           a.o.nkept == b.o.nkept && std::memcmp(&a.o.pmin, &b.o.pmin, sizeof(float)) == 0 &&
           std::memcmp(&a.o.pmax, &b.o.pmax, sizeof(float)) == 0;
}

// the device's wz_state area: the state leaves the "lane" and comes back
volatile unsigned char g_state_mem[sizeof(WzState)];
void through_memory(WzState &st) {
    unsigned char tmp[sizeof(WzState)];
    std::memcpy(tmp, &st, sizeof st);
    for (size_t i = 0; i < sizeof st; i++) g_state_mem[i] = tmp[i];
    std::memset(&st, 0xa5, sizeof st);
    for (size_t i = 0; i < sizeof st; i++) tmp[i] = g_state_mem[i];
    std::memcpy(&st, tmp, sizeof st);
}

struct Family {
    const char *name;
    Kind kind;
    int n;
    float s0, s1;
    int columns;
};

struct Tally {
    long long columns = 0, deferred1 = 0, deferred2 = 0, mismatches = 0;
};

// prepares the column like k_stack_wz_prep (G == 1) and runs reference and split
Tally run_family(const Family &fam, int cap, uint64_t seed) {
    Tally t;
    Rng rng(seed);
    std::vector<float> ranks((size_t)RS::R * RS::PW);
    float col[NP];
    for (int c = 0; c < fam.columns; c++) {
        make_column(rng, fam.kind, fam.n, col);
        float v[NP];
        int kept = 0;
        for (int e = 0; e < NP; e++) {
            float x = f_inf();
            if (e < fam.n && col[e] != 0.f) {
                x = col[e];
                kept++;
            }
            v[e] = x;
        }
        RS rs;
        rs.base = ranks.data();
        rs.stride = RS::PW;
        rs.p = 0;
        double W1, W2;
        float c0;
        if (wz_prepare<NP, 1>(v, 0, kept, kept, fam.n, rs, W1, W2, c0)) continue;   // kept == 0
        const int m = NP;                          // G * E of the one-lane layout
        t.columns++;
        Result ref, got;
        ref.route = wz_finish(rs, kept, W1, W2, c0, m, fam.s0, fam.s1, ref.o);
        // head
        WzState st;
        got.route = wz_finish_cap(rs, kept, W1, W2, c0, m, fam.s0, fam.s1, cap, got.o, st);
        // tail pass 1 (defers again), tail pass 2 (to the end)
        for (int pass = 0; pass < 2 && got.route == kWzDeferred; pass++) {
            (pass == 0 ? t.deferred1 : t.deferred2)++;
            through_memory(st);
            WzConst k;
            float ymax, vmin;
            got.route = wz_consts(rs, kept, c0, m, fam.s0, fam.s1, k, ymax, vmin);
            got.o.fallback = 0;
            if (!got.route) got.route = wz_rounds_cap(rs, k, st, pass == 1 ? -1 : cap, got.o);
        }
        if (!same(ref, got)) {
            if (t.mismatches++ < 5)
                std::fprintf(stderr, "MISMATCH %s cap %d column %d: route %d / %d\n", fam.name, cap, c, ref.route,
                             got.route);
        }
    }
    return t;
}

}  // namespace

int main() {
    const Family fams[] = {
        {"recipe N=65 s3/3", RECIPE, 65, 3.f, 3.f, 4096},    {"recipe N=70 s3/3", RECIPE, 70, 3.f, 3.f, 4096},
        {"recipe N=100 s3/3", RECIPE, 100, 3.f, 3.f, 8192},  {"recipe N=128 s3/3", RECIPE, 128, 3.f, 3.f, 4096},
        {"recipe N=70 s2/2", RECIPE, 70, 2.f, 2.f, 8192},    {"recipe N=100 s2/2", RECIPE, 100, 2.f, 2.f, 4096},
        {"recipe N=100 s1.5/2", RECIPE, 100, 1.5f, 2.f, 4096}, {"zeros N=100 s3/3", ZEROS, 100, 3.f, 3.f, 4096},
        {"zeros N=65 s2/2", ZEROS, 65, 2.f, 2.f, 4096},      {"ties N=100 s3/3", TIES, 100, 3.f, 3.f, 4096},
        {"ties N=128 s2/2", TIES, 128, 2.f, 2.f, 4096},      {"constant N=100 s3/3", CONSTANT, 100, 3.f, 3.f, 2048},
        {"heavy N=100 s3/3", HEAVY, 100, 3.f, 3.f, 4096},    {"heavy N=70 s1.5/2", HEAVY, 70, 1.5f, 2.f, 4096},
    };
    long long bad = 0;
    int fail = 0;
    for (int cap = 1; cap <= 3; cap++) {
        int fi = 0;
        for (const Family &f : fams) {
            const Tally t = run_family(f, cap, 20260821ull + 1000ull * (uint64_t)fi++);
            std::printf("cap %d  %-22s columns %6lld  deferred once %6lld (%5.1f %%)  twice %6lld (%5.1f %%)  "
                        "mismatches %lld\n",
                        cap, f.name, t.columns, t.deferred1, 100.0 * t.deferred1 / (double)t.columns, t.deferred2,
                        100.0 * t.deferred2 / (double)t.columns, t.mismatches);
            bad += t.mismatches;
            // exercise checks: the resume must really run
            if (cap == 2 && f.kind == RECIPE && f.n == 100 && f.s0 == 3.f && t.deferred1 * 100 < t.columns) {
                std::fprintf(stderr, "FAIL: %s defers under 1 %% of its columns at cap 2\n", f.name);
                fail = 1;
            }
            if (cap == 2 && f.kind == RECIPE && f.n == 70 && f.s0 == 2.f && t.deferred2 * 10 < t.columns) {
                std::fprintf(stderr, "FAIL: %s defers under 10 %% of its columns twice at cap 2\n", f.name);
                fail = 1;
            }
        }
    }
    if (bad) {
        std::fprintf(stderr, "FAIL: %lld columns differ from wz_finish\n", bad);
        fail = 1;
    }
    if (!fail) std::printf("wz_split ok\n");
    return fail;
}

// tests/hostsim/wz_fused_main.cpp -- TEST BUILD: the fused kernel of the
// WINSORIZED moment path (stack_wz.h: k_stack_wz_fused1) against the two
// kernels it replaces, one column at a time on the host.
//
// Every column runs twice from the same gathered samples:
//   fused:      wz_prepare1<RSL, true> (the ranks go to a wave's LDS tile:
//               RankStore::store_full_lds, or RankStore::store when kept is
//               below the bucket's floor), then wz_finish_cap on that tile;
//   two-kernel: wz_prepare1<RSL> (the HBM record: store_full / store_buf with
//               the descriptor's range check restated), the meta words through
//               an int4, the record's column copied into a tile as
//               k_stack_wz_rounds_lds stages it, then wz_finish_cap.
// Route, WzState bytes, PixOut, the meta words, the moments and c0 must be
// equal, and so must every rank either tile answers (RankStore::fetch over
// [0, kept)).  A lane of a device wave also takes the run-time slot loops with
// a kmin that is another lane's kept: store() and store_buf() are compared on
// every column with kmin = 1, kept / 2 and kept as well.  N = 65, 72, 73, 100,
// 104, 105, 120, 121, 128 (each real-slot bucket's ends); the 14 families of
// wz_split_main.cpp, kept of 1-3 and 39-41, constant columns and walks past
// the 16 stored ranks.  The program also fails when its families miss the
// cases they are there for.  Stand-alone: built for the host with the address
// and undefined-behaviour sanitizers and run as its own process
// (tests/test_wz_fused_host.py).
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
constexpr int kCap = 2;            // the head's rounds cap (SGPU_WZ_SPLIT default)
constexpr int kCnt = 200;          // pixels of the model chunk (the record's stride)

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

// the kinds of wz_walk_main.cpp: the five of wz_split_main.cpp, a core with
// `arg` samples 8-8.5 widths out at one end (PLANT_*: the first clamp
// iteration takes exactly those), `arg` samples present (KEPT), one value (FLAT)
enum Kind { RECIPE, ZEROS, TIES, CONSTANT, HEAVY, PLANT_LO, PLANT_HI, KEPT, FLAT };

void make_column(Rng &r, Kind kind, int n, int arg, float *col) {
    const double level = 0.05 + 0.02 * r.uni();
    for (int f = 0; f < n; f++) {
        double x = level + 0.005 * r.normal();
        if (kind == HEAVY) {
            x = level + 0.002 * std::tan(3.141592653589793 * (r.uni() - 0.5));
        } else if (kind == PLANT_LO || kind == PLANT_HI) {
            const double w = 0.005;
            x = level + w * (2.0 * r.uni() - 1.0);
            if (f < arg) x = level + (kind == PLANT_LO ? -1.0 : 1.0) * w * (8.0 + 0.5 * r.uni());
        } else if (kind != FLAT) {
            if (r.uni() < 0.01) x += 0.2 + 0.4 * r.uni();
            if (r.uni() < 0.001) x *= 0.1;
        }
        if (kind == TIES) x = std::round(x * 512.0) / 512.0;
        if (kind == CONSTANT || kind == FLAT) x = level;
        x = x < 1e-6 ? 1e-6 : (x > 1.0 ? 1.0 : x);
        col[f] = (float)x;
        if (kind == ZEROS && r.uni() < 0.2) col[f] = 0.f;
        if (kind == KEPT && f >= arg) col[f] = 0.f;
    }
    if (kind == CONSTANT && r.uni() < 0.5) col[(int)(r.uni() * n)] += 0.25f;
}

struct Family {
    const char *name;
    Kind kind;
    float s0, s1;
    int columns, arg;
};

struct Tally {
    long long columns = 0, full = 0, slots = 0, deferred = 0, fallback = 0, results = 0, mismatches = 0;
};

bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }

// the gathered column of gather_column<.., DROP_ZERO>: samples in frame
// order, a null one and every slot past the last frame +Inf
int gathered(const float *col, int n, float (&v)[NP]) {
    int kept = 0;
    for (int e = 0; e < NP; e++) {
        v[e] = f_inf();
        if (e < n && col[e] != 0.f) {
            v[e] = col[e];
            kept++;
        }
    }
    return kept;
}

template <int RSL>
void run_column(const Family &fam, int n, const float *col, int c, Tally &t) {
    const float canary = __builtin_nanf("");
    const int lane = c & 63, loc = (c * 37) % kCnt;
    float v[NP];
    const int kept = gathered(col, n, v);
    if (kept == 0) return;                    // the kernels route it to the exact kernel before any rank is read
    t.columns++;
    (kept >= RSL - 7 ? t.full : t.slots)++;
    const int el = (n + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);

    // fused: the wave's LDS tile
    std::vector<float> tile_a((size_t)RS::R * 64, canary);
    RS ra;
    ra.base = tile_a.data();
    ra.stride = 64;
    ra.p = lane;
    double W1a, W2a;
    float c0a;
    {
        float w[NP];
        std::memcpy(w, v, sizeof w);
        wz_prepare1<RSL, true>(w, kept, n, ra, W1a, W2a, c0a);
    }
    PixOut oa;
    WzState sta;
    std::memset(&oa, 0, sizeof oa);
    std::memset(&sta, 0, sizeof sta);
    const int route_a = wz_finish_cap<0>(ra, kept, W1a, W2a, c0a, el, fam.s0, fam.s1, kCap, oa, sta);

    // two-kernel: the HBM record, the meta words, the staged tile
    std::vector<float> rec((size_t)RS::R * kCnt, canary), tile_b((size_t)RS::R * 64, canary);
    RS rp;
    rp.base = rec.data();
    rp.stride = kCnt;
    rp.p = loc;
    double W1b, W2b;
    float c0b;
    {
        float w[NP];
        std::memcpy(w, v, sizeof w);
        wz_prepare1<RSL>(w, kept, n, rp, W1b, W2b, c0b);
    }
    const int meta[4] = {kept, rp.hi0, rp.mid0, rp.mid1};
    for (int j = 0; j < RS::R; j++) tile_b[(size_t)j * 64 + lane] = rec[(size_t)j * kCnt + loc];
    RS rb;
    rb.base = tile_b.data();
    rb.stride = 64;
    rb.p = lane;
    rb.kept = meta[0];
    rb.hi0 = meta[1];
    rb.mid0 = meta[2];
    rb.mid1 = meta[3];
    PixOut ob;
    WzState stb;
    std::memset(&ob, 0, sizeof ob);
    std::memset(&stb, 0, sizeof stb);
    const int route_b = wz_finish_cap<0>(rb, kept, W1b, W2b, c0b, el, fam.s0, fam.s1, kCap, ob, stb);

    bool ok = route_a == route_b && same_bits(&sta, &stb, sizeof sta);
    ok = ok && ra.kept == meta[0] && ra.hi0 == meta[1] && ra.mid0 == meta[2] && ra.mid1 == meta[3];
    ok = ok && same_bits(&W1a, &W1b, 8) && same_bits(&W2a, &W2b, 8) && same_bits(&c0a, &c0b, 4);
    if (route_a == 0)
        ok = ok && same_bits(&oa.res, &ob.res, 8) && oa.rl == ob.rl && oa.rh == ob.rh && oa.nkept == ob.nkept &&
             same_bits(&oa.pmin, &ob.pmin, 4) && same_bits(&oa.pmax, &ob.pmax, 4);
    // every rank either tile answers, and nothing stored outside the lane's column
    for (int r = 0; r < kept; r++) {
        float xa = 0.f, xb = 0.f;
        const bool fa = ra.fetch(r, xa), fb = rb.fetch(r, xb);
        ok = ok && fa == fb && (!fa || same_bits(&xa, &xb, 4));
    }
    for (size_t i = 0; i < tile_a.size(); i++)
        if ((int)(i & 63) != lane && tile_a[i] == tile_a[i]) ok = false;

    // the run-time slot loops with another lane's kmin
    float s[NP];
    std::memcpy(s, v, sizeof s);
    sort_col<NP, 1, RSL>(s, 0);
    const int kmins[3] = {1, kept / 2 > 0 ? kept / 2 : 1, kept};
    for (int kmin : kmins) {
        std::vector<float> ta((size_t)RS::R * 64, canary), tr((size_t)RS::R * kCnt, canary);
        RS a, b;
        a.base = ta.data();
        a.stride = 64;
        a.p = lane;
        a.kept = kept;
        b.base = tr.data();
        b.stride = kCnt;
        b.p = loc;
        b.kept = kept;
        a.store(s, 0, kmin, n);
        b.store_buf(s, 0, kmin, n);
        ok = ok && a.hi0 == b.hi0 && a.mid0 == b.mid0 && a.mid1 == b.mid1;
        for (int r = 0; r < kept; r++) {
            float xa = 0.f, xb = 0.f;
            const bool fa = a.fetch(r, xa), fb = b.fetch(r, xb);
            ok = ok && fa == fb && (!fa || same_bits(&xa, &xb, 4));
        }
    }

    t.deferred += route_a == kWzDeferred;
    t.fallback += route_a == 1;
    t.results += route_a == 0;
    if (!ok && t.mismatches++ < 5)
        std::fprintf(stderr, "MISMATCH %s N %d column %d kept %d: route %d / %d\n", fam.name, n, c, kept, route_a,
                     route_b);
}

template <int RSL>
Tally run_family(const Family &fam, int n, uint64_t seed) {
    Tally t;
    Rng rng(seed);
    float col[NP];
    for (int c = 0; c < fam.columns; c++) {
        make_column(rng, fam.kind, n, fam.arg, col);
        run_column<RSL>(fam, n, col, c, t);
    }
    return t;
}

// the bucket of the one-lane prep's picker (rs_pick_prep1: N in [RSL - 7, RSL], from 72)
Tally run_family_n(const Family &fam, int n, uint64_t seed) {
    const int rsl = n <= 72 ? 72 : (n + 7) & ~7;
    switch (rsl) {
        case 72: return run_family<72>(fam, n, seed);
        case 80: return run_family<80>(fam, n, seed);
        case 104: return run_family<104>(fam, n, seed);
        case 112: return run_family<112>(fam, n, seed);
        case 120: return run_family<120>(fam, n, seed);
        default: return run_family<128>(fam, n, seed);
    }
}

}  // namespace

int main() {
    const Family fams[] = {
        // the 14 families of wz_split_main.cpp (kind and sigmas; N from the list below)
        {"recipe s3/3", RECIPE, 3.f, 3.f, 256, 0},     {"recipe s3/3 b", RECIPE, 3.f, 3.f, 256, 0},
        {"recipe s3/3 c", RECIPE, 3.f, 3.f, 512, 0},   {"recipe s3/3 d", RECIPE, 3.f, 3.f, 256, 0},
        {"recipe s2/2", RECIPE, 2.f, 2.f, 512, 0},     {"recipe s2/2 b", RECIPE, 2.f, 2.f, 256, 0},
        {"recipe s1.5/2", RECIPE, 1.5f, 2.f, 256, 0},  {"zeros s3/3", ZEROS, 3.f, 3.f, 256, 0},
        {"zeros s2/2", ZEROS, 2.f, 2.f, 256, 0},       {"ties s3/3", TIES, 3.f, 3.f, 256, 0},
        {"ties s2/2", TIES, 2.f, 2.f, 256, 0},         {"constant s3/3", CONSTANT, 3.f, 3.f, 256, 0},
        {"heavy s3/3", HEAVY, 3.f, 3.f, 256, 0},       {"heavy s1.5/2", HEAVY, 1.5f, 2.f, 256, 0},
        // few samples, the three regions overlapping (kept < R = 40) or just apart
        {"kept 1", KEPT, 3.f, 3.f, 32, 1},             {"kept 2", KEPT, 3.f, 3.f, 64, 2},
        {"kept 3", KEPT, 3.f, 3.f, 64, 3},             {"kept 39", KEPT, 3.f, 3.f, 128, 39},
        {"kept 40", KEPT, 3.f, 3.f, 128, 40},          {"kept 41", KEPT, 3.f, 3.f, 128, 41},
        {"flat", FLAT, 3.f, 3.f, 32, 0},
        // walks past the 16 stored ranks of an end: the sorted kernel's pixels
        {"plant lo 17", PLANT_LO, 3.f, 3.f, 64, 17},   {"plant lo 20", PLANT_LO, 3.f, 3.f, 64, 20},
        {"plant hi 17", PLANT_HI, 3.f, 3.f, 64, 17},   {"plant hi 20", PLANT_HI, 3.f, 3.f, 64, 20},
    };
    const int ns[] = {65, 72, 73, 100, 104, 105, 120, 121, 128};
    long long bad = 0;
    int fail = 0;
    for (int n : ns) {
        Tally all;
        long long planted = 0, planted_fb = 0;
        int fi = 0;
        for (const Family &f : fams) {
            const Tally t = run_family_n(f, n, 20261020ull + 1000ull * (uint64_t)fi++ + (uint64_t)n);
            all.columns += t.columns;
            all.full += t.full;
            all.slots += t.slots;
            all.deferred += t.deferred;
            all.fallback += t.fallback;
            all.results += t.results;
            all.mismatches += t.mismatches;
            if (f.kind == PLANT_LO || f.kind == PLANT_HI) {
                planted += t.columns;
                planted_fb += t.fallback;
            }
        }
        std::printf("N %3d  columns %6lld  straight-line store %6lld  slot loops %6lld  deferred %5lld  "
                    "fallback %5lld  results %6lld  mismatches %lld\n",
                    n, all.columns, all.full, all.slots, all.deferred, all.fallback, all.results, all.mismatches);
        bad += all.mismatches;
        // exercise checks
        if (all.full * 2 < all.columns || all.slots * 20 < all.columns) {
            std::fprintf(stderr, "FAIL: N %d does not run both store forms\n", n);
            fail = 1;
        }
        // (each end of the head must be well represented, no more: one column
        // in a hundred deferred, one in ten finished inside the cap)
        if (all.deferred * 100 < all.columns || all.results * 10 < all.columns) {
            std::fprintf(stderr, "FAIL: N %d: too few deferred or finished columns\n", n);
            fail = 1;
        }
        if (planted_fb * 2 < planted) {
            std::fprintf(stderr, "FAIL: N %d: the planted walks stay inside the stored ranks\n", n);
            fail = 1;
        }
    }
    if (bad) {
        std::fprintf(stderr, "FAIL: %lld columns differ between the fused and the two-kernel form\n", bad);
        fail = 1;
    }
    if (!fail) std::printf("wz_fused ok\n");
    return fail;
}

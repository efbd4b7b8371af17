// tests/hostsim/wz_walk_main.cpp -- TEST BUILD: the rejection rounds of the
// WINSORIZED moment path (stack_wz.h: wz_round with its straight-line clamp
// walks, the end-region fetches and the one-exit iteration loop) against the
// form they replace, one column and one round at a time.
//
// The reference below is a verbatim copy of wz_round, wz_clip_counts and
// RankStore::fetch as they stood before the walks were rewritten (the default
// build's text: exits inside the walks, the generic fetch everywhere).  Both
// forms start from the same prepared column; after every round the WzState
// bytes (moments, error bounds, window, counters), the return code and `more`
// must be equal, and at the end route, result bits, rl, rh, nkept, pmin and
// pmax.  The program also fails when its planted families do not reach the
// cases they are there for (see the exercise checks in main).  Stand-alone:
// built for the host with the address and undefined-behaviour sanitizers and
// run as its own process (tests/test_wz_walk_host.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "stack_wz.h"

using namespace sgpu;

namespace ref {

// ---- verbatim: stack_wz.h before the straight-line walks
template <class TS>
SG_HD int wz_clip_counts(const TS &ts, int lo, int hi, float mf, float tl0, float th0, float tl1, float th1,
                         int &cl, int &ch) {
    float x;
    int k = 0;
    for (;;) {
        if (lo + k >= hi || !ts.fetch(lo + k, x)) return 2;
        if (!(mf - x > tl1)) break;
        k++;
    }
    if (mf - x > tl0) return 1;
    cl = k;
    k = 0;
    for (;;) {
        if (hi - 1 - k < lo + cl || !ts.fetch(hi - 1 - k, x)) return 2;
        if (!(x - mf > th1)) break;
        k++;
    }
    if (x - mf > th0) return 1;
    ch = k;
    return 0;
}

template <int NP, int G>
struct Store : RankStore<NP, G> {
    using B = RankStore<NP, G>;
    static constexpr int KT = B::KT, KM = B::KM;
    SG_HD bool fetch(int r, float &x) const {
        const int kept = this->kept, hi0 = this->hi0, mid0 = this->mid0, mid1 = this->mid1;
        float *const base = this->base;
        const long long stride = this->stride, p = this->p;
        const bool lo_ok = r < KT && r < kept, hi_ok = r >= hi0 && r < kept, mid_ok = r >= mid0 && r < mid1;
        const int slot = lo_ok ? r : hi_ok ? KT + KM + r - (kept - KT) : KT + r - (kept / 2 - KM / 2);
        const bool ok = lo_ok || hi_ok || mid_ok;
        x = (base + p)[umul24((unsigned)(ok ? slot : 0), (unsigned)stride)];
        return ok;
    }
};

template <int U16 = 0, class RS>
SG_HD int wz_round(const RS &rs, const WzConst &k, WzState &st, bool &more) {
    const float c0 = k.c0, eps = k.eps, sgc = k.sgc;
    int lo = st.lo, hi = st.hi;
    const int n = hi - lo;
    const double rn = 1.0 / n, rn1 = 1.0 / (n - 1);
    float ma, mb;
    if (!rs.fetch(lo + n / 2 - ((n & 1) ? 0 : 1), ma) || !rs.fetch(lo + n / 2, mb)) return 1;
    const float mf = median_from(ma, mb, n);
    SGPU_WZ_TRACE(0);
    float xw0, xw1;
    if (!rs.fetch(lo, xw0) || !rs.fetch(hi - 1, xw1)) return 1;
    // the round's first sd (siril_stats_float_sd of the window, :226)
    float vlo, vhi;
    const bool flat = xw0 == xw1;         // constant window: every sd below is exactly 0
    var_bounds(st.W1, st.W2, st.E1, st.E2, 0, 0, n, c0, 0.f, 0.f, 0.f, 0.f, false, eps, sgc, rn, rn1, vlo, vhi);
    if (flat) vlo = vhi = 0.f;
    float slo = sqrt_lo(vlo), shi = sqrt_hi(vhi);
    // clamp iterations (:229-237)
    float Llo = -f_inf(), Lhi = -f_inf(), Ulo = f_inf(), Uhi = f_inf();
    int a = 0, c = 0;
    double R1 = st.W1, R2 = st.W2;
    float F1 = st.E1, F2 = st.E2;
    float nlo = xw0, nhi = xw1;           // next samples to clamp: ranks lo + a, hi - 1 - c
    for (int it = 0;;) {
        const float tlo = 1.5f * slo, thi = 1.5f * shi;
        float m0lo = mf - thi, m0hi = mf - tlo, m1lo = mf + tlo, m1hi = mf + thi;
        if (U16) {   // roundf_to_WORD of every end (monotone)
            m0lo = roundf_to_word_f(m0lo);
            m0hi = roundf_to_word_f(m0hi);
            m1lo = roundf_to_word_f(m1lo);
            m1hi = roundf_to_word_f(m1hi);
        }
        Llo = fminf(m1lo, fmaxf(m0lo, Llo));
        Lhi = fminf(m1hi, fmaxf(m0hi, Lhi));
        Ulo = fminf(m1lo, fmaxf(m0lo, Ulo));
        Uhi = fminf(m1hi, fmaxf(m0hi, Uhi));
        while (nlo < Lhi) {
            wz_take(nlo, c0, eps, R1, R2, F1, F2);
            if (++a + c >= n || !rs.fetch(lo + a, nlo)) return 1;
        }
        while (nhi > Ulo) {
            wz_take(nhi, c0, eps, R1, R2, F1, F2);
            if (a + ++c >= n || !rs.fetch(hi - 1 - c, nhi)) return 1;
        }
        SGPU_WZ_TRACE(1);
        var_bounds(R1, R2, F1, F2, a, c, n, c0, Llo, Lhi, Ulo, Uhi, true, eps, sgc, rn, rn1, vlo, vhi);
        if (flat) vlo = vhi = 0.f;
        if (!(vhi - vhi == 0.f)) return 1;
        const float s0lo = slo, s0hi = shi;
        slo = 1.134f * sqrt_lo(vlo);
        shi = 1.134f * sqrt_hi(vhi);
        const float A = slo - s0hi, B = shi - s0lo;      // fl(sigma - sigma0) in [A, B]
        const float dmin = A > 0.f ? A : (B < 0.f ? -B : 0.f);
        const float dmax = fmaxf(fabsf(A), fabsf(B));
        if (dmin > s0hi * 0.0005f) {
            if (++it > kWinsorCap) return 1;
            continue;
        }
        if (dmax <= s0lo * 0.0005f) break;
        return 1;
    }
    // sigma_clipping_float (:238-246) with sigma in [slo, shi]
    int cl = 0, ch = 0;
    if (n - st.r > 4) {
        const float tl0 = slo * k.slo_, th0 = slo * k.shi_, tl1 = shi * k.slo_, th1 = shi * k.shi_;
        if (!(tl0 >= 0.f && th0 >= 0.f)) return 2;
        if (ref::wz_clip_counts(rs, lo, hi, mf, tl0, th0, tl1, th1, cl, ch)) return 1;   // (qualified: the only edit)
    }
    // the clipped samples leave the moments (before the window moves)
    const int lo0 = lo, hi0 = hi;
    bool changed;
    if (cutoff_round(n, st.r, cl, ch, lo, hi, st.rl, st.rh, changed)) return 2;
    for (int j = 0; j < lo - lo0 + (hi0 - hi); j++) {
        float x;
        const int rk = j < lo - lo0 ? lo0 + j : hi0 - 1 - (j - (lo - lo0));
        if (!rs.fetch(rk, x)) return 1;
        wz_take(x, c0, eps, st.W1, st.W2, st.E1, st.E2);
    }
    st.lo = lo;
    st.hi = hi;
    more = changed && hi - lo > 3;
    return 0;
}
// ---- end of the verbatim copy

}  // namespace ref

namespace {

constexpr int NP = 128;
using RS = RankStore<NP, 1>;
using RefRS = ref::Store<NP, 1>;

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

// the five kinds of wz_split_main.cpp, then the planted ones:
// PLANT_LO / PLANT_HI: a core spread evenly over +-w and `arg` samples 8-8.5 w
//   out on one side.  One such sample among 128 already lifts 1.5 sd to
//   1.5 sqrt(1/3 + 64/128) w = 1.37 w, past the core, and 20 among 65 leave it
//   near 5.6 w, short of the planted ones: the first clamp iteration takes
//   exactly `arg` samples at that end and none at the other;
// KEPT: `arg` samples present, every other one missing (0);
// FLAT: one value in every frame.
enum Kind { RECIPE, ZEROS, TIES, CONSTANT, HEAVY, PLANT_LO, PLANT_HI, KEPT, FLAT };

void make_column(Rng &r, Kind kind, int n, int arg, bool u16, float *col) {
    const double level = 0.05 + 0.02 * r.uni();
    for (int f = 0; f < n; f++) {
        double x = level + 0.005 * r.normal();
        if (kind == HEAVY) {                       // Cauchy tails
            x = level + 0.002 * std::tan(3.141592653589793 * (r.uni() - 0.5));
        } else if (kind == PLANT_LO || kind == PLANT_HI) {
            const double w = 0.005;
            x = level + w * (2.0 * r.uni() - 1.0);
            if (f < arg) x = level + (kind == PLANT_LO ? -1.0 : 1.0) * w * (8.0 + 0.5 * r.uni());
        } else if (kind != FLAT) {
            if (r.uni() < 0.01) x += 0.2 + 0.4 * r.uni();      // cosmic ray
            if (r.uni() < 0.001) x *= 0.1;                     // cold pixel
        }
        if (kind == TIES) x = std::round(x * 512.0) / 512.0;
        if (kind == CONSTANT || kind == FLAT) x = level;
        x = x < 1e-6 ? 1e-6 : (x > 1.0 ? 1.0 : x);
        col[f] = (float)x;
        if (kind == ZEROS && r.uni() < 0.2) col[f] = 0.f;
        if (kind == KEPT && f >= arg) col[f] = 0.f;
        if (u16) col[f] = col[f] == 0.f ? 0.f : (float)(int)std::lround((double)col[f] * 65535.0 + 0.5);
    }
    if (kind == CONSTANT && r.uni() < 0.5) col[(int)(r.uni() * n)] += u16 ? 16000.f : 0.25f;   // one outlier on a flat column
}

// samples a first clamp iteration takes at each end (1.5 sd about the median
// of the whole column, plain double arithmetic: only the exercise checks use it)
void first_clamps(const float *col, int n, int &nl, int &nh) {
    std::vector<double> v;
    for (int f = 0; f < n; f++)
        if (col[f] != 0.f) v.push_back(col[f]);
    nl = nh = 0;
    const int m = (int)v.size();
    if (m < 2) return;
    std::vector<double> s = v;
    for (int i = 1; i < m; i++)
        for (int j = i; j > 0 && s[j] < s[j - 1]; j--) std::swap(s[j], s[j - 1]);
    const double med = (m & 1) ? s[m / 2] : 0.5 * (s[m / 2 - 1] + s[m / 2]);
    double mean = 0.0, q = 0.0;
    for (double x : v) mean += x;
    mean /= m;
    for (double x : v) q += (x - mean) * (x - mean);
    const double sd = std::sqrt(q / (m - 1));
    for (double x : v) {
        nl += x < med - 1.5 * sd;
        nh += x > med + 1.5 * sd;
    }
}

struct Family {
    const char *name;
    Kind kind;
    float s0, s1;
    int columns, arg;
    bool u16;
};

struct Tally {
    long long columns = 0, rounds = 0, mismatches = 0, route[3] = {0, 0, 0};
    long long clamps_lo[16] = {0}, clamps_hi[16] = {0};
};

template <int U16>
void run_column(const Family &fam, int n, const float *col, int c, Tally &t) {
    static std::vector<float> ranks((size_t)RS::R * RS::PW);
    float v[NP];
    int kept = 0;
    for (int e = 0; e < NP; e++) {
        float x = f_inf();
        if (e < n && col[e] != 0.f) {
            x = col[e];
            kept++;
        }
        v[e] = x;
    }
    RefRS rr;
    rr.base = ranks.data();
    rr.stride = RS::PW;
    rr.p = 0;
    double W1, W2;
    float c0;
    if (wz_prepare<NP, 1>(v, 0, kept, kept, n, rr, W1, W2, c0)) return;   // kept == 0
    const RS &rs = rr;                                 // the same record, the new fetches
    const int m = NP;                                  // G * E of the one-lane layout
    t.columns++;
    int nl, nh;
    first_clamps(col, n, nl, nh);
    t.clamps_lo[nl < 15 ? nl : 15]++;
    t.clamps_hi[nh < 15 ? nh : 15]++;
    bool bad = false;
    WzConst k0, k1;
    WzState s0, s1;
    PixOut o0, o1;
    std::memset(&s0, 0, sizeof s0);
    std::memset(&s1, 0, sizeof s1);
    std::memset(&o0, 0, sizeof o0);
    std::memset(&o1, 0, sizeof o1);
    int r0 = wz_start<U16>(rr, kept, W1, W2, c0, m, fam.s0, fam.s1, k0, s0, o0);
    int r1 = wz_start<U16>(rs, kept, W1, W2, c0, m, fam.s0, fam.s1, k1, s1, o1);
    if (r0 != r1) bad = true;
    int round = 0;
    if (!bad && r0 == 0) {
        bool more0 = true, more1 = true;
        while (more0) {
            r0 = ref::wz_round<U16>(rr, k0, s0, more0);
            r1 = wz_round<U16>(rs, k1, s1, more1);
            t.rounds++;
            round++;
            if (r0 != r1 || std::memcmp(&s0, &s1, sizeof s0) != 0 || (r0 == 0 && more0 != more1)) {
                bad = true;
                break;
            }
            if (r0) break;
        }
        if (!bad && r0 == 0) {
            r0 = wz_final(rr, k0, s0, o0);
            r1 = wz_final(rs, k1, s1, o1);
        }
    }
    // route as wz_finish maps it
    const int q0 = r0 == 3 ? 0 : r0 == 4 ? 2 : r0, q1 = r1 == 3 ? 0 : r1 == 4 ? 2 : r1;
    if (!bad) {
        bad = q0 != q1;
        if (!bad && q0 == 0)
            bad = std::memcmp(&o0.res, &o1.res, sizeof o0.res) != 0 || o0.rl != o1.rl || o0.rh != o1.rh ||
                  o0.nkept != o1.nkept || std::memcmp(&o0.pmin, &o1.pmin, sizeof(float)) != 0 ||
                  std::memcmp(&o0.pmax, &o1.pmax, sizeof(float)) != 0;
    }
    // and the one-call form the kernels run
    if (!bad) {
        PixOut o2;
        std::memset(&o2, 0, sizeof o2);
        const int q2 = wz_finish<U16>(rs, kept, W1, W2, c0, m, fam.s0, fam.s1, o2);
        bad = q2 != q0 || (q0 == 0 && (std::memcmp(&o0.res, &o2.res, sizeof o0.res) != 0 || o0.rl != o2.rl ||
                                       o0.rh != o2.rh || o0.nkept != o2.nkept));
    }
    if (q0 >= 0 && q0 < 3) t.route[q0]++;
    if (bad && t.mismatches++ < 5)
        std::fprintf(stderr, "MISMATCH %s N %d column %d round %d: rc %d / %d\n", fam.name, n, c, round, r0, r1);
}

Tally run_family(const Family &fam, int n, uint64_t seed) {
    Tally t;
    Rng rng(seed);
    float col[NP];
    for (int c = 0; c < fam.columns; c++) {
        make_column(rng, fam.kind, n, fam.arg, fam.u16, col);
        if (fam.u16) run_column<1>(fam, n, col, c, t);
        else run_column<0>(fam, n, col, c, t);
    }
    return t;
}

}  // namespace

int main() {
    const Family fams[] = {
        // the 14 families of wz_split_main.cpp (its N replaced by the loop below)
        {"recipe s3/3", RECIPE, 3.f, 3.f, 512, 0, false},     {"recipe s3/3 b", RECIPE, 3.f, 3.f, 512, 0, false},
        {"recipe s3/3 c", RECIPE, 3.f, 3.f, 1024, 0, false},   {"recipe s3/3 d", RECIPE, 3.f, 3.f, 512, 0, false},
        {"recipe s2/2", RECIPE, 2.f, 2.f, 1024, 0, false},     {"recipe s2/2 b", RECIPE, 2.f, 2.f, 512, 0, false},
        {"recipe s1.5/2", RECIPE, 1.5f, 2.f, 512, 0, false},  {"zeros s3/3", ZEROS, 3.f, 3.f, 512, 0, false},
        {"zeros s2/2", ZEROS, 2.f, 2.f, 512, 0, false},       {"ties s3/3", TIES, 3.f, 3.f, 512, 0, false},
        {"ties s2/2", TIES, 2.f, 2.f, 512, 0, false},         {"constant s3/3", CONSTANT, 3.f, 3.f, 512, 0, false},
        {"heavy s3/3", HEAVY, 3.f, 3.f, 512, 0, false},       {"heavy s1.5/2", HEAVY, 1.5f, 2.f, 512, 0, false},
        // 1, 2, 3, 4, 5 and 9 clamped samples at one end in one iteration (K - 1, K, K + 1 and
        // 2K + 1 for the trips of K = 2 and 4 samples that were tried)
        {"plant lo 1", PLANT_LO, 3.f, 3.f, 128, 1, false},     {"plant lo 2", PLANT_LO, 3.f, 3.f, 128, 2, false},
        {"plant lo 3", PLANT_LO, 3.f, 3.f, 128, 3, false},     {"plant lo 4", PLANT_LO, 3.f, 3.f, 128, 4, false},
        {"plant lo 5", PLANT_LO, 3.f, 3.f, 128, 5, false},     {"plant lo 9", PLANT_LO, 3.f, 3.f, 128, 9, false},
        {"plant hi 1", PLANT_HI, 3.f, 3.f, 128, 1, false},     {"plant hi 2", PLANT_HI, 3.f, 3.f, 128, 2, false},
        {"plant hi 3", PLANT_HI, 3.f, 3.f, 128, 3, false},     {"plant hi 4", PLANT_HI, 3.f, 3.f, 128, 4, false},
        {"plant hi 5", PLANT_HI, 3.f, 3.f, 128, 5, false},     {"plant hi 9", PLANT_HI, 3.f, 3.f, 128, 9, false},
        // the walk leaves the stored end region
        {"plant lo 16", PLANT_LO, 3.f, 3.f, 128, 16, false},   {"plant lo 17", PLANT_LO, 3.f, 3.f, 128, 17, false},
        {"plant lo 20", PLANT_LO, 3.f, 3.f, 128, 20, false},   {"plant hi 16", PLANT_HI, 3.f, 3.f, 128, 16, false},
        {"plant hi 17", PLANT_HI, 3.f, 3.f, 128, 17, false},   {"plant hi 20", PLANT_HI, 3.f, 3.f, 128, 20, false},
        // small and region-overlapping kept (zero samples are missing)
        {"kept 1", KEPT, 3.f, 3.f, 64, 1, false},              {"kept 2", KEPT, 3.f, 3.f, 128, 2, false},
        {"kept 3", KEPT, 3.f, 3.f, 128, 3, false},             {"kept 39", KEPT, 3.f, 3.f, 256, 39, false},
        {"kept 40", KEPT, 3.f, 3.f, 256, 40, false},           {"kept 41", KEPT, 3.f, 3.f, 256, 41, false},
        {"kept 39 s1.5/2", KEPT, 1.5f, 2.f, 256, 39, false},   {"kept 41 s1.5/2", KEPT, 1.5f, 2.f, 256, 41, false},
        {"flat", FLAT, 3.f, 3.f, 64, 0, false},
        // 16-bit columns
        {"u16 recipe s3/3", RECIPE, 3.f, 3.f, 1024, 0, true},  {"u16 recipe s2/2", RECIPE, 2.f, 2.f, 512, 0, true},
        {"u16 zeros s3/3", ZEROS, 3.f, 3.f, 512, 0, true},    {"u16 ties s2/2", TIES, 2.f, 2.f, 512, 0, true},
        {"u16 constant", CONSTANT, 3.f, 3.f, 512, 0, true},    {"u16 heavy s1.5/2", HEAVY, 1.5f, 2.f, 512, 0, true},
        {"u16 plant lo 5", PLANT_LO, 3.f, 3.f, 128, 5, true},  {"u16 plant hi 9", PLANT_HI, 3.f, 3.f, 128, 9, true},
        {"u16 plant hi 17", PLANT_HI, 3.f, 3.f, 128, 17, true}, {"u16 kept 40", KEPT, 3.f, 3.f, 128, 40, true},
        {"u16 flat", FLAT, 3.f, 3.f, 64, 0, true},
    };
    const int ns[] = {65, 100, 128};
    long long bad = 0, total = 0, rounds = 0;
    int fail = 0;
    for (int n : ns) {
        int fi = 0;
        for (const Family &f : fams) {
            const Tally t = run_family(f, n, 20261019ull + 1000ull * (uint64_t)fi++ + (uint64_t)n);
            std::printf("N %3d  %-18s columns %5lld  rounds %6lld  routes %5lld / %4lld / %4lld  mismatches %lld\n", n,
                        f.name, t.columns, t.rounds, t.route[0], t.route[1], t.route[2], t.mismatches);
            bad += t.mismatches;
            total += t.columns;
            rounds += t.rounds;
            // exercise checks: the planted cases must be the ones the program names
            if (f.kind == PLANT_LO || f.kind == PLANT_HI) {
                const long long *h = f.kind == PLANT_LO ? t.clamps_lo : t.clamps_hi;
                if (f.arg < 15 && h[f.arg] != t.columns) {
                    std::fprintf(stderr, "FAIL: %s N %d: %lld of %lld columns clamp %d samples at that end\n", f.name, n,
                                 h[f.arg], t.columns, f.arg);
                    fail = 1;
                }
                if (f.arg >= 16 && t.route[1] != t.columns) {
                    std::fprintf(stderr, "FAIL: %s N %d: %lld of %lld columns leave the stored ranks\n", f.name, n,
                                 t.route[1], t.columns);
                    fail = 1;
                }
                if (f.arg <= 5 && t.route[0] == 0) {   // (nine planted and the core's own tail: past the 16 stored ranks)
                    std::fprintf(stderr, "FAIL: %s N %d: no column ends on the moment path\n", f.name, n);
                    fail = 1;
                }
            }
            if ((f.kind == KEPT || f.kind == FLAT) && t.columns != f.columns) {
                std::fprintf(stderr, "FAIL: %s N %d: %lld of %d columns ran\n", f.name, n, t.columns, f.columns);
                fail = 1;
            }
            if (f.kind == RECIPE && t.route[0] == 0) {
                std::fprintf(stderr, "FAIL: %s N %d: no column ends on the moment path\n", f.name, n);
                fail = 1;
            }
        }
    }
    std::printf("columns %lld  rounds %lld  mismatches %lld\n", total, rounds, bad);
    if (bad) {
        std::fprintf(stderr, "FAIL: %lld columns differ from the reference rounds\n", bad);
        fail = 1;
    }
    if (!fail) std::printf("wz_walk ok\n");
    return fail;
}

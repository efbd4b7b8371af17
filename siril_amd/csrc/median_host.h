// median_host.h -- the median filter (`fmedian ksize modulation`; DESIGN.md
// 6l, M0-M5) as it is shared by the kernels (median.hip), the C-ABI's host
// side and a stand-alone program (tests/hostsim/fmedian_host_main.cpp): the
// refusals, the conversion, the reference median of one window, the
// modulation, and the selection networks.  Plain C++ unless compiled by hipcc,
// where the arithmetic and the networks are __host__ __device__.
//
// The order is the key order of bkg_host.h (bkg_key / bkg_unkey), the
// reflection and the conversion are those of wavelet_host.h; nothing of them
// is restated here.  The networks are templates over the compare-exchange
// operation, so that a host program can run them on other types (uint64_t
// words of 64 zero-one inputs under AND / OR: the 0-1 principle).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bkg_host.h"
#include "wavelet_host.h"

#if defined(__HIPCC__)
#define SGPU_MED_HD __host__ __device__
#else
#define SGPU_MED_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define SGPU_MED_UNROLL _Pragma("unroll")
#else
#define SGPU_MED_UNROLL
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sgpu_med_host {

constexpr int MED_MIN_KSIZE = 3, MED_MAX_KSIZE = 15, MED_MAX_ITER = 8;

// ---- M0 ----
SGPU_MED_HD inline uint32_t med_key(float v) { return sgpu_bkg_host::bkg_key(v); }
SGPU_MED_HD inline float med_unkey(uint32_t k) { return sgpu_bkg_host::bkg_unkey(k); }
SGPU_MED_HD inline uint32_t med_key_of(float v) { return med_key(v); }
SGPU_MED_HD inline uint32_t med_key_of(uint16_t v) { return med_key(sgpu_wav_host::wav_to_float(v)); }

// ---- M1 ----
SGPU_MED_HD inline int med_radius(int ksize) { return (ksize - 1) / 2; }
SGPU_MED_HD inline int med_rank(int ksize) { return (ksize * ksize - 1) / 2; }

// ---- M5: nullptr, or what is refused ----
inline const char *med_check(int W, int H, int ksize, float modulation, int iterations) {
    if (W < 1 || H < 1) return "fmedian: empty plane";
    if (W > 65535 || H > 65535) return "fmedian: the plane is too large";
    if (ksize < MED_MIN_KSIZE || ksize > MED_MAX_KSIZE || ksize % 2 == 0) return "fmedian: ksize must be odd, 3 .. 15";
    if (med_radius(ksize) > (W < H ? W : H) - 1) return "fmedian: the plane is too small for that window";
    if (!sgpu_wav_host::wav_finite(modulation) || !(modulation >= 0.0f && modulation <= 1.0f))
        return "fmedian: modulation must be in [0, 1]";
    if (iterations < 1 || iterations > MED_MAX_ITER) return "fmedian: iterations must be 1 .. 8";
    return nullptr;
}

// ---- M3: m is the median, x the sample it replaces ----
SGPU_MED_HD inline float med_modulate(float modulation, float m, float x) {
    if (modulation == 1.0f) return m;
    const float keep = 1.0f - modulation;
    const float a = modulation * m;
    const float b = keep * x;
    return a + b;
}

// ---- the networks ----
// Op::lo(a, b) / Op::hi(a, b) are the two halves of a compare-exchange.
struct MedKeyOp {
    SGPU_MED_HD static uint32_t lo(uint32_t a, uint32_t b) { return a < b ? a : b; }
    SGPU_MED_HD static uint32_t hi(uint32_t a, uint32_t b) { return a < b ? b : a; }
};

template <class Op, class T>
SGPU_MED_HD inline void med_cx(T &a, T &b) {
    const T l = Op::lo(a, b), h = Op::hi(a, b);
    a = l, b = h;
}

// ascending sort of v[0 .. N) by odd-even transposition: N rounds
template <class Op, int N, class T>
SGPU_MED_HD inline void med_sort(T (&v)[N]) {
    SGPU_MED_UNROLL
    for (int r = 0; r < N; r++) {
        SGPU_MED_UNROLL
        for (int i = r & 1; i + 1 < N; i += 2) med_cx<Op>(v[i], v[i + 1]);
    }
}

// the smallest of v[0 .. m) to v[0], the largest to v[m - 1]
template <class Op, int N, class T>
SGPU_MED_HD inline void med_ends(T (&v)[N], int m) {
    SGPU_MED_UNROLL
    for (int i = 0; i < N / 2; i++)
        if (i < m - 1 - i) med_cx<Op>(v[i], v[m - 1 - i]);
    const int half = (m + 1) / 2;       // the lower parts (and the middle one) are v[0 .. half), the upper v[m - half .. m)
    SGPU_MED_UNROLL
    for (int i = 1; i < N; i++)
        if (i < half) med_cx<Op>(v[0], v[i]);
    SGPU_MED_UNROLL
    for (int i = N - 2; i >= 0; i--)
        if (i >= m - half && i < m - 1) med_cx<Op>(v[i], v[m - 1]);
}

// The median of c[0 .. NC), NC odd, by forgetful selection: of NC/2 + 2 values neither the smallest nor the
// largest can be the median of all NC, so both are dropped and the next value joins, down to three.
template <class Op, int NC, class T>
SGPU_MED_HD inline T med_select(const T (&c)[NC]) {
    static_assert(NC % 2 == 1 && NC >= 3, "an odd number of candidates");
    constexpr int M = NC / 2 + 2;
    T w[M];
    SGPU_MED_UNROLL
    for (int i = 0; i < M; i++) w[i] = c[i];
    SGPU_MED_UNROLL
    for (int m = M; m > 3; m--) {
        med_ends<Op, M>(w, m);
        w[0] = c[M + (M - m)];      // w[0] and w[m - 1] leave; the next candidate takes w[0]'s place
    }
    med_ends<Op, M>(w, 3);
    return w[1];
}

// In a K x K window whose rows and columns are both sorted, (row a, column b) has (a+1)(b+1) - 1 values not above
// it and (K-a)(K-b) - 1 not below it: it can be the median only if neither count exceeds the median's rank.
SGPU_MED_HD constexpr bool med_candidate(int K, int a, int b) {
    return (a + 1) * (b + 1) <= (K * K + 1) / 2 && (K - a) * (K - b) <= (K * K + 1) / 2;
}
SGPU_MED_HD constexpr int med_ncandidates(int K) {
    int n = 0;
    for (int a = 0; a < K; a++)
        for (int b = 0; b < K; b++) n += med_candidate(K, a, b);
    return n;
}

// The median of K x K values given as K columns, each sorted ascending (col[j][i], i the rank within column j).
// Sorting every rank's row keeps the columns sorted; then (a, b) has (a+1)(b+1) - 1 values not above it and
// (K-a)(K-b) - 1 not below it, which leaves med_ncandidates(K) places where the median can be, as many ruled out
// below as above, and the median of all is the median of those.
template <class Op, int K, class T>
SGPU_MED_HD inline T med_of_sorted_columns(const T (&col)[K][K]) {
    constexpr int NC = med_ncandidates(K);
    T cand[NC];
    int n = 0;
    SGPU_MED_UNROLL
    for (int a = 0; a < K; a++) {
        T row[K];
        SGPU_MED_UNROLL
        for (int b = 0; b < K; b++) row[b] = col[b][a];
        med_sort<Op, K>(row);
        SGPU_MED_UNROLL
        for (int b = 0; b < K; b++)
            if (med_candidate(K, a, b)) cand[n++] = row[b];
    }
    return med_select<Op, NC>(cand);
}

// The whole K x K network on a window in any order, v[row * K + column]: what the kernels do, without the sharing
// of sorted columns between neighbouring outputs.
template <class Op, int K, class T>
SGPU_MED_HD inline T med_network(const T (&v)[K * K]) {
    T col[K][K];
    SGPU_MED_UNROLL
    for (int j = 0; j < K; j++) {
        SGPU_MED_UNROLL
        for (int i = 0; i < K; i++) col[j][i] = v[i * K + j];
        med_sort<Op, K>(col[j]);
    }
    return med_of_sorted_columns<Op, K>(col);
}

// ---- host restatements (the stand-alone program) ----

// M1, M2: the median's key of the window around (x, y) of a float plane
inline uint32_t med_window_ref(const float *plane, int W, int H, int x, int y, int ksize, std::vector<uint32_t> &keys) {
    const int r = med_radius(ksize);
    keys.clear();
    for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++)
            keys.push_back(med_key(plane[(size_t)sgpu_wav_host::wav_refl(y + dy, H) * W + sgpu_wav_host::wav_refl(x + dx, W)]));
    std::nth_element(keys.begin(), keys.begin() + med_rank(ksize), keys.end());
    return keys[med_rank(ksize)];
}

// M0-M4 of one plane
template <typename T>
inline void med_filter_host(const T *in, int W, int H, int ksize, float modulation, int iterations, float *out) {
    const size_t np = (size_t)W * H;
    std::vector<float> y(np), next(np);
    std::vector<uint32_t> keys;
    for (size_t i = 0; i < np; i++) y[i] = sgpu_wav_host::wav_to_float(in[i]);
    for (int t = 0; t < iterations; t++) {
        for (int py = 0; py < H; py++)
            for (int px = 0; px < W; px++)
                next[(size_t)py * W + px] = med_modulate(
                    modulation, med_unkey(med_window_ref(y.data(), W, H, px, py, ksize, keys)), y[(size_t)py * W + px]);
        y.swap(next);
    }
    for (size_t i = 0; i < np; i++) out[i] = y[i];
}

}  // namespace sgpu_med_host

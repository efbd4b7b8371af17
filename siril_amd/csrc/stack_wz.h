// stack_wz.h -- WINSORIZED (float) stack on moments: the column lives in
// registers only for the gather, the sort and ONE pass; every rejection round
// after that is scalar work on the window's moments plus reads of a few ranks
// from an LDS copy of the sorted column's ends and middle.
//
// Why: the reference (rejection_float.c:223-259) runs, per round, an sd pass
// pair, a quickselect median, and per clamp iteration two more O(N) passes
// (siril_stats_float_sd of w_stack); the register-resident sorted path
// (stack_sorted_impl.h) still pays a median select, a fill pass, two sd
// passes, a count pass per round and two passes per iteration.  Here:
//   * ranks: the sorted column's low KT, middle KM and high KT ranks go to
//     LDS (RankStore); medians, tail samples, clip candidates and the window
//     ends are single LDS reads;
//   * moments: W1 = sum (x - c0), W2 = sum (x - c0)^2 over the window (one
//     f64 pass, c0 the first median); a round's clipped samples are
//     subtracted, the clamped tails of an iteration are taken out of them
//     (the samples below L / above U are a prefix / suffix of the window);
//   * sigma: every sd the reference computes -- the round's first sd and the
//     1.134 sd of each clamp iteration -- is known from the moments up to the
//     reference's own float rounding, so it is carried as an interval that
//     provably holds the reference's float (var_bounds below); the stop test
//     and the final clip must have one outcome over the intervals;
//   * mean: sum x = W1 + n c0, exact whenever the sum-order guard proves the
//     window's sums exact, else checked for float stability.
// DATA_USHORT columns (apply_rejection_ushort, median_and_mean.c:831-860; U16
// template flag): the same path on the WORD samples held as exact floats.
// The differences are the ones the 16-bit sorted path has: the Winsorize
// bounds are roundf_to_WORD(median -/+ 1.5 sigma) (:840-841; monotone, so
// the sigma interval maps to integer bound intervals), a first median of 0
// leaves no sample (:747-756: the exact kernel takes the pixel), the sd is
// siril_stats_ushort_sd_32 (statistics.c:115-127: the float-path formula on
// integers) and the mean is the exact integer sum over kept (:1020-1034).
// Any undecidable step, or a rank outside the stored ranges, sends the pixel
// to the register-resident kernel (second launch over the list fb2_list),
// whose own deferrals go to the exact sequential kernel as before.  So every
// pixel's result is the one the sorted path -- i.e. the reference -- gives.
#pragma once
#include "stack_sorted_impl.h"

// Ranks stored per end (KT) and around the median (KM) at N <= 128.  Sized
// from the ranks the rounds visit (scripts/wzstat on the benchmark recipe:
// depth from an end p50 / p99 / p99.9 = 7 / 13-14 / 15-16, from the middle
// 1 / 3 / 4; 16 / 8 hold every read of 99.5 % of the moment-path pixels) so
// that the rounds kernel can stage a wave's records in LDS (R = 40 slots,
// 10 KB per wave, 4 waves / SIMD): config 2 13.65 -> 12.78 ms with the LDS
// rounds (24 / 16 with global reads: 13.65; 16 / 8 with global reads: 14.35,
// the extra fallbacks unpaid; profiles/r05r_ab_*.log)
#ifndef SGPU_WZ_KT
#define SGPU_WZ_KT 16
#endif
#ifndef SGPU_WZ_KM
#define SGPU_WZ_KM 8
#endif
// Ranks per end of the fused form (k_stack_wz_fused1 and the tail passes that
// read what it leaves): its record lives in LDS, where 20 + 8 + 20 = 48 slots
// are 12 KB per wave, 48 KB per block, three blocks in a CU's 160 KB -- the
// occupancy the registers allow anyway -- so the deeper record costs no HBM
// traffic, and about half of the pixels that went to the sorted kernel
// because a walk left 16 ranks stay on the moment path (host counts on the
// benchmark recipe, sigma 3/3: route 1 at depth 16 / 18 / 20 = 0.73 / 0.38 /
// 0.34 % of the pixels; what is left are undecidable steps).  The two-kernel
// forms keep SGPU_WZ_KT: their record is HBM traffic.  (16: the parent's
// record, A/B.)
// The buckets whose kernel fits four waves per SIMD in registers (real-slot
// bound <= 88 at the parent of this change: at most 128 VGPRs) keep 16: four
// blocks of 40 KB are exactly the CU's LDS, and 48 KB tiles would cost them
// the fourth wave (no bench config runs there; not measured).  (With the LDS
// sized by the launch the unshifted RSL = 88 kernel compiles to 131 VGPRs,
// three waves: profiles/r13_wz_depth_kernel_resources.txt.)
#ifndef SGPU_WZ_KT_FUSED
#define SGPU_WZ_KT_FUSED 20
#endif
namespace sgpu {
constexpr int wz_fused_kt(int rsl) { return rsl < kWzDeepMinFrames ? SGPU_WZ_KT : SGPU_WZ_KT_FUSED; }
}
// instrumentation hook of the host statistics tool (scripts/wzstat): empty in
// every product build
#ifndef SGPU_WZ_TRACE
#define SGPU_WZ_TRACE(ev) ((void)0)
#endif

namespace sgpu {

SG_HD unsigned umul24(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}

// sqrtf bounds: RN(sqrt(x)) lies in [sqrt_lo(x), sqrt_hi(x)] (the device's
// v_sqrt_f32 is within 1 ulp; the neighbours of its result bracket the
// correctly rounded root; zero stays exact)
SG_HD float fnext(float r) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, r) + 1u); }
SG_HD float fprev(float r) { return r > 0.f ? __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, r) - 1u) : 0.f; }
SG_HD float fsqrt_raw(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}
SG_HD float sqrt_lo(float x) { return x < 0x1p-100f ? 0.f : fprev(fsqrt_raw(x)); }
SG_HD float sqrt_hi(float x) { return x == 0.f ? 0.f : (x < 0x1p-100f ? 0x1p-49f : fnext(fsqrt_raw(x))); }

// sigma_clipping_float's candidates (rejection_float.c:49-60) for a sigma
// known only to lie in an interval: thresholds tl in [tl0, tl1], th in
// [th0, th1].  Low candidates (mf - x > tl) are a prefix of the sorted window
// and high ones (x - mf > th) a suffix, so they are counted by walking the
// stored ranks from each end under the larger thresholds; the first sample
// that is not a candidate there must not be one under the smaller ones
// either.  Returns 0 (cl / ch set), 1 ambiguous, 2 a walk left the stored
// ranks (count with passes instead).
template <class TS>
SG_HD int wz_clip_counts(const TS &ts, int lo, int hi, float mf, float tl0, float th0, float tl1, float th1,
                         int &cl, int &ch) {
    float x;
    int k = 0;
    for (;;) {
        if (lo + k >= hi || !ts.fetch_lo(lo + k, x)) return 2;
        if (!(mf - x > tl1)) break;
        k++;
    }
    if (mf - x > tl0) return 1;
    cl = k;
    k = 0;
    for (;;) {
        if (hi - 1 - k < lo + cl || !ts.fetch_hi(hi - 1 - k, x)) return 2;
        if (!(x - mf > th1)) break;
        k++;
    }
    if (x - mf > th0) return 1;
    ch = k;
    return 0;
}

// Ranks kept per pixel: [0, KT), [mid0, mid0 + KM) around kept/2 and
// [kept - KT, kept).  LDS layout [rank slot][pixel of the wave]: the wave's
// pixels read consecutive words (no bank conflicts).  KTP: the depth per end
// at NP <= 128 (R, the regions, the fetches and the compact copies follow it).
template <int NP, int G, int KTP = SGPU_WZ_KT>
struct RankStore {
    static constexpr int E = NP / G;
    static constexpr int PW = 64 / G;                      // pixels per wave
    static constexpr int KT = NP <= 128 ? KTP : NP / 4;   // ranks per end
    static constexpr int KM = NP <= 128 ? SGPU_WZ_KM : 16; // ranks around the median
    static constexpr int R = 2 * KT + KM;                  // slots per pixel
    float *base;                                           // rank slot j of this pixel at base[j * stride + p]
    long long stride, p;                                   // LDS: the wave's pixels; global: the launch's
    int kept, mid0, mid1, hi0;                             // stored: [0, KT), [mid0, mid1), [hi0, kept)
    // stores the interleaved sorted column (lane g, slot e = rank e*G + g);
    // the slot loops cover the wave's range of `kept` (kmin..kmax, uniform),
    // the rank tests are per pixel
    SG_HD void store(const float (&v)[E], int g, int kmin, int kmax) {
        mid0 = kept / 2 - KM / 2;
        hi0 = kept - KT;
        hi0 = hi0 < 0 ? 0 : hi0;
        const int eh0 = (kmin - KT) / G - 1, eln = (kmax + G - 1) / G;
        const int em0 = (kmin / 2 - KM / 2) / G - 1, em1 = (kmax / 2 + KM / 2) / G + 1;
        // what the slot loops can reach of this pixel's ranges
        hi0 = hi0 > eh0 * G ? hi0 : (eh0 > 0 ? eh0 * G : 0);
        mid1 = mid0 + KM < (em1 + 1) * G ? mid0 + KM : (em1 + 1) * G;
        mid0 = mid0 > em0 * G ? mid0 : em0 * G;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int r = e * G + g;
            if (e < (KT + G - 1) / G) {
                if (r < KT && r < kept) base[r * stride + p] = v[e];
            }
            if (e >= eh0 && e < eln) {
                if (r >= hi0 && r < kept) base[(KT + KM + r - (kept - KT)) * stride + p] = v[e];
            }
            if (e >= em0 && e <= em1) {
                if (r >= mid0 && r < mid1 && r < kept) base[(KT + r - (kept / 2 - KM / 2)) * stride + p] = v[e];
            }
        }
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
    }
    // The same store into the HBM record of the prep kernel, with the rank
    // tests moved into buffer descriptors: one raw-buffer descriptor per
    // region (low [0, KT), middle [KT, KT + KM), high [KT + KM, R)), whose
    // record count is the region's size, and a per-lane 32-bit byte offset
    // (the pixel's column + the rank's slot within the region, wrapping
    // modulo 2^32 when the slot is negative).  A rank outside its region --
    // below it (a huge unsigned offset) or above it -- is past the record
    // count, and the hardware drops the store; so every slot of the
    // wave-uniform loops is stored unconditionally: one 32-bit add per store
    // instead of a 64-bit multiply, a compare and an exec-mask branch.  The
    // regions then hold exactly what store() puts there (plus +Inf in slots of
    // ranks >= kept, which fetch never reads).  Needs NP * stride * 4 <=
    // 2^32 (negative slots >= -NP stay above the record count), which the
    // launcher enforces (stack_wz_launch.h).  (Host builds, tests/hostsim:
    // the descriptor's range check restated per store -- drop().)
    SG_HD void drop(int region0, int size, int slot, float x) {
        if (slot >= 0 && slot < size) base[(long long)(region0 + slot) * stride + p] = x;
    }
    SG_HD void store_buf(const float (&v)[E], int g, int kmin, int kmax) {
        mid0 = kept / 2 - KM / 2;
        hi0 = kept - KT;
        hi0 = hi0 < 0 ? 0 : hi0;
        const int eh0 = (kmin - KT) / G - 1, eln = (kmax + G - 1) / G;
        const int em0 = (kmin / 2 - KM / 2) / G - 1, em1 = (kmax / 2 + KM / 2) / G + 1;
        hi0 = hi0 > eh0 * G ? hi0 : (eh0 > 0 ? eh0 * G : 0);
        mid1 = mid0 + KM < (em1 + 1) * G ? mid0 + KM : (em1 + 1) * G;
        mid0 = mid0 > em0 * G ? mid0 : em0 * G;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t S4 = (uint32_t)stride * 4u;
        const uint32_t pb = (uint32_t)p * 4u;
        const auto rlo = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)((uint32_t)KT * S4), 0x00020000);
        const auto rmid = __builtin_amdgcn_make_buffer_rsrc(base + (long long)KT * stride, (short)0,
                                                            (int)((uint32_t)KM * S4), 0x00020000);
        const auto rhi = __builtin_amdgcn_make_buffer_rsrc(base + (long long)(KT + KM) * stride, (short)0,
                                                           (int)((uint32_t)KT * S4), 0x00020000);
        const uint32_t blo = pb + (uint32_t)g * S4;
        const uint32_t bhi = pb + (uint32_t)(g + KT - kept) * S4;
        const uint32_t bmid = pb + (uint32_t)(g - (kept / 2 - KM / 2)) * S4;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t eo = (uint32_t)(e * G) * S4;
            const uint32_t x = __builtin_bit_cast(uint32_t, v[e]);     // the b32 store takes the bits
            if (e < (KT + G - 1) / G) __builtin_amdgcn_raw_buffer_store_b32(x, rlo, (int)(blo + eo), 0, 0);
            if (e >= eh0 && e < eln) __builtin_amdgcn_raw_buffer_store_b32(x, rhi, (int)(bhi + eo), 0, 0);
            if (e >= em0 && e <= em1) __builtin_amdgcn_raw_buffer_store_b32(x, rmid, (int)(bmid + eo), 0, 0);
        }
#else
        for (int e = 0; e < E; e++) {
            const int r = e * G + g;
            if (e < (KT + G - 1) / G) drop(0, KT, r, v[e]);
            if (e >= eh0 && e < eln) drop(KT + KM, KT, r + KT - kept, v[e]);
            if (e >= em0 && e <= em1) drop(KT, KM, r - (kept / 2 - KM / 2), v[e]);
        }
#endif
    }
    // store_buf for a sorted column in one lane (G = 1, slot = rank) whose
    // wave has kept in [RSL - 7, RSL] in every lane: the slots that can hold
    // a rank of the high region, [RSL - 7 - KT, RSL), and of the middle one,
    // [(RSL - 7) / 2 - KM / 2, RSL / 2 + KM / 2), are compile-time supersets
    // of every lane's ranges, so the stores stand in a straight line; a slot
    // outside the lane's own range falls outside the region (offsets -7 ..
    // KT + 6 and -4 .. 11 slots: no wrap back into it) and is dropped as in
    // store_buf.  Every rank of the three ranges is stored, so hi0 / mid0 /
    // mid1 are the unclipped ones -- what store() leaves for this wave.
    template <int RSL>
    SG_HD void store_full(const float (&v)[E]) {
        static_assert(G == 1 && RSL % 8 == 0 && RSL - 7 - KT >= KT && RSL <= E, "one lane per pixel, N >= 65");
        mid0 = kept / 2 - KM / 2;
        mid1 = mid0 + KM;
        hi0 = kept - KT;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t S4 = (uint32_t)stride * 4u;
        const uint32_t pb = (uint32_t)p * 4u;
        const auto rlo = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)((uint32_t)KT * S4), 0x00020000);
        const auto rmid = __builtin_amdgcn_make_buffer_rsrc(base + (long long)KT * stride, (short)0,
                                                            (int)((uint32_t)KM * S4), 0x00020000);
        const auto rhi = __builtin_amdgcn_make_buffer_rsrc(base + (long long)(KT + KM) * stride, (short)0,
                                                           (int)((uint32_t)KT * S4), 0x00020000);
        const uint32_t bhi = pb + (uint32_t)(KT - kept) * S4;
        const uint32_t bmid = pb - (uint32_t)mid0 * S4;
#pragma unroll
        for (int e = 0; e < KT; e++)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v[e]), rlo, (int)(pb + (uint32_t)e * S4), 0, 0);
#pragma unroll
        for (int e = RSL / 2 - 4 - KM / 2; e < RSL / 2 + KM / 2; e++)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v[e]), rmid, (int)(bmid + (uint32_t)e * S4), 0, 0);
#pragma unroll
        for (int e = RSL - 7 - KT; e < RSL; e++)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v[e]), rhi, (int)(bhi + (uint32_t)e * S4), 0, 0);
#else
        for (int e = 0; e < KT; e++) drop(0, KT, e, v[e]);
        for (int e = RSL / 2 - 4 - KM / 2; e < RSL / 2 + KM / 2; e++) drop(KT, KM, e - mid0, v[e]);
        for (int e = RSL - 7 - KT; e < RSL; e++) drop(KT + KM, KT, e + KT - kept, v[e]);
#endif
    }
    // store_full into an LDS tile (the fused kernel, k_stack_wz_fused1): LDS
    // has no descriptor to drop a store, so the order does it.  Same
    // compile-time slot ranges; a slot below its lane's range lands in the
    // region underneath (at most 7 slots under the high one: the middle
    // region; 4 under the middle one: the low region), which is stored
    // afterwards and whole by every lane (kept >= RSL - 7 >= KT + KM: every
    // rank of the middle and low regions exists).  Only a slot above the range
    // needs its test: ranks >= kept (the last 7 slots) and the last 4 middle
    // slots.  LDS stores of a lane complete in program order.  Leaves the
    // tile's R slots and hi0 / mid0 / mid1 as store_full leaves the record's.
    // The depth KT moves none of this.  With kept in [RSL - 7, RSL]:
    //   high    slots [RSL - 7 - KT, RSL), KT + 7 stores (27 at KT = 20, 23 at
    //           16); slot e goes to tile row KT + KM + e - hi0, hi0 = kept - KT
    //           in [RSL - 7 - KT, RSL - KT], so e - hi0 >= -7: at worst the
    //           middle region's last 7 rows (KM >= 7), never the low region;
    //   middle  slots [RSL / 2 - 4 - KM / 2, RSL / 2 + KM / 2), KM + 4 = 12
    //           stores; row KT + e - mid0, mid0 = kept / 2 - KM / 2 >= RSL / 2
    //           - 4 - KM / 2, so e - mid0 >= -4: the low region's last 4 rows
    //           (KT >= KM / 2 >= 4);
    //   low     slots [0, KT), stored last and whole, every lane's own ranks.
    // 59 stores at KT = 20 (27 + 12 + 20), 51 at 16.  The high stores read the
    // sorted column's top KT + 7 slots and the low ones its first KT: each
    // sample is read where it already lives until the moments pass, which
    // reads the whole column after them, so a deeper record lengthens no
    // sample's life.
    template <int RSL>
    SG_HD void store_full_lds(const float (&v)[E]) {
        static_assert(G == 1 && RSL % 8 == 0 && RSL - 7 - KT >= KT && RSL <= E, "one lane per pixel, N >= 65");
        static_assert(RSL - 7 >= KT + KM && KM / 2 <= KT && 7 <= KM, "a slot under a region stays inside the next one");
        mid0 = kept / 2 - KM / 2;
        mid1 = mid0 + KM;
        hi0 = kept - KT;
        const int S = (int)stride;
        float *const bl = base + p;
        float *const bh = bl + (KT + KM - hi0) * S;      // rank e of the high region at bh[e * S]
        float *const bm = bl + (KT - mid0) * S;          // of the middle region at bm[e * S]
#pragma unroll
        for (int e = RSL - 7 - KT; e < RSL; e++)
            if (e < RSL - 7 || e < kept) bh[e * S] = v[e];
#pragma unroll
        for (int e = RSL / 2 - 4 - KM / 2; e < RSL / 2 + KM / 2; e++)
            if (e < RSL / 2 || e < mid1) bm[e * S] = v[e];
#pragma unroll
        for (int e = 0; e < KT; e++) bl[e * S] = v[e];
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
    }
    // rank r (0 <= r < kept); false when not stored (the pixel falls back).
    // Branch-free: the slot is selected, one load is issued (slot 0 when the
    // rank is not stored), so the rounds' fetch loops carry no divergent
    // control flow per range test.
    SG_HD bool fetch(int r, float &x) const {
        const bool lo_ok = r < KT && r < kept, hi_ok = r >= hi0 && r < kept, mid_ok = r >= mid0 && r < mid1;
        const int slot = lo_ok ? r : hi_ok ? KT + KM + r - (kept - KT) : KT + r - (kept / 2 - KM / 2);
        const bool ok = lo_ok || hi_ok || mid_ok;
        // slot < R and stride = the chunk's pixels < 2^23 with R * stride <
        // 2^32 (both enforced by the launcher, stack_wz_launch.h): one
        // full-rate 24-bit multiply whose 32-bit product cannot wrap; the
        // pixel's base address is loop-invariant (a 64-bit multiply per fetch
        // was quarter-rate work)
        x = (base + p)[umul24((unsigned)(ok ? slot : 0), (unsigned)stride)];
        return ok;
    }
    // The same for a rank the caller reaches from one end of the window (r >=
    // 0): only that end's region is tested and its slot formula used, one
    // load issued (slot 0 on a miss); a rank outside the region -- past the
    // stored depth, or in another region when they overlap (kept < R) --
    // takes fetch() in a branch a wave rarely enters.  Same value, same
    // answer as fetch() for every r.
    SG_HD bool fetch_lo(int r, float &x) const {
        const bool hit = r < KT && r < kept;
        x = (base + p)[umul24((unsigned)(hit ? r : 0), (unsigned)stride)];
        bool ok = true;
        if (__builtin_expect(!hit, 0)) ok = fetch(r, x);
        return ok;
    }
    SG_HD bool fetch_hi(int r, float &x) const {
        const bool hit = r >= hi0 && r < kept;
        x = (base + p)[umul24((unsigned)(hit ? r + (R - kept) : 0), (unsigned)stride)];
        bool ok = true;
        if (__builtin_expect(!hit, 0)) ok = fetch(r, x);
        return ok;
    }
};

// Bounds of the reference's (float)(vsum / (n - 1)) (siril_stats_float_sd,
// statistics.h:80-106) for the window's samples clamped to [L, U], L in
// [Llo, Lhi], U in [Ulo, Uhi] (no clamp: a = c = 0, widths 0).  R1 / R2:
// moments about c0 of the samples between the clamps at the inner corner
// (Lhi, Ulo); a / c: samples below Lhi / above Ulo; E1 / E2: bounds of the
// absolute f64 errors of R1 / R2.  The argument:
//   * the reference sums fl(fl(w - mean)^2) in f64, mean = (float)(sum w / n);
//     each term is within (1 + u)^3 of (w - mean)^2 (u = 2^-24), the f64 sum
//     within its order bound (sg.c) of the exact one, and
//     sum (w - mean)^2 = V*(L, U) + n (mean - mean*)^2, mean* the exact mean,
//     |mean - mean*| <= half an ulp + the order error of sum w;
//   * V*(L, U) = sum (w - mean*)^2 decreases as L rises or U falls
//     (dV*/dL = 2 a(L) (L - mean*) <= 0): it is smallest at the inner corner,
//     computed here from the moments, and grows by at most
//     2 a |L - mean*| dL + 2 c |U - mean*| dU towards (Llo, Uhi);
//   * every float step after the f64 sum -- the (float) conversion, sqrtf
//     (bracketed by sqrt_lo / sqrt_hi), 1.134f *, 1.5f *, m -+ t, min / max --
//     is monotone, so interval ends map to interval ends.
SG_HD void var_bounds(double R1, double R2, float E1, float E2, int a, int c, int n, float c0, float Llo, float Lhi,
                      float Ulo, float Uhi, bool clamped, float eps, float sgc, double rn, double rn1,
                      float &varlo, float &varhi) {
    const float af = (float)a, cf = (float)c;
    double VA, DA;
    float lAf = 0.f, uAf = 0.f, dL = 0.f, dU = 0.f, wmax;
    if (clamped) {
        const double lA = (double)Lhi - (double)c0, uA = (double)Ulo - (double)c0;
        DA = (double)a * lA + (double)c * uA + R1;
        const double QA = (double)a * (lA * lA) + (double)c * (uA * uA) + R2;
        VA = QA - DA * DA * rn;
        lAf = fabsf((float)lA) * 1.0000002f;
        uAf = fabsf((float)uA) * 1.0000002f;
        // widths of the clamp intervals: fl(Lhi - Llo) <= (1 + 2^-24)(Lhi - Llo)
        // (Lhi >= Llo), so the f32 difference times 1 + 2^-22.3 bounds them
        // from above like the f64 form did
        dL = (Lhi - Llo) * 1.0000002f;
        dU = (Uhi - Ulo) * 1.0000002f;
        wmax = fmaxf(fabsf(Llo), fabsf(Uhi));
    } else {
        DA = R1;
        VA = R2 - DA * DA * rn;
        // |w| <= max |x| over the window: |c0| + the moments' spread bound
        wmax = fabsf(c0) + sqrtf((float)R2 * 1.0001f + E2) * 1.0001f;
    }
    const float rnf = (float)rn * 1.0000002f;
    const float DAf = fabsf((float)DA) * 1.0000002f;
    const float fe1 = E1 + eps * (af * lAf + cf * uAf);
    const float fe2 = E2 + eps * (af * lAf * lAf + cf * uAf * uAf);
    const float eV = fe2 + eps * DAf * DAf * rnf + (2.f * DAf + fe1) * fe1 * rnf;
    const float dev = (DAf + af * dL + cf * dU + fe1) * rnf;
    const float dB = 2.f * af * (lAf + dL + dev) * dL + 2.f * cf * (uAf + dU + dev) * dU;
    const float dmu = wmax * (0x1p-23f + sgc) + fe1 * rnf + 0x1p-120f;
    const float u3c = 3.0000002f * 0x1p-24f + sgc + 0x1p-49f;
    const float eHi = (eV + dB + (float)n * dmu * dmu) * (1.f + 0x1p-18f);
    const double Vlo = (VA - (double)(eV * (1.f + 0x1p-18f))) * (1.0 - (double)u3c) - (double)n * 0x1p-125;
    const double Vhi = (VA + (double)eHi) * (1.0 + (double)u3c) + (double)n * 0x1p-125;
    varlo = (float)((Vlo > 0.0 ? Vlo : 0.0) * rn1);
    varhi = (Vhi - Vhi == 0.0) ? (float)(Vhi * rn1) : f_inf();
}

// median_win's rounding (sorting.c:240-273, 468-513) on two fetched ranks
SG_HD float median_from(float a, float b, int n) {
    if (n & 1) return b;
    if (n < 9) return (float)((double)(a + b) / 2.0);
    return (float)(((double)a + b) / 2.0);
}

// Rejection state of one pixel between rounds (kept in HBM between the head
// and the tail passes of the split rounds) and the per-pixel constants the
// rounds read (recomputed from the stored ranks at every launch).
struct WzState {
    double W1, W2;           // window moments about c0
    float E1, E2;            // their absolute error bounds
    int lo, hi, r, rl, rh;   // window, cutoff counter, rejected low / high
    int pad;
};
struct WzConst {
    SumGuard sg;
    float c0, eps, sgc, slo_, shi_;
    int kept;
    bool exact_w1;
};

// The per-pixel constants (the preamble of the reference's loop): 0, or 1
// when the extreme ranks are not stored.  m: samples the moments pass visited.
template <class RS>
SG_HD int wz_consts(const RS &rs, int kept, float c0, int m, float slo_, float shi_, WzConst &k, float &ymax,
                    float &vmin) {
    float vmax;
    if (!rs.fetch(0, vmin) || !rs.fetch(kept - 1, vmax)) return 1;
    // m = G * el slots of the prep's G lanes.  Depth of its summation tree
    // (wz_prepare): el / NACC chained adds per lane, NACC - 1 to combine the
    // chains, log2 G lane combines (gsum_t) -- 14 + 1 + 2 = 17 at G = 4, N =
    // 100 (el = 28); the depth passed, m / NACC + NACC + 9 = 67 there, bounds
    // it for every G >= 1 (G * el / NACC >= el / NACC, 9 >= log2 G up to 512).
    // One lane per pixel (wz_prepare1, G = 1): m = el (100 at N = 100, where
    // four lanes gave 112), el / NACC chained adds + NACC - 1 combines and no
    // lane level -- 50 + 1 against the 100 / 2 + 2 + 9 = 61 passed
    k.sg = make_guard(vmin, vmax, m + 2, (m + SGPU_NACC - 1) / SGPU_NACC + SGPU_NACC + 9, kept);
    k.eps = (float)(4 * m + 64) * 0x1p-53f;
    k.sgc = (float)k.sg.c * 1.0001f;
    k.c0 = c0;
    k.slo_ = slo_;
    k.shi_ = shi_;
    k.kept = kept;
    ymax = fmaxf(fabsf(vmin - c0), fabsf(vmax - c0)) * 1.0001f;
    // every y and every partial sum of them on the grid of ulp(vmin) / 2 (c0
    // may be a midpoint) within 2^53 of it
    k.exact_w1 = vmin > 0.f && (ebits(vmax) - ebits(vmin) + 26 + ceil_log2(kept) <= 53);
    return 0;
}

// take sample x out of the moments (one clamped or clipped sample)
SG_HD void wz_take(float x, float c0, float eps, double &M1, double &M2, float &F1, float &F2) {
    const double y = (double)x - (double)c0;
    M1 -= y;
    M2 = fma(-y, y, M2);
    F1 += eps * fabsf((float)y);
    F2 += eps * (float)(y * y);
}

// One clamp walk of an iteration (rejection_float.c:229-237 on the sorted
// window): the samples below Lhi at the low end (HI = 0: ranks r0 + cnt
// upwards) or above Ulo at the high end (HI = 1: ranks r0 - cnt downwards)
// leave the moments, lows ascending, highs descending.  nx is the next
// sample, already fetched; cnt the samples this end has given up, other those
// of the other end.  A trip is one straight line: take nx, fetch the next
// rank from this end's region of the record (fetch_lo / fetch_hi), and note
// in `bad` (sticky) what ends the pixel's moment path -- no sample left
// between the ends (cnt + other >= n), or the next rank not stored.  A bad
// lane leaves the walk at once, takes nothing more in this or the other walk,
// and the caller returns 1 after the iteration's arithmetic.  The fetch is
// issued whatever the count says (no branch around it), so at the high end
// the rank is kept from falling below 0; what it reads then is never used.
// (Trips of K = 2, 3 and 4 samples -- K rows of the record at constant
// offsets from one address, sample j taken when the ones before it were --
// measured slower the larger K: DESIGN.md section 8.)
template <int HI, class RS>
SG_HD void wz_walk(const RS &rs, int r0, float bound, float c0, float eps, int n, int other, int &cnt, float &nx,
                   double &M1, double &M2, float &F1, float &F2, bool &bad) {
    while ((HI ? nx > bound : nx < bound) && !bad) {
        wz_take(nx, c0, eps, M1, M2, F1, F2);
        cnt++;
        const int r = HI ? (r0 - cnt > 0 ? r0 - cnt : 0) : r0 + cnt;
        const bool ok = HI ? rs.fetch_hi(r, nx) : rs.fetch_lo(r, nx);
        bad = cnt + other >= n || !ok;
    }
}

// One rejection round of the pixel on moments (rejection_float.c:223-259,
// one pass of its do-while).  Returns 0 (st updated; more: another round
// follows), 1: the sorted kernel takes the pixel, 2: the exact kernel takes
// it (order-dependent cutoff, as the sorted path decides).
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
    if (!rs.fetch_lo(lo, xw0) || !rs.fetch_hi(hi - 1, xw1)) return 1;
    // the round's first sd (siril_stats_float_sd of the window, :226)
    float vlo, vhi;
    const bool flat = xw0 == xw1;         // constant window: every sd below is exactly 0
    var_bounds(st.W1, st.W2, st.E1, st.E2, 0, 0, n, c0, 0.f, 0.f, 0.f, 0.f, false, eps, sgc, rn, rn1, vlo, vhi);
    if (flat) vlo = vhi = 0.f;
    float slo = sqrt_lo(vlo), shi = sqrt_hi(vhi);
    // clamp iterations (:229-237).  The loop has one exit: what would end the
    // pixel's moment path (a walk's `bad`, a sigma bound that is not finite,
    // the iteration cap, a stop test the interval does not decide) is
    // collected in `bad` and returned after it, so the state below is
    // updated in place and nothing is copied on the way round.
    float Llo = -f_inf(), Lhi = -f_inf(), Ulo = f_inf(), Uhi = f_inf();
    int a = 0, c = 0;
    double R1 = st.W1, R2 = st.W2;
    float F1 = st.E1, F2 = st.E2;
    float nlo = xw0, nhi = xw1;           // next samples to clamp: ranks lo + a, hi - 1 - c
    bool bad = false;
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
        wz_walk<0>(rs, lo, Lhi, c0, eps, n, c, a, nlo, R1, R2, F1, F2, bad);
        wz_walk<1>(rs, hi - 1, Ulo, c0, eps, n, a, c, nhi, R1, R2, F1, F2, bad);
        SGPU_WZ_TRACE(1);
        var_bounds(R1, R2, F1, F2, a, c, n, c0, Llo, Lhi, Ulo, Uhi, true, eps, sgc, rn, rn1, vlo, vhi);
        if (flat) vlo = vhi = 0.f;
        bad |= !(vhi - vhi == 0.f);
        const float s0lo = slo, s0hi = shi;
        slo = 1.134f * sqrt_lo(vlo);
        shi = 1.134f * sqrt_hi(vhi);
        const float A = slo - s0hi, B = shi - s0lo;      // fl(sigma - sigma0) in [A, B]
        const float dmin = A > 0.f ? A : (B < 0.f ? -B : 0.f);
        const float dmax = fmaxf(fabsf(A), fabsf(B));
        const bool go = dmin > s0hi * 0.0005f;           // another iteration; else it must be a sure stop
        it += go ? 1 : 0;
        bad |= go ? it > kWinsorCap : !(dmax <= s0lo * 0.0005f);
        if (!go || bad) break;
    }
    if (bad) return 1;
    // sigma_clipping_float (:238-246) with sigma in [slo, shi]
    int cl = 0, ch = 0;
    if (n - st.r > 4) {
        const float tl0 = slo * k.slo_, th0 = slo * k.shi_, tl1 = shi * k.slo_, th1 = shi * k.shi_;
        if (!(tl0 >= 0.f && th0 >= 0.f)) return 2;
        if (wz_clip_counts(rs, lo, hi, mf, tl0, th0, tl1, th1, cl, ch)) return 1;
    }
    // the clipped samples leave the moments (before the window moves)
    const int lo0 = lo, hi0 = hi;
    bool changed;
    if (cutoff_round(n, st.r, cl, ch, lo, hi, st.rl, st.rh, changed)) return 2;
    for (int j = 0; j < lo - lo0; j++) {
        float x;
        if (!rs.fetch_lo(lo0 + j, x)) return 1;
        wz_take(x, c0, eps, st.W1, st.W2, st.E1, st.E2);
    }
    for (int j = 0; j < hi0 - hi; j++) {
        float x;
        if (!rs.fetch_hi(hi0 - 1 - j, x)) return 1;
        wz_take(x, c0, eps, st.W1, st.W2, st.E1, st.E2);
    }
    st.lo = lo;
    st.hi = hi;
    more = changed && hi - lo > 3;
    return 0;
}

// mean of the kept window (median_and_mean.c:1083-1097): sum x = W1 + n c0
template <class RS>
SG_HD int wz_final(const RS &rs, const WzConst &k, const WzState &st, PixOut &o) {
    const int n = st.hi - st.lo;
    o.rl = st.rl;
    o.rh = st.rh;
    if (!rs.fetch(st.lo, o.pmin) || !rs.fetch(st.hi - 1, o.pmax)) return 1;
    const double s = st.W1 + (double)n * (double)k.c0;
    o.res = s / (double)n;
    o.nkept = n;
    if (!k.exact_w1) {
        const double e = (double)st.E1 * 1.0001 + sum_bound(k.sg, s, o.pmin, o.pmax, n) + fabs(s) * 0x1p-50;
        if (!f32_stable(o.res, e / n)) return 1;
    }
    return 0;
}

// Start of a pixel: 3 when o is final already (kept == 1), 1 for the sorted
// kernel, else 0 with k / st ready for the rounds.
template <int U16 = 0, class RS>
SG_HD int wz_start(const RS &rs, int kept, double W1, double W2, float c0, int m, float slo_, float shi_,
                   WzConst &k, WzState &st, PixOut &o) {
    o.rl = o.rh = 0;
    o.res = 0.0;
    o.nkept = 0;
    o.pmin = o.pmax = 0.f;
    o.fallback = 0;
    if (kept == 1) {                        // apply_rejection_float returns kept <= 1 (:140-142)
        float v0;
        if (!rs.fetch(0, v0)) return 1;
        o.res = (double)v0;
        o.pmin = o.pmax = v0;
        o.nkept = 1;
        return 3;
    }
    if (U16 && c0 == 0.f) return 4;         // 16-bit: median 0 -> no sample kept (:747-756): exact kernel
    float ymax, vmin;
    if (wz_consts(rs, kept, c0, m, slo_, shi_, k, ymax, vmin)) return 1;
    st.W1 = W1;
    st.W2 = W2;
    st.E1 = k.eps * (float)kept * ymax;
    st.E2 = k.eps * (float)W2;
    st.lo = 0;
    st.hi = kept;
    st.r = st.rl = st.rh = 0;
    st.pad = 0;
    return 0;
}

// Second half of a pixel: from the stored ranks and the window moments (W1,
// W2 about c0) to the result, every round in one call.  Returns the route
// (0 result in o, 1 sorted kernel, 2 exact kernel).  m: samples the moments
// pass visited.  (A one-phase-per-call state machine with lane refill, so
// that lanes do not wait for the slowest pixel of their wave, was built and
// measured slower: 25.1 vs 17.1 ms for config 2 -- every trip pays every
// phase some lane is in.  The split rounds below compact the pixels that
// outlast the head's cap instead.)
template <int U16 = 0, class RS>
SG_HD int wz_finish(const RS &rs, int kept, double W1, double W2, float c0, int m, float slo_, float shi_,
                    PixOut &o) {
    WzConst k;
    WzState st;
    int rc = wz_start<U16>(rs, kept, W1, W2, c0, m, slo_, shi_, k, st, o);
    if (rc == 3) return 0;
    if (rc == 4) return 2;
    if (rc) return rc;
    bool more = true;
    while (more)
        if ((rc = wz_round<U16>(rs, k, st, more))) return rc;
    return wz_final(rs, k, st, o);
}

// Split rounds (SGPU_WZ_SPLIT): at most `cap` rounds from the state st, then
// the pixel is handed on with its state (route kWzDeferred; st holds what the
// next pass resumes from, after wz_consts has rebuilt the constants).  cap <=
// 0: no cap.  The rounds, their order and every value they compute are the
// ones of wz_finish's loop, so a pixel resumed any number of times gets
// wz_finish's result bit for bit (tests/hostsim/wz_split_main.cpp).
constexpr int kWzDeferred = 5;
template <int U16 = 0, class RS>
SG_HD int wz_rounds_cap(const RS &rs, const WzConst &k, WzState &st, int cap, PixOut &o) {
    bool more = true;
    for (int r = 0; more; r++) {
        if (r == cap) return kWzDeferred;
        if (const int rc = wz_round<U16>(rs, k, st, more)) return rc;
    }
    return wz_final(rs, k, st, o);
}

// What the head leaves for the tail passes.  The ranks of a deferred pixel
// are its column of the slot-major record: gathered from there, 64 listed
// pixels touch nearly every line of the chunk's record (one pixel in 16 is
// listed at sigma 3/3: the first build's tail pass re-read the whole record,
// 0.67 GB per chunk, and halved the speed of the prep kernel running beside
// it).  So the head copies the R ranks of its i-th deferring lane to words
// [i * R, (i + 1) * R) of its own tile of the record -- the R x tw words of
// its tw <= 64 pixels' columns, taken row after row -- which it has staged in
// LDS and nobody reads again: a pixel's copy is R contiguous words in at most
// two rows, and a tail lane reads three 64-byte sectors instead of R.
// List entry: head block, index of the copy in the tile, lane (loc = 64 *
// block + lane).
SG_HD long long wz_crec_index(int f, int tw, long long cnt, long long col0) {
    const int row = tw == 64 ? f >> 6 : f / tw, col = tw == 64 ? f & 63 : f % tw;
    return (long long)row * cnt + col0 + col;
}
SG_HD int wz_entry(int block, int ci, int lane) { return (block << 12) | (ci << 6) | lane; }

// wz_finish with a rounds cap: the head pass of the split
template <int U16 = 0, class RS>
SG_HD int wz_finish_cap(const RS &rs, int kept, double W1, double W2, float c0, int m, float slo_, float shi_,
                        int cap, PixOut &o, WzState &st) {
    WzConst k;
    const int rc = wz_start<U16>(rs, kept, W1, W2, c0, m, slo_, shi_, k, st, o);
    if (rc == 3) return 0;
    if (rc == 4) return 2;
    if (rc) return rc;
    return wz_rounds_cap<U16>(rs, k, st, cap <= 0 ? -1 : cap, o);
}

// First half: sort the gathered column, store its ranks, and the window
// moments about the first median c0 (one f64 pass; ranks >= kept hold +Inf
// and add 0).  Returns 2 for the exact kernel (kept == 0), else 0.
// GBUF: the record is the prep kernel's HBM one (RankStore::store_buf).
// RS: RankStore<NP, G> at any depth.
template <int NP, int G, int RSL = NP / G, bool GBUF = false, class RS>
SG_HD int wz_prepare(float (&v)[NP / G], int g, int kept, int kmin, int N, RS &rs, double &W1, double &W2,
                     float &c0) {
    constexpr int E = NP / G;
    static_assert(RS::E == E && RS::PW == 64 / G, "the record of this column layout");
    if (kept == 0) return 2;                // quickmedian of the whole stack (median_and_mean.c:1040)
    sort_col<NP, G, RSL>(v, g);
    if constexpr (G == 2) to_interleaved2<E>(v, g);
    else if constexpr (G > 2) to_interleaved<E, G>(v, g);
    rs.kept = kept;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (GBUF) rs.store_buf(v, g, kmin, N);
    else rs.store(v, g, kmin, N);
#else
    rs.store(v, g, kmin, N);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (GBUF) {
        // c0 from the middle slots only: the two ranks median_win reads,
        // (kept - 1) / 2 .. kept / 2, lie in slots [(kmin / 2 - 1) / G,
        // (N / 2) / G] over the wave (kept in [kmin, N]), a wave-uniform
        // window of a few slots -- a select chain over it instead of two
        // 63-deep select trees over the whole column
        const int ra = kept / 2 - ((kept & 1) ? 0 : 1), rb = kept / 2;
        const int ew0 = (kmin / 2 - 1) / G, ew1 = (N / 2) / G;
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (e >= ew0 && e <= ew1) {
                sa = (e == ra / G) ? v[e] : sa;
                sb = (e == rb / G) ? v[e] : sb;
            }
        }
        c0 = median_from(gbcast<G>(sa, ra & (G - 1)), gbcast<G>(sb, rb & (G - 1)), kept);
    } else {
        c0 = (float)median_win<E, G, true>(v, 0, kept);
    }
#else
    c0 = (float)median_win<E, G, true>(v, 0, kept);
#endif
    const int el = (((N + G - 1) / G) + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
    const int elim = el < E ? el : E;
    double s1[SGPU_NACC], s2[SGPU_NACC];
#pragma unroll
    for (int q = 0; q < SGPU_NACC; q++) s1[q] = s2[q] = 0.0;
    const double cd = (double)c0;
#pragma unroll
    for (int e = 0; e < E; e++) {
        SG_STOP4(e, elim);
        const float xe = v[e] < f_inf() ? v[e] : c0;
        const double y = (double)xe - cd;
        s1[e % SGPU_NACC] += y;
        s2[e % SGPU_NACC] = fma(y, y, s2[e % SGPU_NACC]);
    }
    W1 = s1[0];
    W2 = s2[0];
#pragma unroll
    for (int q = 1; q < SGPU_NACC; q++) {
        W1 += s1[q];
        W2 += s2[q];
    }
    W1 = gsum_t<G>(W1);
    W2 = gsum_t<G>(W2);
    return 0;
}

// One pixel after the gather, prep and rounds in one call on an LDS-style
// rank store: the host simulation's entry (tests/hostsim); no kernel calls it.
template <int NP, int G, int U16 = 0, class RS>
SG_HD int wz_pixel(float (&v)[NP / G], int g, int kept, int kmin, int N, float slo_, float shi_, RS &rs,
                   PixOut &o) {
    constexpr int E = NP / G;
    double W1, W2;
    float c0;
    o.rl = o.rh = 0;
    if (wz_prepare<NP, G>(v, g, kept, kmin, N, rs, W1, W2, c0)) return 2;
    return wz_finish<U16>(rs, kept, W1, W2, c0, G * E, slo_, shi_, o);
}

// The rounds on a rank store that holds EVERY rank of the sorted column (no
// stored-range fallbacks): the host simulation runs wz_finish on it against
// the oracle (tests/hostsim sim_wz1_pixels), which checks the rounds apart
// from RankStore's ranges.  No kernel uses it.
struct ColStore {
    const float *base;                   // the pixel's row: rank r at base[r]
    int kept;
    SG_HD bool fetch(int r, float &x) const {
        const bool ok = r >= 0 && r < kept;
        x = base[ok ? r : 0];
        return ok;
    }
    // every rank is stored: RankStore's end fetches are plain reads here
    SG_HD bool fetch_lo(int r, float &x) const { return fetch(r, x); }
    SG_HD bool fetch_hi(int r, float &x) const { return fetch(r, x); }
};

// From the sorted column (ranks 0..N-1 in row[], missing samples +Inf at
// ranks >= kept) to the result: first median (median_win's rounding), the
// window moments about it in rank order (accumulator q takes ranks = q mod
// SGPU_NACC; ranks >= kept add 0), then every round on ColStore.
SG_HD int wz1_pixel(const float *row, int kept, int N, float sig0, float sig1, PixOut &o) {
    const int k2 = kept / 2;
    const float c0 = median_from(row[(kept & 1) ? k2 : k2 - 1], row[k2], kept);
    const double cd = (double)c0;
    double s1[SGPU_NACC], s2[SGPU_NACC];
#pragma unroll
    for (int q = 0; q < SGPU_NACC; q++) s1[q] = s2[q] = 0.0;
    const int el = (N + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
    for (int e = 0; e < el; e += SGPU_NACC) {
#pragma unroll
        for (int q = 0; q < SGPU_NACC; q++) {
            const int r = e + q;
            const float xe = r < kept ? row[r < N ? r : 0] : c0;
            const double y = (double)xe - cd;
            s1[q] += y;
            s2[q] = fma(y, y, s2[q]);
        }
    }
    double W1 = s1[0], W2 = s2[0];
#pragma unroll
    for (int q = 1; q < SGPU_NACC; q++) {
        W1 += s1[q];
        W2 += s2[q];
    }
    ColStore cs;
    cs.base = row;
    cs.kept = kept;
    return wz_finish(cs, kept, W1, W2, c0, el, sig0, sig1, o);
}

// ---------------------------------------------------------------- two-kernel form
// The path split where its needs split: k_stack_wz_prep (gather, sort,
// rank store, moments: the register-wide part, G lanes per pixel) writes a
// record per pixel to HBM -- ranks slot-major (lanes of a wave read
// neighbouring words), moments and packed bounds -- and k_stack_wz_rounds
// runs the latency-bound scalar rounds one lane per pixel at a few dozen
// VGPRs, so four times the pixels per SIMD are in flight.
// RSL: real-slot bound of the sort network (sort_col; the launch picks it
// with rs_pick, stack_sorted_rs*.hip instantiate the pruned variants)
template <int NP, int G, int XF, int W, int RSL = NP / G, int U16 = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
void k_stack_wz_prep(KParams p) {
    constexpr int E = NP / G;
    using RS = RankStore<NP, G>;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long loc = gid / G;
    const int g = (int)(gid % G);
    if (loc >= p.wz_cnt) return;              // group-uniform; no cross-wave work below
    const long long pix = p.wz_pix0 + loc;
    const int x = (int)(pix % p.W);
    int kept = 0, bad = 0;
    float v[E];
#ifndef SGPU_PREP_GATHER_RS
#define SGPU_PREP_GATHER_RS 0    // 1: the gather also bounded at RSL (A/B; the runtime gather stop already skips those loads)
#endif
    gather_column<XF, E, G, true, U16, SGPU_PREP_GATHER_RS ? RSL : E, false>(p, v, pix, x, g, kept, bad);
    bad = gsum_t<G>(bad);
    kept = gsum_t<G>(kept);
    int kmin = kept;
#pragma unroll
    for (int lm = 32; lm >= 1; lm >>= 1) kmin = min(kmin, __shfl_xor(kmin, lm, 64));
    kmin = __builtin_amdgcn_readfirstlane(kmin);
    RS rs;
    rs.base = p.wz_ranks;
    rs.stride = p.wz_cnt;
    rs.p = loc;
    double W1 = 0.0, W2 = 0.0;
    float c0 = 0.f;
#ifndef SGPU_WZ_GBUF
#define SGPU_WZ_GBUF 1          // 0: the record stored with per-rank predicates (RankStore::store; A/B)
#endif
    const int route = bad ? 2 : wz_prepare<NP, G, RSL, SGPU_WZ_GBUF != 0>(v, g, kept, kmin, p.nframes, rs, W1, W2, c0);
    if (g == 0) {
        p.wz_mom[loc] = W1;
        p.wz_mom[p.wz_cnt + loc] = W2;
        p.wz_mom[2 * p.wz_cnt + loc] = (double)c0;
        int4 m;
        m.x = route ? -1 : kept;
        m.y = rs.hi0;
        m.z = rs.mid0;
        m.w = rs.mid1;
        reinterpret_cast<int4 *>(p.wz_meta)[loc] = m;
    }
}

// One lane per pixel (NP = 128, float): the column sorted in one lane has no
// cross-lane merge (v_med3 + lane exchanges) and no interleave; what the
// four-lane form spends there is 60 instructions a pixel against the 36 of
// oem_sort<128, 104>.  The kernel is written for the wave that has (nearly)
// every sample -- every lane's kept >= RSL - 7, the lowest N of the real-slot
// bucket (rs_pick: N in [RSL - 7, RSL]) -- because then everything that
// depends on `kept` lies in compile-time slot ranges:
//   * ranks [kept - KT, kept) in slots [RSL - 7 - KT, RSL), ranks
//     [kept / 2 - KM / 2, kept / 2 + KM / 2) in [RSL / 2 - KM, RSL / 2 + KM /
//     2): with the low KT slots 51 unconditional stores through the region
//     descriptors of store_buf (RankStore::store_full), no branch;
//   * the two ranks of the first median in slots [RSL / 2 - 4, RSL / 2];
//   * +Inf (a missing sample) only in slots >= RSL - 7: the moments pass
//     needs its `finite ? v : c0` select there alone, and N >= RSL - 7 puts
//     its one stop (el = round4(N)) at RSL - 4 or RSL.
// A wave with a lane below that (nulls, a frame's border) takes the run-time
// slot loops of the G-lane form in a wave-uniform branch.  Either way the
// record, the moments (same accumulators, same order) and m.y/z/w are what
// wz_prepare<128, 1> gives.
// LDS: the ranks go to the wave's LDS tile (k_stack_wz_fused1: rs.base the
// tile, rs.stride 64, rs.p the lane) through store_full_lds / store instead of
// the HBM record; everything else is the same code.
// (wave_any / wave_min: one lane is the wave in a host build, tests/hostsim)
SG_HD bool wave_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(x) != 0ull;
#else
    return x;
#endif
}
SG_HD int wave_min(int x) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int lm = 32; lm >= 1; lm >>= 1) x = min(x, __shfl_xor(x, lm, 64));
    x = __builtin_amdgcn_readfirstlane(x);
#endif
    return x;
}
// (wz_prepare1_sorted: everything after the sort -- the fused kernel sets its
// tile's RankStore up between the two, so that nothing of it lives through
// the sort)
// RS: RankStore<128, 1> at the depth of the form that runs
template <int RSL, bool LDS = false, class RS>
SG_HD void wz_prepare1_sorted(const float (&v)[128], int kept, int N, RS &rs, double &W1, double &W2, float &c0) {
    static_assert(RS::E == 128 && RS::PW == 64, "one lane per pixel, N <= 128");
    constexpr int E = 128, K0 = RSL - 7;
    static_assert(RSL % 8 == 0 && RSL >= 72 && RSL <= E, "real-slot buckets of rs_pick(128, 1, N)");
    rs.kept = kept;
    const int ra = kept / 2 - ((kept & 1) ? 0 : 1), rb = kept / 2;
    const int el = (N + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
    double s1[SGPU_NACC], s2[SGPU_NACC];
#pragma unroll
    for (int q = 0; q < SGPU_NACC; q++) s1[q] = s2[q] = 0.0;
    float sa = 0.f, sb = 0.f;
    if (!wave_any(kept < K0)) {
        if constexpr (LDS) rs.template store_full_lds<RSL>(v);
        else rs.template store_full<RSL>(v);
#pragma unroll
        for (int e = RSL / 2 - 4; e <= RSL / 2; e++) {
            sa = (e == ra) ? v[e] : sa;
            sb = (e == rb) ? v[e] : sb;
        }
        c0 = median_from(sa, sb, kept);
        const double cd = (double)c0;
#pragma unroll
        for (int e = 0; e < RSL; e++) {
            if (e == RSL - 4 && el <= RSL - 4) break;
            const float xe = (e < K0 || v[e] < f_inf()) ? v[e] : c0;
            const double y = (double)xe - cd;
            s1[e % SGPU_NACC] += y;
            s2[e % SGPU_NACC] = fma(y, y, s2[e % SGPU_NACC]);
        }
    } else {
        const int kmin = wave_min(kept);
        if constexpr (LDS) rs.store(v, 0, kmin, N);
        else rs.store_buf(v, 0, kmin, N);
        const int ew0 = kmin / 2 - 1, ew1 = N / 2;
#pragma unroll
        for (int e = 0; e <= RSL / 2; e++) {
            if (e >= ew0 && e <= ew1) {
                sa = (e == ra) ? v[e] : sa;
                sb = (e == rb) ? v[e] : sb;
            }
        }
        c0 = median_from(sa, sb, kept);
        const double cd = (double)c0;
        const int elim = el < RSL ? el : RSL;
#pragma unroll
        for (int e = 0; e < RSL; e++) {
            SG_STOP4(e, elim);
            // the sorted column's +Inf are its ranks >= kept; the compare
            // follows its slot's turn (pinned: 128 of them moved to the front
            // each held an SGPR pair to its select)
            int ke = kept;
            opaque(ke);
            const float xe = e < ke ? v[e] : c0;
            const double y = (double)xe - cd;
            s1[e % SGPU_NACC] += y;
            s2[e % SGPU_NACC] = fma(y, y, s2[e % SGPU_NACC]);
        }
    }
    W1 = s1[0];
    W2 = s2[0];
#pragma unroll
    for (int q = 1; q < SGPU_NACC; q++) {
        W1 += s1[q];
        W2 += s2[q];
    }
}

template <int RSL, bool LDS = false, class RS>
SG_HD void wz_prepare1(float (&v)[128], int kept, int N, RS &rs, double &W1, double &W2, float &c0) {
    sort_col<128, 1, RSL>(v, 0);
    wz_prepare1_sorted<RSL, LDS>(v, kept, N, rs, W1, W2, c0);
}

template <int NP, int XF, int W, int RSL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
void k_stack_wz_prep1(KParams p) {
    static_assert(NP == 128, "one lane per pixel: N <= 128");
    using RS = RankStore<NP, 1>;
    const long long loc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (loc >= p.wz_cnt) return;
    const long long pix = p.wz_pix0 + loc;
    int kept = 0, bad = 0;
    float v[NP];
    gather_column<XF, NP, 1, true, 0, RSL, SGPU_GATHER_SLOTSTEP, true>(p, v, pix, (int)(pix % p.W), 0, kept, bad);
    // the NaN / Inf test is settled here: its only reader is the record's
    // last store, and left to the compiler the detector's chain sinks below
    // the sort with a copy of every gathered sample alive (104 VGPRs)
    opaque(bad);
    RS rs;
    rs.base = p.wz_ranks;
    rs.stride = p.wz_cnt;
    rs.p = loc;
    double W1, W2;
    float c0;
    // a column with a NaN or no sample goes through as well (wave-uniform
    // code; what it stores stays in its own column of the record, unread)
    wz_prepare1<RSL>(v, kept, p.nframes, rs, W1, W2, c0);
    p.wz_mom[loc] = W1;
    p.wz_mom[p.wz_cnt + loc] = W2;
    p.wz_mom[2 * p.wz_cnt + loc] = (double)c0;
    int4 m;
    m.x = (bad || kept == 0) ? -1 : kept;
    m.y = rs.hi0;
    m.z = rs.mid0;
    m.w = rs.mid1;
    reinterpret_cast<int4 *>(p.wz_meta)[loc] = m;
}

// PG (here and in the rounds kernels below): the lanes per pixel of the prep
// kernel that wrote the records -- PG * el slots went into its moments, the
// term count its error bounds take (the launcher passes the prep's own G).
// Global rank reads, five waves per SIMD: N > 128 and the 16-bit path.
template <int NP, int U16 = 0, int PG = NP / 64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8)))
void k_stack_wz_rounds(KParams p) {
    using RS = RankStore<NP, 1>;
    const long long loc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int rl = 0, rh = 0;
    if (loc < p.wz_cnt) {
        const long long pix = p.wz_pix0 + loc;
        const int4 m = reinterpret_cast<const int4 *>(p.wz_meta)[loc];
        int route = 2;
        PixOut o;
        if (m.x > 0) {
            RS rs;
            rs.base = p.wz_ranks;
            rs.stride = p.wz_cnt;
            rs.p = loc;
            rs.kept = m.x;
            rs.hi0 = m.y;
            rs.mid0 = m.z;
            rs.mid1 = m.w;
            constexpr int G = PG;              // the prep kernel's lanes per pixel
            const int N = p.nframes;
            const int el = (((N + G - 1) / G) + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
            route = wz_finish<U16>(rs, m.x, p.wz_mom[loc], p.wz_mom[p.wz_cnt + loc],
                                   (float)p.wz_mom[2 * p.wz_cnt + loc], G * el, p.sig0, p.sig1, o);
        }
        if (route == 1) {
            const int slot = wave_append(p.fb2_count, true);
            p.fb2_list[slot] = (int)pix;
        } else if (route == 2) {
            const int slot = wave_append(p.fb_count, true);
            p.fb_list[slot] = (int)pix;
        } else {
            double res = o.res;
            if (is_weighted(p)) res = weighted_mean<U16>(p, pix, (int)(pix % p.W), o.pmin, o.pmax, o.nkept);
            if constexpr (U16) write_result16(p, pix, res, o.rl, o.rh);
            else write_result(p, pix, res, o.rl, o.rh);
            rl = o.rl;
            rh = o.rh;
        }
    }
    add_counts(p, rl, rh);
}

// Rounds kernel with the rank records staged in LDS (N <= 128): one wave per
// block copies its 64 pixels' R rank slots
// (slot-major rows of the workspace: every copy instruction reads 256
// contiguous bytes) into LDS, so the dependent rank reads of the rounds
// (medians, tail walks, clip walks) are LDS round trips instead of L2 / HBM
// misses -- half of the global-read kernel's wave-cycles waited on them
// (profiles/r05q_pmc_rounds.json).  At R = 40 slots (KT = 16, KM = 8) a wave
// takes 10 KB: 16 waves per CU, the register-bound occupancy too.  (At the
// round-3 R = 64 the LDS held 10 waves per CU and the staging lost.)
template <int NP, int U16 = 0, int PG = NP / 64>
__global__ __launch_bounds__(64) void k_stack_wz_rounds_lds(KParams p, WzSplit sp) {
    using RS = RankStore<NP, 1>;
    __shared__ float s_rank[RS::R * 64];
    const int lane = (int)threadIdx.x;
    const long long loc = (long long)blockIdx.x * 64 + lane;
    const bool live = loc < p.wz_cnt;
    int4 m = make_int4(0, 0, 0, 0);
    if (live) m = reinterpret_cast<const int4 *>(p.wz_meta)[loc];
    {
        float t[RS::R];
#if defined(__HIP_DEVICE_COMPILE__)
        // one descriptor over the record (R * cnt * 4 bytes < 2^31: the
        // launcher's NP * ch * 4 <= 2^32 bound) and a 32-bit byte offset per
        // lane: slot j's uniform part goes to soffset (no 64-bit multiply per
        // slot); lanes past the chunk read zeros, discarded below
        const uint32_t S4 = (uint32_t)p.wz_cnt * 4u;
        const auto rr = __builtin_amdgcn_make_buffer_rsrc(p.wz_ranks, (short)0, (int)((uint32_t)RS::R * S4), 0x00020000);
        const int vo = live ? (int)((uint32_t)loc * 4u) : (int)((uint32_t)RS::R * S4);
#pragma unroll
        for (int j = 0; j < RS::R; j++)
            t[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, vo, (int)((uint32_t)j * S4), 0));
#else
#pragma unroll
        for (int j = 0; j < RS::R; j++) t[j] = live ? p.wz_ranks[(long long)j * p.wz_cnt + loc] : 0.f;
#endif
#pragma unroll
        for (int j = 0; j < RS::R; j++) s_rank[j * 64 + lane] = t[j];
    }
    __syncthreads();
    int rl = 0, rh = 0;
    if (live) {
        const long long pix = p.wz_pix0 + loc;
        int route = 2;
        PixOut o;
        WzState st;
        if (m.x > 0) {
            RS rs;
            rs.base = s_rank;
            rs.stride = 64;
            rs.p = lane;
            rs.kept = m.x;
            rs.hi0 = m.y;
            rs.mid0 = m.z;
            rs.mid1 = m.w;
            constexpr int G = PG;
            const int N = p.nframes;
            const int el = (((N + G - 1) / G) + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
            // (16-bit columns stay on the one nest: their kernel with the
            // capped form measured 12.39 against 12.29 ms, winsorized100_u16)
            if constexpr (U16)
                route = wz_finish<U16>(rs, m.x, p.wz_mom[loc], p.wz_mom[p.wz_cnt + loc],
                                       (float)p.wz_mom[2 * p.wz_cnt + loc], G * el, p.sig0, p.sig1, o);
            else
                route = wz_finish_cap<U16>(rs, m.x, p.wz_mom[loc], p.wz_mom[p.wz_cnt + loc],
                                           (float)p.wz_mom[2 * p.wz_cnt + loc], G * el, p.sig0, p.sig1, sp.cap, o, st);
        }
        if (!U16 && route == kWzDeferred) {
            // more rounds than the cap: the pixel goes to the tail pass with
            // its state and a compact copy of its ranks (wz_crec_index); no
            // result, no fallback list, no rejection totals
            const unsigned long long dm = __ballot(true);          // the wave's deferring lanes
            const int ci = (int)__popcll(dm & ((1ull << lane) - 1ull));
            const long long col0 = (long long)blockIdx.x * 64;
            const int tw = (int)(p.wz_cnt - col0 < 64 ? p.wz_cnt - col0 : 64);
            const int stripe = (int)blockIdx.x / sp.bps;
            const int slot = wave_append(sp.cnt_out + stripe * kWzStripeStep, true);
            sp.list_out[stripe * sp.bps * 64 + slot] = wz_entry((int)blockIdx.x, ci, lane);
            reinterpret_cast<WzState *>(p.wz_state)[loc] = st;
            static_assert(RS::R % 4 == 0, "a copy is whole 16-byte pieces");
            if (tw == 64 && (p.wz_cnt & 3) == 0) {
                // full tile, rows 16-byte aligned: four words of the copy never
                // straddle a row -- R / 4 wide stores, 32-bit index arithmetic
                // (R * cnt words < 2^30: the launcher's bound)
                const unsigned cnt = (unsigned)p.wz_cnt, c0w = (unsigned)col0;
#pragma unroll 2
                for (int j = 0; j < RS::R; j += 4) {
                    const unsigned f = (unsigned)(ci * RS::R + j);
                    const float4 q = make_float4(s_rank[j * 64 + lane], s_rank[(j + 1) * 64 + lane],
                                                 s_rank[(j + 2) * 64 + lane], s_rank[(j + 3) * 64 + lane]);
                    *reinterpret_cast<float4 *>(p.wz_ranks + (umul24(f >> 6, cnt) + c0w + (f & 63u))) = q;
                }
            } else {
#pragma unroll 4
                for (int j = 0; j < RS::R; j++)
                    p.wz_ranks[wz_crec_index(ci * RS::R + j, tw, p.wz_cnt, col0)] = s_rank[j * 64 + lane];
            }
        } else if (route == 1) {
            const int slot = wave_append(p.fb2_count, true);
            p.fb2_list[slot] = (int)pix;
        } else if (route == 2) {
            const int slot = wave_append(p.fb_count, true);
            p.fb_list[slot] = (int)pix;
        } else {
            double res = o.res;
            if (is_weighted(p)) res = weighted_mean<U16>(p, pix, (int)(pix % p.W), o.pmin, o.pmax, o.nkept);
            if constexpr (U16) write_result16(p, pix, res, o.rl, o.rh);
            else write_result(p, pix, res, o.rl, o.rh);
            rl = o.rl;
            rh = o.rh;
        }
    }
    add_counts(p, rl, rh);
}

// Fused form (SGPU_WZ=7; float, N = 65..128): k_stack_wz_prep1 and the capped
// head k_stack_wz_rounds_lds<128, 0, 1> in one kernel, so that the rank record
// never goes to HBM.  A wave of the one-lane prep holds exactly the 64 pixels
// of a head block (its tile: wave w of block b is head block 4 b + w), a lane
// owns its pixel's sorted column, and the R rank slots go straight into the
// wave's own [slot][lane] LDS tile -- the layout the head stages -- with no
// cross-wave exchange and no block barrier.  Gather, NaN pin, sort, moments,
// c0 and meta are wz_prepare1's, the rounds wz_finish_cap's with the same m,
// the routes the head's; so every pixel ends exactly as on the two-kernel
// path.  Only a deferring lane leaves something in the workspace, and leaves
// all k_stack_wz_tail reads: its state, meta, moments, the compact copy of its
// ranks in its tile of the (otherwise unwritten) record and the list entry.
// The record never leaves the CU, so from RSL = 96 up it is the deeper one
// (wz_fused_kt: SGPU_WZ_KT_FUSED ranks per end, R = 48): four waves x 12 KB of
// LDS per block, three blocks in a CU's 160 KB; the register budget is the
// prep's (three waves per SIMD), the rounds need fewer once the column is
// dead.
template <int NP, int XF, int W, int RSL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
void k_stack_wz_fused1(KParams p, WzSplit sp) {
    static_assert(NP == 128, "one lane per pixel: N <= 128");
    using RS = RankStore<NP, 1, wz_fused_kt(RSL)>;
    static_assert(W * 4 * RS::R * 64 * sizeof(float) <= 160 * 1024, "W blocks' tiles in one CU's LDS");
    // The tiles, 4 * R * 64 floats.  At depth SGPU_WZ_KT (RSL <= 88) declared
    // with their size, 40 KB, as they always were: those kernels compile to
    // the instructions they had.  At the deeper record they are sized by the
    // launch (wz_fused_lds_bytes): declared with its size, 48 KB puts the
    // compiler's occupancy estimate at three waves and its scheduler at ease
    // with all 168 VGPRs of that budget -- the RSL = 104 kernel then peaks at
    // the end of the gather and spills 4 dwords to scratch, where it took 158
    // VGPRs and none with 40 KB; unsized, it compiles to 158 and no scratch.
    float *s_rank;
    if constexpr (wz_fused_kt(RSL) == SGPU_WZ_KT) {
        __shared__ float s_sized[4 * RS::R * 64];
        s_rank = s_sized;
    } else {
        extern __shared__ float s_unsized[];
        s_rank = s_unsized;
    }
    // the head block of this wave (wave-uniform; nothing below crosses waves)
    if (((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 >= p.wz_cnt) return;
    int kept = 0, bad = 0;
    double W1, W2;
    float c0;
    RS rs;
    float v[NP];
    {
        // a lane past the chunk gathers the wave's first pixel (valid
        // addresses, wave-uniform code) and is discarded below
        const long long c = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64, l = c + (threadIdx.x & 63);
        const long long gp = p.wz_pix0 + (l < p.wz_cnt ? l : c);
        gather_column<XF, NP, 1, true, 0, RSL, SGPU_GATHER_SLOTSTEP, true>(p, v, gp, (int)(gp % p.W), 0, kept, bad);
    }
    opaque(bad);                              // (k_stack_wz_prep1: the NaN test settled before the sort)
    sort_col<NP, 1, RSL>(v, 0);
    // everything that depends on the thread index is worked out after the
    // sort, from a copy of it the compiler cannot trace back: the sort's peak
    // holds the column, kept and bad, as the prep kernel's does
    int tid = (int)threadIdx.x;
    opaque(tid);
    const int lane = tid & 63;
    const long long tile = (long long)blockIdx.x * 4 + (tid >> 6);
    const long long col0 = tile * 64;
    const long long loc = col0 + lane;
    const bool live = loc < p.wz_cnt;
    const long long pix = p.wz_pix0 + (live ? loc : col0);
    float *const tile_rank = s_rank + (tid >> 6) * (RS::R * 64);
    rs.base = tile_rank;
    rs.stride = 64;
    rs.p = lane;
    wz_prepare1_sorted<RSL, true>(v, kept, p.nframes, rs, W1, W2, c0);
    int rl = 0, rh = 0;
    if (live) {
        int route = 2;
        PixOut o;
        WzState st;
        if (!bad && kept > 0) {
            const int N = p.nframes;
            const int el = (N + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);   // the prep's slots (G = 1)
            route = wz_finish_cap<0>(rs, kept, W1, W2, c0, el, p.sig0, p.sig1, sp.cap, o, st);
        }
        if (route == kWzDeferred) {
            // as the head: state, compact copy of the ranks, striped list
            // entry -- and what the prep kernel would have left for the tail
            const unsigned long long dm = __ballot(true);
            const int ci = (int)__popcll(dm & ((1ull << lane) - 1ull));
            const int tw = (int)(p.wz_cnt - col0 < 64 ? p.wz_cnt - col0 : 64);
            const int stripe = (int)tile / sp.bps;
            const int slot = wave_append(sp.cnt_out + stripe * kWzStripeStep, true);
            sp.list_out[stripe * sp.bps * 64 + slot] = wz_entry((int)tile, ci, lane);
            reinterpret_cast<WzState *>(p.wz_state)[loc] = st;
            p.wz_mom[loc] = W1;
            p.wz_mom[p.wz_cnt + loc] = W2;
            p.wz_mom[2 * p.wz_cnt + loc] = (double)c0;
            reinterpret_cast<int4 *>(p.wz_meta)[loc] = make_int4(kept, rs.hi0, rs.mid0, rs.mid1);
            if (tw == 64 && (p.wz_cnt & 3) == 0) {
                const unsigned cnt = (unsigned)p.wz_cnt, c0w = (unsigned)col0;
#pragma unroll 2
                for (int j = 0; j < RS::R; j += 4) {
                    const unsigned f = (unsigned)(ci * RS::R + j);
                    const float4 q = make_float4(tile_rank[j * 64 + lane], tile_rank[(j + 1) * 64 + lane],
                                                 tile_rank[(j + 2) * 64 + lane], tile_rank[(j + 3) * 64 + lane]);
                    *reinterpret_cast<float4 *>(p.wz_ranks + (umul24(f >> 6, cnt) + c0w + (f & 63u))) = q;
                }
            } else {
#pragma unroll 4
                for (int j = 0; j < RS::R; j++)
                    p.wz_ranks[wz_crec_index(ci * RS::R + j, tw, p.wz_cnt, col0)] = tile_rank[j * 64 + lane];
            }
        } else if (route == 1) {
            const int slot = wave_append(p.fb2_count, true);
            p.fb2_list[slot] = (int)pix;
        } else if (route == 2) {
            const int slot = wave_append(p.fb_count, true);
            p.fb_list[slot] = (int)pix;
        } else {
            double res = o.res;
            if (is_weighted(p)) res = weighted_mean<0>(p, pix, (int)(pix % p.W), o.pmin, o.pmax, o.nkept);
            write_result(p, pix, res, o.rl, o.rh);
            rl = o.rl;
            rh = o.rh;
        }
    }
    add_counts(p, rl, rh);
}

// Tail pass of the split rounds: the pixels the pass before handed on, read
// from its striped list (WzSplit).  One wave per block, as the head: the wave
// stages the rank slots of 64 listed pixels in LDS (from the compact copies
// the head left in its tiles, wz_crec_index), reloads their state, rebuilds
// the constants (wz_consts) and runs
// sp.cap more rounds -- every remaining round when `last`.  A pixel ends as in
// the head: result, fallback lists, or sp.list_out again.  Block b takes
// stripe b % nstripes and every (gridDim / nstripes)-th tile of it; the
// stripe's count is read on the device (no host read-back).
// KTP: the depth of the records the head left (the fused kernel's is deeper).
template <int NP, int PG = NP / 64, int KTP = SGPU_WZ_KT>
__global__ __launch_bounds__(64) void k_stack_wz_tail(KParams p, WzSplit sp, int last) {
    using RS = RankStore<NP, 1, KTP>;
    __shared__ float s_rank[RS::R * 64];
    const int lane = (int)threadIdx.x;
    const int stripe = (int)(blockIdx.x % (unsigned)sp.nstripes);
    const int t0 = (int)(blockIdx.x / (unsigned)sp.nstripes), tstep = (int)(gridDim.x / (unsigned)sp.nstripes);
    const int seg = stripe * sp.bps * 64;
    int n = sp.cnt_in[stripe * kWzStripeStep];
    n = n < sp.bps * 64 ? n : sp.bps * 64;           // never past the stripe's entries
    if (t0 == 0 && lane == 0 && n > 0 && sp.def) atomicAdd(sp.def, n);
    int rl = 0, rh = 0;
    for (int i0 = t0 * 64; i0 < n; i0 += tstep * 64) {     // block-uniform trip count
        const bool live = i0 + lane < n;
        int ent = 0;
        if (live) ent = sp.list_in[seg + i0 + lane];
        const long long col0 = (long long)(ent >> 12) * 64;  // the head block's first pixel
        const long long loc = col0 + (ent & 63);
        int4 m = make_int4(0, 0, 0, 0);
        if (live) m = reinterpret_cast<const int4 *>(p.wz_meta)[loc];
        __syncthreads();                              // the tile before is through with s_rank
        {
            // the pixel's compact copy (wz_crec_index), every load issued
            // before the first LDS store
            float t[RS::R];
            const int tw = (int)(p.wz_cnt - col0 < 64 ? p.wz_cnt - col0 : 64);
            const int f0 = ((ent >> 6) & 63) * RS::R;
            // full tile of a chunk whose rows are 16-byte aligned: the head's
            // wide pieces; else (the chunk's partial last tile, an odd chunk) word by word
            const bool wide = tw == 64 && (p.wz_cnt & 3) == 0;
            const unsigned cnt = (unsigned)p.wz_cnt, c0w = (unsigned)col0;
#pragma unroll
            for (int j = 0; j < RS::R; j += 4) {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                const unsigned f = (unsigned)(f0 + j);
                if (live && wide)
                    q = *reinterpret_cast<const float4 *>(p.wz_ranks + (umul24(f >> 6, cnt) + c0w + (f & 63u)));
                t[j] = q.x;
                t[j + 1] = q.y;
                t[j + 2] = q.z;
                t[j + 3] = q.w;
            }
            if (live && !wide) {
#pragma unroll
                for (int j = 0; j < RS::R; j++) t[j] = p.wz_ranks[wz_crec_index(f0 + j, tw, p.wz_cnt, col0)];
            }
#pragma unroll
            for (int j = 0; j < RS::R; j++) s_rank[j * 64 + lane] = t[j];
        }
        __syncthreads();
        if (live) {
            const long long pix = p.wz_pix0 + loc;
            int route = 2;
            PixOut o;
            WzState st;
            if (m.x > 0) {
                RS rs;
                rs.base = s_rank;
                rs.stride = 64;
                rs.p = lane;
                rs.kept = m.x;
                rs.hi0 = m.y;
                rs.mid0 = m.z;
                rs.mid1 = m.w;
                constexpr int G = PG;
                const int N = p.nframes;
                const int el = (((N + G - 1) / G) + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
                WzConst k;
                float ymax, vmin;
                route = wz_consts(rs, m.x, (float)p.wz_mom[2 * p.wz_cnt + loc], G * el, p.sig0, p.sig1, k, ymax, vmin);
                st = reinterpret_cast<const WzState *>(p.wz_state)[loc];
                o.fallback = 0;
                if (!route) route = wz_rounds_cap(rs, k, st, last ? -1 : sp.cap, o);
            }
            if (route == kWzDeferred) {
                const int slot = wave_append(sp.cnt_out + stripe * kWzStripeStep, true);
                sp.list_out[seg + slot] = ent;       // its compact copy stays where it is
                reinterpret_cast<WzState *>(p.wz_state)[loc] = st;
            } else if (route == 1) {
                const int slot = wave_append(p.fb2_count, true);
                p.fb2_list[slot] = (int)pix;
            } else if (route == 2) {
                const int slot = wave_append(p.fb_count, true);
                p.fb_list[slot] = (int)pix;
            } else {
                double res = o.res;
                if (is_weighted(p)) res = weighted_mean(p, pix, (int)(pix % p.W), o.pmin, o.pmax, o.nkept);
                write_result(p, pix, res, o.rl, o.rh);
                rl += o.rl;
                rh += o.rh;
            }
        }
    }
    add_counts(p, rl, rh);
}

}  // namespace sgpu

// tests/hostsim/wz_depth_main.cpp -- TEST BUILD: the straight-line rank store
// of the fused kernel's LDS tile (stack_wz.h: RankStore::store_full_lds) at
// the fused form's depth (SGPU_WZ_KT_FUSED ranks per end, R = 48 slots)
// against the run-time slot loops (RankStore::store), on the host.
//
// store_full_lds has no range test below a region: a slot under a lane's
// range lands in the region underneath and the later, whole store of that
// region overwrites it.  That argument depends on the slot ranges, and the
// ranges on the depth; so for every real-slot bucket RSL = 72 .. 128, every
// kept in [RSL - 7, RSL] (the waves that take the straight line) and every
// lane of a tile, both stores run on the same sorted column and must leave
//   * the same R words in the lane's column of the tile, bit for bit
//     (canaries where neither stores: ranks >= kept do not exist here, kept
//     >= R, so every slot is written),
//   * the same hi0 / mid0 / mid1,
//   * every other lane's column untouched,
//   * the same answer from fetch / fetch_lo / fetch_hi for every rank, and a
//     miss exactly on the ranks outside [0, KT), [mid0, mid1), [kept - KT, kept).
// Depths 20, 18 and 16 (the two-kernel forms' record).  Distinct sample
// values per slot, so a store into a wrong row cannot pass.  Stand-alone:
// built for the host with the address and undefined-behaviour sanitizers and
// run as its own process (tests/test_wz_depth_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "stack_wz.h"

using namespace sgpu;

namespace {

long long g_cases = 0, g_bad = 0;

template <int KT, int RSL>
void run_bucket() {
    using RS = RankStore<128, 1, KT>;
    static_assert(RS::R == 2 * KT + SGPU_WZ_KM, "slots of the record");
    const uint32_t canary = 0x7fc0dead;              // a NaN no sample carries
    for (int kept = RSL - 7; kept <= RSL; kept++) {
        for (int lane = 0; lane < 64; lane += (lane % 7 == 0 ? 1 : 3)) {
            // the sorted column: ranks [0, kept) ascending and distinct, the rest +Inf
            float v[128];
            for (int e = 0; e < 128; e++)
                v[e] = e < kept ? 0.125f + 0.001f * (float)(e + 3 * lane + kept) + 0.25f * (float)e : f_inf();
            std::vector<uint32_t> ta((size_t)RS::R * 64, canary), tb((size_t)RS::R * 64, canary);
            RS a, b;
            a.base = reinterpret_cast<float *>(ta.data());
            b.base = reinterpret_cast<float *>(tb.data());
            a.stride = b.stride = 64;
            a.p = b.p = lane;
            a.kept = b.kept = kept;
            a.template store_full_lds<RSL>(v);
            // the slot loops with the bucket's extremes as the wave's range of kept
            b.store(v, 0, RSL - 7, RSL);
            bool ok = a.hi0 == b.hi0 && a.mid0 == b.mid0 && a.mid1 == b.mid1;
            ok = ok && a.hi0 == kept - KT && a.mid0 == kept / 2 - SGPU_WZ_KM / 2 && a.mid1 == a.mid0 + SGPU_WZ_KM;
            for (int j = 0; j < RS::R; j++)
                for (int l = 0; l < 64; l++) {
                    const uint32_t wa = ta[(size_t)j * 64 + l], wb = tb[(size_t)j * 64 + l];
                    if (l != lane) ok = ok && wa == canary && wb == canary;
                    else ok = ok && wa == wb && wa != canary;
                }
            for (int r = 0; r < kept; r++) {
                const bool stored = r < KT || (r >= a.mid0 && r < a.mid1) || r >= kept - KT;
                float x0 = -1.f, x1 = -1.f, x2 = -1.f, y0 = -1.f;
                const bool f0 = a.fetch(r, x0), f1 = a.fetch_lo(r, x1), f2 = a.fetch_hi(r, x2), g0 = b.fetch(r, y0);
                ok = ok && f0 == stored && f1 == stored && f2 == stored && g0 == stored;
                if (stored)
                    ok = ok && std::memcmp(&x0, &v[r], 4) == 0 && std::memcmp(&x1, &v[r], 4) == 0 &&
                         std::memcmp(&x2, &v[r], 4) == 0 && std::memcmp(&y0, &v[r], 4) == 0;
            }
            g_cases++;
            if (!ok && g_bad++ < 8) std::fprintf(stderr, "MISMATCH depth %d RSL %d kept %d lane %d\n", KT, RSL, kept, lane);
        }
    }
}

template <int KT>
void run_depth() {
    run_bucket<KT, 72>();
    run_bucket<KT, 80>();
    run_bucket<KT, 88>();
    run_bucket<KT, 96>();
    run_bucket<KT, 104>();
    run_bucket<KT, 112>();
    run_bucket<KT, 120>();
    run_bucket<KT, 128>();
}

}  // namespace

int main() {
    static_assert(SGPU_WZ_KT_FUSED == 20 || SGPU_WZ_KT_FUSED == 18 || SGPU_WZ_KT_FUSED == 16,
                  "the fused form's depth is one of those run here");
    run_depth<20>();
    run_depth<18>();
    run_depth<16>();
    std::printf("cases %lld  mismatches %lld\n", g_cases, g_bad);
    if (g_bad || g_cases < 3 * 8 * 8 * 20) {
        std::fprintf(stderr, "FAIL\n");
        return 1;
    }
    std::printf("wz_depth ok\n");
    return 0;
}

// tests/hostsim/wz_depth_count.hip -- TEST BUILD: the route of every pixel on
// the WINSORIZED moment path (stack_wz.h) at a given depth of the rank record,
// on the host: the one-lane prep with the LDS tile store (wz_prepare1<RSL,
// true>, the bucket of the launch's N) on a record of KT ranks per end, then
// every round (wz_finish; the capped head and the tail passes run the same
// rounds on the same record and end on the same route).  route[j]: 0 answered,
// 1 the register-resident sorted kernel (sgpu_last_wz_fallback counts these),
// 2 the exact kernel.  tests/test_wz_depth_gpu.py compares the GPU's fallback
// counts under the fused form (depth wz_fused_kt of the bucket) and the
// two-kernel form (depth SGPU_WZ_KT) with these.
#include "stack_wz.h"

using namespace sgpu;

namespace {

template <int KT, int RSL>
int route_of(float (&v)[128], int kept, int n, float s0, float s1) {
    using RS = RankStore<128, 1, KT>;
    static float tile[RS::R * 64];
    RS rs;
    rs.base = tile;
    rs.stride = 64;
    rs.p = 0;
    double W1, W2;
    float c0;
    wz_prepare1<RSL, true>(v, kept, n, rs, W1, W2, c0);
    PixOut o;
    const int el = (n + SGPU_STOP_GRAN - 1) & ~(SGPU_STOP_GRAN - 1);
    return wz_finish<0>(rs, kept, W1, W2, c0, el, s0, s1, o);
}

template <int KT>
int route_kt(float (&v)[128], int kept, int n, float s0, float s1) {
    switch (n <= 72 ? 72 : (n + 7) & ~7) {     // rs_pick_prep1
        case 72: return route_of<KT, 72>(v, kept, n, s0, s1);
        case 80: return route_of<KT, 80>(v, kept, n, s0, s1);
        case 88: return route_of<KT, 88>(v, kept, n, s0, s1);
        case 96: return route_of<KT, 96>(v, kept, n, s0, s1);
        case 104: return route_of<KT, 104>(v, kept, n, s0, s1);
        case 112: return route_of<KT, 112>(v, kept, n, s0, s1);
        case 120: return route_of<KT, 120>(v, kept, n, s0, s1);
        default: return route_of<KT, 128>(v, kept, n, s0, s1);
    }
}

}  // namespace

// the depth of each form's record in this build, at n frames
extern "C" int wz_depth_of(int fused, int n) {
    return fused ? wz_fused_kt(n <= 72 ? 72 : (n + 7) & ~7) : SGPU_WZ_KT;
}

// frames [n][ncol] (frame-major), 65 <= n <= 128; kt in {16, 18, 20}; returns -1 on another
extern "C" int wz_depth_routes(const float *frames, int n, long long ncol, float s0, float s1, int kt, int *route) {
    if (n < 65 || n > 128 || (kt != 16 && kt != 18 && kt != 20)) return -1;
    for (long long j = 0; j < ncol; j++) {
        float v[128];
        int kept = 0, bad = 0;
        for (int e = 0; e < 128; e++) {
            float x = f_inf();
            if (e < n) {
                x = frames[(long long)e * ncol + j];
                if (!(x - x == 0.f)) bad = 1;
                if (x == 0.f) x = f_inf();
                else kept++;
            }
            v[e] = x;
        }
        if (bad || kept == 0) route[j] = 2;
        else route[j] = kt == 16 ? route_kt<16>(v, kept, n, s0, s1)
                      : kt == 18 ? route_kt<18>(v, kept, n, s0, s1) : route_kt<20>(v, kept, n, s0, s1);
    }
    return 0;
}

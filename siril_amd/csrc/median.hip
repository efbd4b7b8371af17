// median.hip -- the median filter (`fmedian ksize modulation`; Siril's
// filters/median) of planes resident in HBM: ksize x ksize windows, 3 .. 15,
// exact.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// filter is specified in DESIGN.md 6l (M0-M5), lives in median_host.h and is
// restated in tests/median_ref.py; that restatement is the contract.  Parity
// with a Siril binary is unpinned.
//
// A median is a selection: every kernel works on the ordered keys of bkg_key
// with unsigned integer min / max and compares, never on floats (float
// min / max do not order NaN and +-0 as M2 does), and returns one of the
// window's samples with its own bits.
//
// One launch per iteration, one workgroup per 64 x 32 tile: the keys of the
// tile and a halo of r, reflected at load, in LDS; lane t of the 256 owns, in
// each of two passes, four neighbouring pixels of a row.
//   k_med_net<K>   K = 3, 5, 7.  The K + 3 columns under the lane's four windows
//                  are sorted once (shared by up to four windows each); every
//                  window then takes the median of its K sorted columns with
//                  the network of median_host.h.
//   k_med_sel<K>   K = 3 .. 15.  An exact selection by bisection over the key
//                  bits, most significant first: the median is the largest v
//                  with fewer than rank + 1 keys below it.  Column minima and
//                  maxima (shared like the sorted columns) give each window's
//                  smallest and largest key, and only the bits in which those
//                  two differ are bisected.
// Global accesses are 16 bytes per lane (8 for WORD input) when the width, the
// pointers and the strides are multiples of four samples / 16 bytes, and one
// sample per access otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "median_host.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_med_host;
using sgpu_wav_host::wav_refl;

namespace sgpu {

constexpr int MED_TILE = 64, MED_TILE_H = 32;       // a tile is 64 pixels wide and 32 high

struct MedArgs {
    const void *in;         // T samples, plane p at in + p*in_ps
    long long in_ps;
    float *out;             // plane p at out + p*out_ps
    long long out_ps;
    float modulation;
    int W, H, narrow;
};

// the tile's geometry for a window of K: the halo is widened to whole quads on the left and the right, so that
// every quad of the plane is a quad of the tile
template <int K>
struct MedGeom {
    static constexpr int R = (K - 1) / 2, R4 = (R + 3) & ~3;
    static constexpr int NQ = 1 + 2 * (R4 / 4);                 // quads a lane reads per window row
    static constexpr int PITCH = MED_TILE + 2 * R4 + 4;         // one quad of padding spreads the rows over the banks
    static constexpr int ROWS = MED_TILE_H + 2 * R;
    static constexpr int NCOL = K + 3;                          // columns under four neighbouring windows
    static constexpr int OFF = R4 - R;                          // of the first of them in the quads read
};

// The keys of the tile (tx0, ty0) and its halo, reflected (M1) at load.
template <typename T, int K, bool VEC>
__device__ __forceinline__ void med_load_tile(const MedArgs &a, uint32_t *s, int tx0, int ty0, int p) {
    using G = MedGeom<K>;
    const T *src = static_cast<const T *>(a.in) + (long long)p * a.in_ps;
    const int W = a.W, H = a.H;
    constexpr int QROW = (MED_TILE + 2 * G::R4) / 4, TOTAL = QROW * G::ROWS, NIT = (TOTAL + 255) / 256;
    // the scalar form of one quad; past the reflection's reach (columns no window of this tile reads) the index is
    // only kept inside the row
    auto by_sample = [&](int i) {
        const int ly = i / QROW, q = i - ly * QROW, gx = tx0 - G::R4 + 4 * q;
        const T *row = src + (long long)min(max(wav_refl(ty0 - G::R + ly, H), 0), H - 1) * W;
#pragma unroll
        for (int e = 0; e < 4; e++)
            s[ly * G::PITCH + 4 * q + e] = med_key_of(row[min(max(wav_refl(gx + e, W), 0), W - 1)]);
    };
    if constexpr (VEC) {
        // A lane's NIT quads are loaded without a branch between them, so that all are in flight before the first
        // is waited for: a quad that is not whole inside the plane loads the row's first one instead and is redone
        // sample by sample afterwards.
        using Q = std::conditional_t<sizeof(T) == 4, float4, ushort4>;
        Q v[NIT];
#pragma unroll
        for (int t = 0; t < NIT; t++) {
            const int i = min((int)threadIdx.x + 256 * t, TOTAL - 1), ly = i / QROW, gx = tx0 - G::R4 + 4 * (i - ly * QROW);
            const T *row = src + (long long)min(max(wav_refl(ty0 - G::R + ly, H), 0), H - 1) * W;
            v[t] = *reinterpret_cast<const Q *>(row + (gx >= 0 && gx + 3 < W ? gx : 0));
        }
#pragma unroll
        for (int t = 0; t < NIT; t++) {
            const int i = threadIdx.x + 256 * t, ly = i / QROW, q = i - ly * QROW, gx = tx0 - G::R4 + 4 * q;
            if (i < TOTAL && gx >= 0 && gx + 3 < W)
                *reinterpret_cast<uint4 *>(s + ly * G::PITCH + 4 * q) =
                    make_uint4(med_key_of(v[t].x), med_key_of(v[t].y), med_key_of(v[t].z), med_key_of(v[t].w));
        }
        for (int i = threadIdx.x; i < TOTAL; i += 256) {
            const int gx = tx0 - G::R4 + 4 * (i % QROW);
            if (gx < 0 || gx + 3 >= W) by_sample(i);
        }
    } else {
        for (int i = threadIdx.x; i < TOTAL; i += 256) by_sample(i);
    }
}

// A row is read as whole quads, 16 bytes per lane, which the LDS serves without a bank conflict at the lanes' stride
// of 16 bytes.  Left to itself the compiler drops the samples of a quad that no window uses and reads the others as
// pairs of dwords, which collide four ways on the banks (two rows of 16 quads per half wave, every address a multiple
// of four dwords); the volatile access keeps the quad whole.
typedef uint32_t med_u32x4 __attribute__((ext_vector_type(4)));

// one window row under the lane's four windows: the NQ quads around column 4*qi of the tile, row ly of the LDS
template <int K>
__device__ __forceinline__ void med_read_row(const uint32_t *s, int ly, int qi, uint32_t (&v)[4 * MedGeom<K>::NQ]) {
    using G = MedGeom<K>;
    const uint32_t *at = s + ly * G::PITCH + 4 * qi;        // the tile's column 4*qi - R4 .. of the plane
#pragma unroll
    for (int j = 0; j < G::NQ; j++) {
        const med_u32x4 q = *(const volatile __attribute__((address_space(3))) med_u32x4 *)(at + 4 * j);
        v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
    }
}

// M3 and the store of the four outputs at (x .. x+3, y)
template <bool VEC>
__device__ __forceinline__ void med_store(const MedArgs &a, int p, int x, int y, const uint32_t (&m)[4],
                                          const uint32_t (&c)[4]) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = med_modulate(a.modulation, med_unkey(m[e]), med_unkey(c[e]));
    float *dst = a.out + (long long)p * a.out_ps + (long long)y * a.W + x;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (x + e < a.W) dst[e] = o[e];
    }
}

template <typename T, int K, bool VEC>
__global__ __launch_bounds__(256) void k_med_net(MedArgs a) {
    using G = MedGeom<K>;
    __shared__ __attribute__((aligned(16))) uint32_t s[G::PITCH * G::ROWS];
    const int tx0 = blockIdx.x * MED_TILE, ty0 = blockIdx.y * MED_TILE_H, p = blockIdx.z;
    med_load_tile<T, K, VEC>(a, s, tx0, ty0, p);
    __syncthreads();
    const int qi = threadIdx.x & 15, x = tx0 + 4 * qi;
    if (x >= a.W) return;
#pragma unroll
    for (int i = 0; i < MED_TILE_H / 16; i++) {
        const int ty = (threadIdx.x >> 4) + 16 * i, y = ty0 + ty;
        if (y >= a.H) continue;
        uint32_t col[G::NCOL][K];
#pragma unroll
        for (int d = 0; d < K; d++) {
            uint32_t v[4 * G::NQ];
            med_read_row<K>(s, ty + d, qi, v);
#pragma unroll
            for (int c = 0; c < G::NCOL; c++) col[c][d] = v[G::OFF + c];
        }
        uint32_t centre[4], m[4];
#pragma unroll
        for (int e = 0; e < 4; e++) centre[e] = col[e + G::R][G::R];
#pragma unroll
        for (int c = 0; c < G::NCOL; c++) med_sort<MedKeyOp, K>(col[c]);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            uint32_t w[K][K];
#pragma unroll
            for (int c = 0; c < K; c++)
#pragma unroll
                for (int d = 0; d < K; d++) w[c][d] = col[e + c][d];
            m[e] = med_of_sorted_columns<MedKeyOp, K>(w);
        }
        med_store<VEC>(a, p, x, y, m, centre);
    }
}

template <typename T, int K, bool VEC>
__global__ __launch_bounds__(256) void k_med_sel(MedArgs a) {
    using G = MedGeom<K>;
    __shared__ __attribute__((aligned(16))) uint32_t s[G::PITCH * G::ROWS];
    const int tx0 = blockIdx.x * MED_TILE, ty0 = blockIdx.y * MED_TILE_H, p = blockIdx.z;
    med_load_tile<T, K, VEC>(a, s, tx0, ty0, p);
    __syncthreads();
    const int qi = threadIdx.x & 15, x = tx0 + 4 * qi;
    if (x >= a.W) return;
    constexpr uint32_t RANK = (K * K - 1) / 2;
#pragma unroll 1
    for (int i = 0; i < MED_TILE_H / 16; i++) {
        const int ty = (threadIdx.x >> 4) + 16 * i, y = ty0 + ty;
        if (y >= a.H) continue;
        uint32_t v[4 * G::NQ], centre[4], res[4];
        int nbits = 32;
#pragma unroll
        for (int e = 0; e < 4; e++) res[e] = 0;
        if (a.narrow) {
            // the smallest and the largest key of every window, from those of the columns
            uint32_t cmin[G::NCOL], cmax[G::NCOL];
#pragma unroll
            for (int d = 0; d < K; d++) {
                med_read_row<K>(s, ty + d, qi, v);
#pragma unroll
                for (int c = 0; c < G::NCOL; c++) {
                    cmin[c] = d ? min(cmin[c], v[G::OFF + c]) : v[G::OFF + c];
                    cmax[c] = d ? max(cmax[c], v[G::OFF + c]) : v[G::OFF + c];
                }
                if (d == G::R) {
#pragma unroll
                    for (int e = 0; e < 4; e++) centre[e] = v[G::OFF + G::R + e];
                }
            }
            nbits = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                uint32_t lo = cmin[e], hi = cmax[e];
#pragma unroll
                for (int c = 1; c < K; c++) lo = min(lo, cmin[e + c]), hi = max(hi, cmax[e + c]);
                const int nb = 32 - __clz((int)(lo ^ hi));      // __clz(0) is 32
                res[e] = nb >= 32 ? 0u : (hi >> (nb & 31)) << (nb & 31);    // the bits all keys of the window share
                nbits = max(nbits, nb);
            }
        } else {
            med_read_row<K>(s, ty + G::R, qi, v);
#pragma unroll
            for (int e = 0; e < 4; e++) centre[e] = v[G::OFF + G::R + e];
        }
        // A bit above a window's own range changes nothing: set in the shared bits, the candidate is res itself
        // (no key is below it); clear, the candidate is above every key.
#pragma unroll 1
        for (int b = nbits - 1; b >= 0; b--) {
            uint32_t cand[4], cnt[4];
#pragma unroll
            for (int e = 0; e < 4; e++) cand[e] = res[e] | (1u << b), cnt[e] = 0;
#pragma unroll
            for (int d = 0; d < K; d++) {
                med_read_row<K>(s, ty + d, qi, v);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int c = 0; c < K; c++) cnt[e] += v[G::OFF + e + c] < cand[e];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) res[e] = cnt[e] <= RANK ? cand[e] : res[e];
        }
        med_store<VEC>(a, p, x, y, res, centre);
    }
}

}  // namespace sgpu

// ===================================================================== host
namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// true when the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const char *a0 = (const char *)a, *b0 = (const char *)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

template <typename T, int K, bool VEC>
void launch_one(sgpu_context *c, const sgpu::MedArgs &a, int P, bool net) {
    const dim3 grid((unsigned)((a.W + sgpu::MED_TILE - 1) / sgpu::MED_TILE),
                    (unsigned)((a.H + sgpu::MED_TILE_H - 1) / sgpu::MED_TILE_H), (unsigned)P);
    if constexpr (K <= SGPU_FMEDIAN_MAX_NETWORK_KSIZE) {
        if (net) {
            hipLaunchKernelGGL((sgpu::k_med_net<T, K, VEC>), grid, dim3(256), 0, c->stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((sgpu::k_med_sel<T, K, VEC>), grid, dim3(256), 0, c->stream, a);
}

template <typename T, bool VEC>
void launch_k(sgpu_context *c, const sgpu::MedArgs &a, int P, int ksize, bool net) {
    switch (ksize) {
        case 3: return launch_one<T, 3, VEC>(c, a, P, net);
        case 5: return launch_one<T, 5, VEC>(c, a, P, net);
        case 7: return launch_one<T, 7, VEC>(c, a, P, net);
        case 9: return launch_one<T, 9, VEC>(c, a, P, net);
        case 11: return launch_one<T, 11, VEC>(c, a, P, net);
        case 13: return launch_one<T, 13, VEC>(c, a, P, net);
        default: return launch_one<T, 15, VEC>(c, a, P, net);
    }
}

// 16-byte global accesses (8 for WORD) when both ends of the launch allow them, one sample per access otherwise
template <typename T>
void launch_v(sgpu_context *c, const sgpu::MedArgs &a, int P, int ksize, bool net, bool vec) {
    if (vec) return launch_k<T, true>(c, a, P, ksize, net);
    return launch_k<T, false>(c, a, P, ksize, net);
}

}  // namespace

extern "C" int sgpu_fmedian_check(int width, int height, int ksize, float modulation, int iterations) {
    if (const char *why = med_check(width, height, ksize, modulation, iterations)) return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_fmedian_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width,
                                          int height, long plane_stride, int ksize, float modulation, int iterations,
                                          int route, float *d_out, long out_stride) {
    if (!c) return fail(SGPU_BAD_ARGUMENT, "fmedian: no context");
    if (const char *why = med_check(width, height, ksize, modulation, iterations)) return fail(SGPU_BAD_ARGUMENT, why);
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "fmedian: element size must be 2 or 4");
    if (nplanes < 0 || nplanes > 65535) return fail(SGPU_BAD_ARGUMENT, "fmedian: bad number of planes");
    const size_t npix = (size_t)width * height;
    if (plane_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "fmedian: plane_stride < width*height");
    if (out_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "fmedian: out_stride < width*height");
    if (route < SGPU_FMEDIAN_ROUTE_AUTO || route > SGPU_FMEDIAN_ROUTE_SELECT_WIDE)
        return fail(SGPU_BAD_ARGUMENT, "fmedian: route must be 0 .. 3");
    if (route == SGPU_FMEDIAN_ROUTE_NETWORK && ksize > SGPU_FMEDIAN_MAX_NETWORK_KSIZE)
        return fail(SGPU_BAD_ARGUMENT, "fmedian: no network for that ksize");
    c->med_launches = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "fmedian: null planes");
    if (overlaps(d_in, ((size_t)(nplanes - 1) * plane_stride + npix) * elem_size, d_out,
                 ((size_t)(nplanes - 1) * out_stride + npix) * sizeof(float)))
        return fail(SGPU_BAD_ARGUMENT, "fmedian: the output overlaps the input");
    HIP_TRY(hipSetDevice(c->device));
    const long long ws_ps = ((long long)npix + 3) & ~3LL;
    if (iterations > 1)
        if (int r = c->med_ws.ensure((size_t)2 * nplanes * ws_ps * sizeof(float))) return r;
    float *ws[2] = {(float *)c->med_ws.p, (float *)c->med_ws.p + (size_t)nplanes * ws_ps};
    const bool net = route == SGPU_FMEDIAN_ROUTE_NETWORK ||
                     (route == SGPU_FMEDIAN_ROUTE_AUTO && ksize <= SGPU_FMEDIAN_MAX_NETWORK_KSIZE);
    const int vec_in = width % 4 == 0 && aligned16(d_in) && plane_stride % 4 == 0;
    const int vec_out = width % 4 == 0 && aligned16(d_out) && out_stride % 4 == 0;
    sgpu::MedArgs a = {};
    a.modulation = modulation, a.W = width, a.H = height, a.narrow = route != SGPU_FMEDIAN_ROUTE_SELECT_WIDE;
    for (int t = 0; t < iterations; t++) {
        const bool first = t == 0, last = t == iterations - 1;
        a.in = first ? d_in : (const void *)ws[(t - 1) & 1];
        a.in_ps = first ? plane_stride : ws_ps;
        a.out = last ? d_out : ws[t & 1];
        a.out_ps = last ? out_stride : ws_ps;
        const bool vec = width % 4 == 0 && (!first || vec_in) && (!last || vec_out);
        if (!c->med_ev[t]) HIP_TRY(hipEventCreate(&c->med_ev[t]));
        HIP_TRY(hipEventRecord(c->med_ev[t], c->stream));
        c->med_what[t] = 100 * (net ? SGPU_FMEDIAN_ROUTE_NETWORK : a.narrow ? SGPU_FMEDIAN_ROUTE_SELECT : SGPU_FMEDIAN_ROUTE_SELECT_WIDE) + ksize;
        if (first && elem_size == 2)
            launch_v<uint16_t>(c, a, nplanes, ksize, net, vec);
        else
            launch_v<float>(c, a, nplanes, ksize, net, vec);
        HIP_TRY(hipGetLastError());
    }
    if (!c->med_ev[iterations]) HIP_TRY(hipEventCreate(&c->med_ev[iterations]));
    HIP_TRY(hipEventRecord(c->med_ev[iterations], c->stream));
    c->med_launches = iterations;
    return SGPU_OK;
}

extern "C" int sgpu_fmedian_last_kernel_ms(sgpu_context *c, float *ms, int *what, int *nlaunches) {
    if (!c || !ms || !what || !nlaunches) return fail(SGPU_BAD_ARGUMENT, "fmedian_last_kernel_ms: null argument");
    *nlaunches = c->med_launches;
    if (!c->med_launches) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->med_ev[c->med_launches]));
    for (int k = 0; k < c->med_launches; k++) {
        HIP_TRY(hipEventElapsedTime(&ms[k], c->med_ev[k], c->med_ev[k + 1]));
        what[k] = c->med_what[k];
    }
    return SGPU_OK;
}

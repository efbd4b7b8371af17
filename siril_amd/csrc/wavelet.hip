// wavelet.hip -- a trous ("with holes") wavelet decomposition and weighted
// reconstruction (`wavelet`, `wrecons`; Siril's filters/wavelets) of planes
// resident in HBM.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// arithmetic is specified in DESIGN.md 6j (W0-W5), lives in wavelet_host.h and
// is restated in tests/wavelet_ref.py; that restatement is the contract.
// Parity with a Siril binary is unpinned.
//
// Scale j smooths c_j at step 2^j, rows first, then columns of the row result,
// into c_{j+1}, and w_j = c_j - c_{j+1}.  c_j ping-pongs in the context's
// workspace.  The launches of one call, nothing returns to the host between
// them:
//   k_wav_tile   scales 0 and 1 in one launch, one workgroup per 64 x 32 tile:
//                c_0 of the tile and a halo in LDS (only coordinates inside the
//                plane are stored; a tap that leaves the plane is reflected
//                first and looked up then), the row pass into a second LDS
//                plane, the column pass back in place, scale 0 on the region
//                scale 1 needs; four pixels of a row per lane and step.
//   k_wav_row    every further scale, where a square halo would cost more than
//   k_wav_col    a trip through memory: the row pass into the workspace, then
//                the column pass, four pixels per lane.
//   k_wav_recon  W4 on stored planes, four pixels per lane.
// Every kernel writes either w_j (transform) or updates the accumulator in
// d_out (fused reconstruction, which never writes a detail plane); both go
// through the same functions of wavelet_host.h in the same order, so the
// fused result equals the reconstruction of the stored planes bit for bit.
// Accesses are 16 bytes per lane (8 for WORD input) when the width, the
// pointers and the strides are multiples of four samples / 16 bytes, and one
// sample per access otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sgpu_internal.h"
#include "wavelet_host.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_wav_host;

namespace sgpu {

constexpr int WAV_TILE = 64, WAV_TILE_H = 32;     // a tile is 64 pixels wide and 32 high
constexpr int WAV_GROUP = 2;        // scales 0 and 1 share the tiled launch, the others run as a row and a column launch
                                    // (the table of forms)

struct WavCoef {
    float k[WAV_MAX_LAYERS];
};

struct WavTile {
    const void *in;         // the input: T samples, plane p at in + p*in_ps
    long long in_ps;
    float *cnext;           // c_{ns}, plane p at cnext + p*ws_ps; not written by the last launch
    long long ws_ps;
    float *out;             // transform: plane k of image p at out + p*out_is + k*out_ps; fused: the accumulator at out + p*out_is
    long long out_ps, out_is;
    WavCoef coef;
    int W, H, type, n, ns, halo, pitch, rows, vec;
};

__device__ __forceinline__ float4 wav_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void wav_st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

__device__ __forceinline__ float4 wav_smooth4(int type, const float4 &m2, const float4 &m1, const float4 &c,
                                              const float4 &p1, const float4 &p2) {
    return make_float4(wav_smooth(type, m2.x, m1.x, c.x, p1.x, p2.x), wav_smooth(type, m2.y, m1.y, c.y, p1.y, p2.y),
                       wav_smooth(type, m2.z, m1.z, c.z, p1.z, p2.z), wav_smooth(type, m2.w, m1.w, c.w, p1.w, p2.w));
}

// four values to / from global memory at x .. x+3 of a row that ends at xend
__device__ __forceinline__ void wav_store_quad(float *dst, const float (&v)[4], int x, int xend, int vec) {
    if (vec) {
        wav_st4(dst, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (x + e < xend) dst[e] = v[e];
    }
}
__device__ __forceinline__ void wav_load_quad(const float *src, float (&v)[4], int x, int xend, int vec) {
    if (vec) {
        const float4 q = wav_ld4(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = x + e < xend ? src[e] : 0.0f;
    }
}

// One row quad of the tile's row pass at step S (1 or 2): the three aligned quads around x hold every tap.
template <int S>
__device__ __forceinline__ float4 wav_row_quad(int type, const float *at) {
    const float4 l = wav_ld4(at - 4), m = wav_ld4(at), r = wav_ld4(at + 4);
    const float v[12] = {l.x, l.y, l.z, l.w, m.x, m.y, m.z, m.w, r.x, r.y, r.z, r.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = wav_smooth(type, v[4 + e - 2 * S], v[4 + e - S], v[4 + e], v[4 + e + S], v[4 + e + 2 * S]);
    return make_float4(o[0], o[1], o[2], o[3]);
}

// Scales 0 .. ns-1 (ns <= 2) of a 64 x 32 tile.  Work is dealt in quads of four pixels of a row; (r, q) walks a
// region of nq quads per row 256 quads at a time without a division per quad.
#define WAV_QUADS(nq, nr)                                                        \
    for (int dq_ = 256 % (nq), dr_ = 256 / (nq), r = tid / (nq), q = tid - r * (nq); r < (nr); \
         q += dq_, r += dr_, r += q >= (nq), q -= q >= (nq) ? (nq) : 0)

// Lane t of the 256 owns, in each of two passes i, the four pixels (tx0 + 4*(t & 15) .., ty0 + (t >> 4) + 16*i)
// of the tile: its accumulators stay in registers from the first scale of the launch to the last.
template <typename T, bool FUSED>
__global__ __launch_bounds__(256) void k_wav_tile(WavTile a) {
    extern __shared__ __attribute__((aligned(16))) float s_wav[];
    const int tid = threadIdx.x, W = a.W, H = a.H, type = a.type, R = wav_radius(type), pitch = a.pitch;
    const bool b3 = type == 2;
    const int p = blockIdx.z, tx0 = blockIdx.x * WAV_TILE, ty0 = blockIdx.y * WAV_TILE_H;
    const int tx1 = min(W, tx0 + WAV_TILE), ty1 = min(H, ty0 + WAV_TILE_H);
    float *A = s_wav, *B = s_wav + a.rows * pitch;
    int h = a.halo;
    // the region that is loaded: the tile and its halo widened to whole quads and by one more quad each side
    // (the row pass reads whole quads around its taps), clipped to the plane
    const int rx0 = max(0, ((tx0 - h) & ~3) - 4), rx1 = min(W, ((tx1 + h + 3) & ~3) + 4), ry0 = max(0, ty0 - h);
    int iy0 = ry0, iy1 = min(H, ty1 + h);
    {
        const T *src = static_cast<const T *>(a.in) + (long long)p * a.in_ps;
        const int nq = (rx1 - rx0 + 3) >> 2, nr = iy1 - iy0;
        WAV_QUADS(nq, nr) {
            const int x = rx0 + 4 * q;
            const T *s = src + (long long)(iy0 + r) * W + x;
            float *d = A + r * pitch + 4 * q;
            if (a.vec) {
                if constexpr (sizeof(T) == 4) {
                    wav_st4(d, wav_ld4(reinterpret_cast<const float *>(s)));
                } else {
                    const ushort4 v = *reinterpret_cast<const ushort4 *>(s);
                    wav_st4(d, make_float4(wav_to_float(v.x), wav_to_float(v.y), wav_to_float(v.z), wav_to_float(v.w)));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (x + e < rx1) d[e] = wav_to_float(s[e]);
            }
        }
    }
    const int qx = tx0 + 4 * (tid & 15), qy = ty0 + (tid >> 4);
    const long long img = (long long)p * a.out_is;
    constexpr int NI = WAV_TILE_H / 16;
    float acc[NI][4];
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[i][e] = 0.0f;
    __syncthreads();
    for (int j = 0; j < a.ns; j++) {
        const int s = 1 << j, reach = R * s;
        h -= reach;     // the halo the scales after this one still need
        const int ox0 = max(0, tx0 - h), ox1 = min(W, tx1 + h), oy0 = max(0, ty0 - h), oy1 = min(H, ty1 + h);
        const int cx0 = ox0 & ~3, nq = (ox1 - cx0 + 3) >> 2;        // the output columns, in whole quads
        // rows: every row of the input region.  A quad whose taps stay inside the plane reads them as three
        // aligned quads; one at the plane's edge reflects tap by tap.
        WAV_QUADS(nq, iy1 - iy0) {
            const int x = cx0 + 4 * q, at = (iy0 - ry0 + r) * pitch + (x - rx0);
            if (x - 4 >= rx0 && x + 8 <= rx1 && x - reach >= 0 && x + 3 + reach < W) {
                wav_st4(B + at, s == 1 ? wav_row_quad<1>(type, A + at) : wav_row_quad<2>(type, A + at));
            } else {
                const float *row = A + (iy0 - ry0 + r) * pitch - rx0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int xe = x + e;
                    if (xe < ox0 || xe >= ox1) continue;
                    const float m2 = b3 ? row[wav_refl(xe - 2 * s, W)] : 0.0f, p2 = b3 ? row[wav_refl(xe + 2 * s, W)] : 0.0f;
                    B[at + e] = wav_smooth(type, m2, row[wav_refl(xe - s, W)], row[xe], row[wav_refl(xe + s, W)], p2);
                }
            }
        }
        __syncthreads();
        // columns, the tile's own pixels: c_{j+1} replaces c_j in place, w_j leaves
        const float kj = a.coef.k[j];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int y = qy + 16 * i;
            if (y < ty1 && qx < tx1) {
                const int col = qx - rx0;
                const float4 m1 = wav_ld4(B + (wav_refl(y - s, H) - ry0) * pitch + col);
                const float4 p1 = wav_ld4(B + (wav_refl(y + s, H) - ry0) * pitch + col);
                const float4 m2 = b3 ? wav_ld4(B + (wav_refl(y - 2 * s, H) - ry0) * pitch + col) : m1;
                const float4 p2 = b3 ? wav_ld4(B + (wav_refl(y + 2 * s, H) - ry0) * pitch + col) : p1;
                const float4 t = wav_ld4(B + (y - ry0) * pitch + col), c0 = wav_ld4(A + (y - ry0) * pitch + col);
                const float4 c1 = wav_smooth4(type, m2, m1, t, p1, p2);
                wav_st4(A + (y - ry0) * pitch + col, c1);
                const float w[4] = {wav_detail(c0.x, c1.x), wav_detail(c0.y, c1.y), wav_detail(c0.z, c1.z),
                                    wav_detail(c0.w, c1.w)};
                if constexpr (FUSED) {
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[i][e] = j == 0 ? wav_first(kj, w[e]) : wav_add(acc[i][e], kj, w[e]);
                } else {
                    wav_store_quad(a.out + img + (long long)j * a.out_ps + (long long)y * W + qx, w, qx, tx1, a.vec);
                }
            }
        }
        // columns, the halo the next scale of this launch reads: the quads of the output region outside the tile
        if (h > 0) {
            WAV_QUADS(nq, oy1 - oy0) {
                const int x = cx0 + 4 * q, y = oy0 + r, col = x - rx0;
                if (x >= tx0 && x < tx1 && y >= ty0 && y < ty1) continue;
                const float4 m1 = wav_ld4(B + (wav_refl(y - s, H) - ry0) * pitch + col);
                const float4 p1 = wav_ld4(B + (wav_refl(y + s, H) - ry0) * pitch + col);
                const float4 m2 = b3 ? wav_ld4(B + (wav_refl(y - 2 * s, H) - ry0) * pitch + col) : m1;
                const float4 p2 = b3 ? wav_ld4(B + (wav_refl(y + 2 * s, H) - ry0) * pitch + col) : p1;
                wav_st4(A + (y - ry0) * pitch + col, wav_smooth4(type, m2, m1, wav_ld4(B + (y - ry0) * pitch + col), p1, p2));
            }
        }
        __syncthreads();
        iy0 = oy0, iy1 = oy1;
    }
    // the tile of c_{ns}: on to the next launch, or the residual
    const bool last = a.ns == a.n - 1;
    const float kl = a.coef.k[a.n - 1];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int y = qy + 16 * i;
        if (y < ty1 && qx < tx1) {
            const float4 c4 = wav_ld4(A + (y - ry0) * pitch + (qx - rx0));
            const float c[4] = {c4.x, c4.y, c4.z, c4.w};
            const long long at = (long long)y * W + qx;
            if (!last) wav_store_quad(a.cnext + (long long)p * a.ws_ps + at, c, qx, tx1, a.vec);
            if constexpr (FUSED) {
                if (last) {
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[i][e] = a.n == 1 ? wav_first(kl, c[e]) : wav_add(acc[i][e], kl, c[e]);
                }
                wav_store_quad(a.out + img + at, acc[i], qx, tx1, a.vec);
            } else if (last) {
                wav_store_quad(a.out + img + (long long)(a.n - 1) * a.out_ps + at, c, qx, tx1, a.vec);
            }
        }
    }
}
#undef WAV_QUADS

// The row pass of one scale on its own: t = rows of c_j smoothed, four pixels per lane.
__global__ __launch_bounds__(256) void k_wav_row(const float *c, float *t, long long ps, int W, int type, int s,
                                                 int vec) {
    const int x = 4 * (blockIdx.x * 256 + threadIdx.x), y = blockIdx.y;
    if (x >= W) return;
    const bool b3 = type == 2;
    const float *row = c + (long long)blockIdx.z * ps + (long long)y * W;
    float *dst = t + (long long)blockIdx.z * ps + (long long)y * W + x;
    const int reach = wav_radius(type) * s;
    if (vec && x - reach >= 0 && x + 3 + reach < W) {      // s is a multiple of four here: every tap is a whole quad
        const float4 m1 = wav_ld4(row + x - s), p1 = wav_ld4(row + x + s);
        const float4 m2 = b3 ? wav_ld4(row + x - 2 * s) : m1, p2 = b3 ? wav_ld4(row + x + 2 * s) : p1;
        wav_st4(dst, wav_smooth4(type, m2, m1, wav_ld4(row + x), p1, p2));
        return;
    }
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int xe = min(x + e, W - 1);
        const float m2 = b3 ? row[wav_refl(xe - 2 * s, W)] : 0.0f, p2 = b3 ? row[wav_refl(xe + 2 * s, W)] : 0.0f;
        v[e] = wav_smooth(type, m2, row[wav_refl(xe - s, W)], row[xe], row[wav_refl(xe + s, W)], p2);
    }
    wav_store_quad(dst, v, x, W, vec);
}

// The column pass of the same scale: c_{j+1} from t, then w_j or the accumulator.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_wav_col(const float *t, const float *c, float *cnext, long long ps, float *out,
                                                 long long out_ps, long long out_is, int W, int H, int type, int s,
                                                 int j, int n, float kj, float kl, int vec) {
    const int x = 4 * (blockIdx.x * 256 + threadIdx.x), y = blockIdx.y;
    if (x >= W) return;
    const bool b3 = type == 2, last = j == n - 2;
    const long long pl = (long long)blockIdx.z * ps, at = (long long)y * W + x, img = (long long)blockIdx.z * out_is;
    const float *tp = t + pl + x;
    float m2[4], m1[4], tc[4], p1[4], p2[4], c0[4], c1[4], w[4];
    wav_load_quad(tp + (long long)wav_refl(y - s, H) * W, m1, x, W, vec);
    wav_load_quad(tp + (long long)wav_refl(y + s, H) * W, p1, x, W, vec);
    wav_load_quad(tp + (long long)(b3 ? wav_refl(y - 2 * s, H) : y) * W, m2, x, W, vec);
    wav_load_quad(tp + (long long)(b3 ? wav_refl(y + 2 * s, H) : y) * W, p2, x, W, vec);
    wav_load_quad(tp + (long long)y * W, tc, x, W, vec);
    wav_load_quad(c + pl + at, c0, x, W, vec);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        c1[e] = wav_smooth(type, m2[e], m1[e], tc[e], p1[e], p2[e]);
        w[e] = wav_detail(c0[e], c1[e]);
    }
    if (!last) wav_store_quad(cnext + pl + at, c1, x, W, vec);
    if constexpr (FUSED) {
        float acc[4];
        if (j > 0) wav_load_quad(out + img + at, acc, x, W, vec);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            acc[e] = j == 0 ? wav_first(kj, w[e]) : wav_add(acc[e], kj, w[e]);
            if (last) acc[e] = wav_add(acc[e], kl, c1[e]);
        }
        wav_store_quad(out + img + at, acc, x, W, vec);
    } else {
        wav_store_quad(out + img + (long long)j * out_ps + at, w, x, W, vec);
        if (last) wav_store_quad(out + img + (long long)(n - 1) * out_ps + at, c1, x, W, vec);
    }
}

// W4 on stored planes, four pixels of the flat plane per lane.
__global__ __launch_bounds__(256) void k_wav_recon(const float *planes, long long ps, long long is, int n, WavCoef coef,
                                                   float *out, long long os, long long npix, int vec) {
    const long long i = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i >= npix) return;
    const float *src = planes + (long long)blockIdx.y * is + i;
    const int x = 0, xend = (int)min((long long)4, npix - i), v4 = vec && xend == 4;
    float acc[4], v[4];
    wav_load_quad(src, v, x, xend, v4);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] = wav_first(coef.k[0], v[e]);
    for (int k = 1; k < n; k++) {
        wav_load_quad(src + (long long)k * ps, v, x, xend, v4);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = wav_add(acc[e], coef.k[k], v[e]);
    }
    wav_store_quad(out + (long long)blockIdx.y * os + i, acc, x, xend, v4);
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

struct WavTimer {
    sgpu_context *c;
    int n = 0;
    int begin(int what) {       // before a launch
        if (n >= SGPU_WAVELET_MAX_LAUNCHES) return fail(SGPU_BAD_ARGUMENT, "wavelet: too many launches");
        if (!c->wav_ev[n]) HIP_TRY(hipEventCreate(&c->wav_ev[n]));
        HIP_TRY(hipEventRecord(c->wav_ev[n], c->stream));
        c->wav_what[n++] = what;
        return SGPU_OK;
    }
    int end() {
        HIP_TRY(hipGetLastError());
        if (!c->wav_ev[n]) HIP_TRY(hipEventCreate(&c->wav_ev[n]));
        HIP_TRY(hipEventRecord(c->wav_ev[n], c->stream));
        c->wav_launches = n;
        return SGPU_OK;
    }
};

template <typename T, bool FUSED>
int launch_tile(sgpu_context *c, sgpu::WavTile a, int P) {
    const int R = wav_radius(a.type);
    a.halo = R * ((1 << a.ns) - 1);
    a.rows = sgpu::WAV_TILE_H + 2 * a.halo;
    a.pitch = (sgpu::WAV_TILE + 2 * a.halo + 16 + 3) & ~3;      // whole quads and one more each side
    const size_t lds = (size_t)2 * a.rows * a.pitch * sizeof(float);
    if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)sgpu::k_wav_tile<T, FUSED>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    const dim3 grid((unsigned)((a.W + sgpu::WAV_TILE - 1) / sgpu::WAV_TILE),
                    (unsigned)((a.H + sgpu::WAV_TILE_H - 1) / sgpu::WAV_TILE_H), (unsigned)P);
    hipLaunchKernelGGL((sgpu::k_wav_tile<T, FUSED>), grid, dim3(256), lds, c->stream, a);
    return SGPU_OK;
}

// The launches of one transform (FUSED: into the accumulator d_out; else into the n planes at d_out).
template <typename T, bool FUSED>
int run_wavelet(sgpu_context *c, const void *d_in, int P, int W, int H, long in_ps, int n, int type,
                const sgpu::WavCoef &coef, float *d_out, long out_ps, long out_is) {
    const long long npix = (long long)W * H, ws_ps = (npix + 3) & ~3LL;
    if (n > 1)
        if (int r = c->wav_ws.ensure((size_t)3 * P * ws_ps * sizeof(float))) return r;
    float *ws[2] = {(float *)c->wav_ws.p, (float *)c->wav_ws.p + (size_t)P * ws_ps};
    float *tbuf = (float *)c->wav_ws.p + (size_t)2 * P * ws_ps;
    const int vec = W % 4 == 0 && aligned16(d_in) && in_ps % 4 == 0 && aligned16(d_out) && out_ps % 4 == 0 &&
                    out_is % 4 == 0;
    WavTimer tm{c};
    sgpu::WavTile a = {};
    a.in = d_in, a.in_ps = in_ps, a.ws_ps = ws_ps, a.out = d_out, a.out_ps = out_ps, a.out_is = out_is, a.coef = coef;
    a.W = W, a.H = H, a.type = type, a.n = n, a.vec = vec;
    a.ns = std::min(sgpu::WAV_GROUP, n - 1), a.cnext = ws[0];
    if (int r = tm.begin(a.ns)) return r;
    if (int r = launch_tile<T, FUSED>(c, a, P)) return r;
    const float *cur = ws[0];
    int flip = 1;
    const dim3 rgrid((unsigned)((W + 1023) / 1024), (unsigned)H, (unsigned)P);
    for (int j = a.ns; j < n - 1; j++, flip ^= 1) {
        const int s = 1 << j;
        if (int r = tm.begin(100 + 10 * j + 1)) return r;
        hipLaunchKernelGGL(sgpu::k_wav_row, rgrid, dim3(256), 0, c->stream, cur, tbuf, ws_ps, W, type, s,
                           vec && s % 4 == 0);
        if (int r = tm.begin(200 + 10 * j + 1)) return r;
        hipLaunchKernelGGL((sgpu::k_wav_col<FUSED>), rgrid, dim3(256), 0, c->stream, (const float *)tbuf, cur, ws[flip],
                           ws_ps, d_out, (long long)out_ps, (long long)out_is, W, H, type, s, j, n, coef.k[j],
                           coef.k[n - 1], vec);
        cur = ws[flip];
    }
    return tm.end();
}

// what every entry refuses: sizes, strides, counts
const char *check_planes(const sgpu_context *c, int elem_size, int P, int W, int H, long stride) {
    if (!c) return "wavelet: no context";
    if (elem_size != 2 && elem_size != 4) return "element size must be 2 or 4";
    if (P < 0 || P > 65535) return "wavelet: bad number of planes";
    if (W > 65535 || H > 65535 || (long long)W * H >= (1LL << 31)) return "wavelet: the plane is too large";
    if (stride < (long)W * H) return "plane_stride < width*height";
    return nullptr;
}

int check_coef(const float *coef, int n, sgpu::WavCoef *k) {
    if (!coef) return fail(SGPU_BAD_ARGUMENT, "wavelet: no coefficients");
    *k = sgpu::WavCoef{};
    for (int i = 0; i < n; i++) {
        if (!wav_finite(coef[i])) return fail(SGPU_BAD_ARGUMENT, "wavelet: a coefficient is not finite");
        k->k[i] = coef[i];
    }
    return SGPU_OK;
}

}  // namespace

extern "C" int sgpu_wavelet_check(int width, int height, int nbr_layers, int type) {
    if (const char *why = wav_check(width, height, nbr_layers, type)) return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_wavelet_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width,
                                          int height, long plane_stride, int nbr_layers, int type, float *d_planes,
                                          long out_plane_stride, long out_image_stride) {
    if (const char *why = wav_check(width, height, nbr_layers, type)) return fail(SGPU_BAD_ARGUMENT, why);
    if (const char *why = check_planes(c, elem_size, nplanes, width, height, plane_stride))
        return fail(SGPU_BAD_ARGUMENT, why);
    const size_t npix = (size_t)width * height;
    if (out_plane_stride < (long)npix || out_image_stride < (long)(nbr_layers - 1) * out_plane_stride + (long)npix)
        return fail(SGPU_BAD_ARGUMENT, "wavelet: the output planes overlap each other");
    c->wav_launches = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_planes) return fail(SGPU_BAD_ARGUMENT, "wavelet: null planes");
    const size_t in_span = ((size_t)(nplanes - 1) * plane_stride + npix) * elem_size;
    const size_t out_span =
        ((size_t)(nplanes - 1) * out_image_stride + (size_t)(nbr_layers - 1) * out_plane_stride + npix) * sizeof(float);
    if (overlaps(d_in, in_span, d_planes, out_span))
        return fail(SGPU_BAD_ARGUMENT, "wavelet: the output overlaps the input");
    HIP_TRY(hipSetDevice(c->device));
    const sgpu::WavCoef none = {};
    if (elem_size == 4)
        return run_wavelet<float, false>(c, d_in, nplanes, width, height, plane_stride, nbr_layers, type, none, d_planes,
                                         out_plane_stride, out_image_stride);
    return run_wavelet<uint16_t, false>(c, d_in, nplanes, width, height, plane_stride, nbr_layers, type, none, d_planes,
                                        out_plane_stride, out_image_stride);
}

extern "C" int sgpu_wrecons_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width,
                                          int height, long plane_stride, int nbr_layers, int type, const float *coef,
                                          float *d_out, long out_stride) {
    if (const char *why = wav_check(width, height, nbr_layers, type)) return fail(SGPU_BAD_ARGUMENT, why);
    if (const char *why = check_planes(c, elem_size, nplanes, width, height, plane_stride))
        return fail(SGPU_BAD_ARGUMENT, why);
    const size_t npix = (size_t)width * height;
    if (out_stride < (long)npix) return fail(SGPU_BAD_ARGUMENT, "out_stride < width*height");
    sgpu::WavCoef k;
    if (int r = check_coef(coef, nbr_layers, &k)) return r;
    c->wav_launches = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "wrecons: null planes");
    if (overlaps(d_in, ((size_t)(nplanes - 1) * plane_stride + npix) * elem_size, d_out,
                 ((size_t)(nplanes - 1) * out_stride + npix) * sizeof(float)))
        return fail(SGPU_BAD_ARGUMENT, "wrecons: the output overlaps the input");
    HIP_TRY(hipSetDevice(c->device));
    if (elem_size == 4)
        return run_wavelet<float, true>(c, d_in, nplanes, width, height, plane_stride, nbr_layers, type, k, d_out, 0,
                                        out_stride);
    return run_wavelet<uint16_t, true>(c, d_in, nplanes, width, height, plane_stride, nbr_layers, type, k, d_out, 0,
                                       out_stride);
}

extern "C" int sgpu_wavelet_reconstruct_device(sgpu_context *c, const float *d_planes, int nplanes, int width, int height,
                                               long plane_stride, long image_stride, int nbr_layers, const float *coef,
                                               float *d_out, long out_stride) {
    if (nbr_layers < 1 || nbr_layers > WAV_MAX_LAYERS) return fail(SGPU_BAD_ARGUMENT, "wavelet: nbr_layers must be 1 .. 6");
    if (width < 1 || height < 1) return fail(SGPU_BAD_ARGUMENT, "wavelet: empty plane");
    if (const char *why = check_planes(c, 4, nplanes, width, height, plane_stride)) return fail(SGPU_BAD_ARGUMENT, why);
    const size_t npix = (size_t)width * height;
    if (image_stride < (long)(nbr_layers - 1) * plane_stride + (long)npix || out_stride < (long)npix)
        return fail(SGPU_BAD_ARGUMENT, "wavelet: the planes overlap each other");
    sgpu::WavCoef k;
    if (int r = check_coef(coef, nbr_layers, &k)) return r;
    c->wav_launches = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_planes || !d_out) return fail(SGPU_BAD_ARGUMENT, "wavelet: null planes");
    if (overlaps(d_planes,
                 ((size_t)(nplanes - 1) * image_stride + (size_t)(nbr_layers - 1) * plane_stride + npix) * sizeof(float),
                 d_out, ((size_t)(nplanes - 1) * out_stride + npix) * sizeof(float)))
        return fail(SGPU_BAD_ARGUMENT, "wavelet: the output overlaps the planes");
    HIP_TRY(hipSetDevice(c->device));
    const int vec = aligned16(d_planes) && aligned16(d_out) && plane_stride % 4 == 0 && image_stride % 4 == 0 &&
                    out_stride % 4 == 0;
    WavTimer tm{c};
    if (int r = tm.begin(300 + nbr_layers)) return r;
    hipLaunchKernelGGL(sgpu::k_wav_recon, dim3((unsigned)((npix + 1023) / 1024), (unsigned)nplanes), dim3(256), 0,
                       c->stream, d_planes, (long long)plane_stride, (long long)image_stride, nbr_layers, k, d_out,
                       (long long)out_stride, (long long)npix, vec);
    return tm.end();
}

extern "C" int sgpu_wavelet_last_kernel_ms(sgpu_context *c, float *ms, int *what, int *nlaunches) {
    if (!c || !ms || !what || !nlaunches) return fail(SGPU_BAD_ARGUMENT, "wavelet_last_kernel_ms: null argument");
    *nlaunches = c->wav_launches;
    if (!c->wav_launches) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->wav_ev[c->wav_launches]));
    for (int k = 0; k < c->wav_launches; k++) {
        HIP_TRY(hipEventElapsedTime(&ms[k], c->wav_ev[k], c->wav_ev[k + 1]));
        what[k] = c->wav_what[k];
    }
    return SGPU_OK;
}

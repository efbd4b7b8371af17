// calibrate.hip -- the `calibrate` command's per-frame work (Siril
// core/preprocess.c preprocess() / darkOptimization(), filters/
// cosmetic_correction.c, core/arithm.c imoper / soper / siril_fdiv) on frames
// resident in HBM: bias, dark and flat in one streaming pass, the dark
// optimisation search, master preparation (region statistics, CFA
// equalisation of the flat, the deviant-pixel list) and cosmetic correction.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// arithmetic is specified in DESIGN.md "Calibration" (S1-S7) and restated in
// tests/calib_ref.py; that restatement is the contract, compared bit for bit.
// Parity with a Siril binary is unpinned.
//
// Arithmetic (float, one rounding per operation, no FMA):
//   S1  WORD v -> (float)v * (1.0f / 65535.0f)
//   S2  x -= bias[p] | level;  t = k_f * dark[p]; x -= t;
//       x = flat[p] == 0 ? 0 : norm * (x / flat[p]);  no clamp
//   S3  k_f: golden-section search on [0, 2] (15 evaluations) of sigma(S4) of
//       x_b - k * dark over the central 512 x 512 area
//   S4  n, sum, sum of squares in double over v != 0, not NaN: rows left to
//       right, then rows top to bottom
//   S5  Bayer site means over the central third, the diagonal with the closer
//       pair of means is green, the other two sites are scaled to it
//   S6  HOT: dark >= (float)(median + hot * sigma), else COLD: dark <
//       (float)(median - cold * sigma); raster order
//   S7  HOT: mean (double sum, raster order) of the in-bounds 8 neighbours at
//       `step`; COLD: quickmedian_float of the in-bounds 24; in place, in
//       list order
//
// Kernels:
//   k_calibrate_vec     8 WORD / 4 float pixels per lane, every access of a
//                       64-lane group gap-free (16-byte master loads, float
//                       loads and stores; 8-byte WORD loads); the lane's
//                       master samples stay in registers over the loop on the
//                       frames of the call, frame loads and stores are
//                       non-temporal
//   k_calibrate_scalar  the same arithmetic one pixel per lane: the tail of
//                       W*H and every call whose pointers or stride are not
//                       16-byte aligned
//   k_dark_optimize     one workgroup per frame runs the whole search: tiles
//                       of the area go through LDS, one thread per row sums
//                       its row left to right, thread 0 combines the rows in
//                       order and steps the bracket
//   k_row_sums, k_deviant_*, k_equalize_cfa   master preparation, once per
//                       master
//   k_cosmetic_level / k_cosmetic_tail   entries grouped by dependency level
//                       (an entry's level is one more than the highest level
//                       of an earlier entry inside its 5 x 5 window), one
//                       launch per level over (frame, entry); levels past
//                       CC_LEVEL_CAP run in list order on one lane per frame
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "sgpu_internal.h"

#pragma clang fp contract(off)

using sgpu_host::fail;

namespace sgpu {

typedef float cvf4 __attribute__((ext_vector_type(4)));      // nontemporal builtins take clang vectors
typedef uint32_t cvu4 __attribute__((ext_vector_type(4)));

constexpr int CAL_UNROLL = 4;       // frames whose loads are in flight together per lane
constexpr int CC_LEVEL_CAP = 32;    // dependency levels launched one by one; the rest is sequential
constexpr int DV_THREADS = 256, DV_PER_THREAD = 4, DV_CHUNK = DV_THREADS * DV_PER_THREAD;

struct CalMasters {
    const float *bias, *dark, *flat;
    const float *k;                 // per-frame dark factors (device), or null: 1
    float level, norm;
    int use_level;
};

__device__ __forceinline__ float cal_to_float(float v) { return v; }
__device__ __forceinline__ float cal_to_float(uint16_t v) { return (float)v * (1.0f / 65535.0f); }

// S2 on one sample
__device__ __forceinline__ float cal_pixel(float x, bool hb, float b, bool hd, float d, float k, bool hf, float fl,
                                           float norm) {
    if (hb) x = x - b;
    if (hd) {
        const float t = k * d;
        x = x - t;
    }
    if (hf) x = (fl == 0.0f) ? 0.0f : norm * (x / fl);
    return x;
}

// Lane l of a 64-lane group handles the pixels [g*64*PX + q*256 + 4*l, +4) for
// q < PX/4, so that every 16-byte access of the group (master loads, stores)
// covers 1 KiB without gaps; a WORD lane therefore reads its frame samples as
// two 8-byte loads 256 pixels apart, not as one 16-byte load (whose 8 pixels
// would store as two 16-byte pieces 32 bytes apart: see DESIGN.md).
template <typename T>
__global__ __launch_bounds__(256) void k_calibrate_vec(const T *in, float *out, long long nlanes, long long fstride,
                                                       int N, CalMasters m) {
    constexpr int PX = 16 / (int)sizeof(T), Q = PX / 4;
    typedef uint32_t raw_t __attribute__((ext_vector_type(sizeof(T))));      // four samples
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nlanes) return;
    const long long p0 = (v >> 6) * (64 * PX) + (v & 63) * 4;
    const bool hb = m.bias || m.use_level, hd = m.dark != nullptr, hf = m.flat != nullptr;
    cvf4 b[Q], d[Q], fl[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const long long p = p0 + q * 256;
        b[q] = cvf4{m.level, m.level, m.level, m.level};
        d[q] = cvf4{0.f, 0.f, 0.f, 0.f};
        fl[q] = cvf4{1.f, 1.f, 1.f, 1.f};
        if (m.bias) b[q] = *reinterpret_cast<const cvf4 *>(m.bias + p);
        if (hd) d[q] = *reinterpret_cast<const cvf4 *>(m.dark + p);
        if (hf) fl[q] = *reinterpret_cast<const cvf4 *>(m.flat + p);
    }
    auto frame = [&](int f, const raw_t *raw) {
        const float k = m.k ? m.k[f] : 1.0f;
        float *o = out + (long long)f * fstride + p0;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            float x[4];
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int j = 0; j < 4; j++) x[j] = __uint_as_float(raw[q][j]);
            } else {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    x[2 * j] = cal_to_float((uint16_t)(raw[q][j] & 0xffffu));
                    x[2 * j + 1] = cal_to_float((uint16_t)(raw[q][j] >> 16));
                }
            }
            cvf4 r;
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = cal_pixel(x[j], hb, b[q][j], hd, d[q][j], k, hf, fl[q][j], m.norm);
            __builtin_nontemporal_store(r, reinterpret_cast<cvf4 *>(o + q * 256));
        }
    };
    auto load = [&](int f, raw_t *raw) {
        const T *src = in + (long long)f * fstride + p0;
#pragma unroll
        for (int q = 0; q < Q; q++) raw[q] = __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(src + q * 256));
    };
    int f = 0;
    for (; f + CAL_UNROLL <= N; f += CAL_UNROLL) {
        raw_t raw[CAL_UNROLL][Q];
#pragma unroll
        for (int u = 0; u < CAL_UNROLL; u++) load(f + u, raw[u]);
#pragma unroll
        for (int u = 0; u < CAL_UNROLL; u++) frame(f + u, raw[u]);
    }
    for (; f < N; f++) {
        raw_t raw[Q];
        load(f, raw);
        frame(f, raw);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_calibrate_scalar(const T *in, float *out, long long p_begin,
                                                          long long p_end, long long fstride, int N, CalMasters m) {
    const long long p = p_begin + (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= p_end) return;
    const bool hb = m.bias || m.use_level, hd = m.dark != nullptr, hf = m.flat != nullptr;
    const float b = m.bias ? m.bias[p] : m.level, d = hd ? m.dark[p] : 0.f, fl = hf ? m.flat[p] : 1.f;
    for (int f = 0; f < N; f++) {
        const float k = m.k ? m.k[f] : 1.0f;
        const float x = cal_to_float(in[(long long)f * fstride + p]);
        out[(long long)f * fstride + p] = cal_pixel(x, hb, b, hd, d, k, hf, fl, m.norm);
    }
}

// ---- S4 ---------------------------------------------------------------------
struct RowSum {
    double n, s, q;
};

__device__ __forceinline__ void rs_add(RowSum &r, float v) {
    if (v != 0.0f && v == v) {
        r.n += 1.0;
        r.s += (double)v;
        r.q += (double)v * (double)v;
    }
}

// one thread per row of the region
__global__ __launch_bounds__(256) void k_row_sums(const float *pl, int W, int x0, int y0, int x1, int nrows, int step,
                                                  RowSum *rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    const float *row = pl + (long long)(y0 + r * step) * W;
    RowSum a = {0.0, 0.0, 0.0};
    for (int x = x0; x < x1; x += step) rs_add(a, row[x]);
    rows[r] = a;
}

// rows top to bottom -> sigma (S4's last lines)
__host__ __device__ inline void rs_combine(const RowSum *rows, int nrows, double *n_out, double *mean_out,
                                           double *sigma_out) {
    double n = 0.0, s = 0.0, q = 0.0;
#pragma unroll 8
    for (int r = 0; r < nrows; r++) {
        n += rows[r].n;
        s = s + rows[r].s;
        q = q + rows[r].q;
    }
    double mean = 0.0, sigma = 0.0;
    if (n > 0.0) {
        mean = s / n;
        const double t = q / n;
        const double mm = mean * mean;
        const double var = t - mm;
        sigma = (n > 1.0 && var > 0.0) ? sqrt(var) : 0.0;
    }
    *n_out = n;
    *mean_out = mean;
    *sigma_out = sigma;
}

// ---- S3 ---------------------------------------------------------------------
// The area is walked in tiles of DO_ROWS rows x DO_COLS columns: the workgroup
// loads a tile of v = x_b - k * dark with 16 consecutive lanes on 16
// consecutive columns (a row-per-lane walk of global memory would touch 64
// cache lines per load), then each thread adds its own row's DO_COLS samples
// from LDS, left to right, while the next tile's loads are in flight.  Same
// per-row order, same bits.
constexpr int DO_ROWS = 512, DO_COLS = 16, DO_PER_THREAD = DO_COLS;     // tile samples per thread

template <typename T>
__global__ __launch_bounds__(DO_ROWS) void k_dark_optimize(const T *in, long long fstride, int W, int ax, int ay,
                                                           int aw, int ah, const float *bias, int use_level,
                                                           float level, const float *dark, double GR,
                                                           RowSum *rows_all, float *k_out) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const T *src = in + (long long)f * fstride;
    __shared__ float tile[DO_ROWS][DO_COLS + 1];       // + 1: a row per lane reads conflict-free
    __shared__ RowSum s_rows[DO_ROWS];
    // the row sums stay in LDS when the area has at most DO_ROWS rows (thread 0
    // walks them once per evaluation)
    RowSum *rows = ah <= DO_ROWS ? s_rows : rows_all + (size_t)f * ah;
    __shared__ float s_k;
    __shared__ int s_done;
    // the bracket lives in thread 0
    float a = 0.f, b = 2.f, c = 0.f, d = 0.f;
    double fc = 0.0, fd = 0.0;
    int phase = 0;      // 0: first c, 1: first d, 2: a new c, 3: a new d
    if (tid == 0) {
        c = (float)((double)b - GR * ((double)b - (double)a));
        d = (float)((double)a + GR * ((double)b - (double)a));
        s_k = c;
        s_done = 0;
    }
    const bool hb = bias || use_level, has_plane = bias != nullptr;
    const float *bplane = has_plane ? bias : dark;      // always loadable: no control flow in the tile loads
    for (;;) {
        __syncthreads();
        if (s_done) break;
        const float k = s_k;
        for (int r0 = 0; r0 < ah; r0 += DO_ROWS) {
            RowSum acc = {0.0, 0.0, 0.0};
            float vbuf[DO_PER_THREAD];
            // this thread's DO_PER_THREAD samples of the tile at column c0: all
            // loads are independent and issued together
            auto fetch = [&](int c0) {
#pragma unroll
                for (int j = 0; j < DO_PER_THREAD; j++) {
                    // positions past the area are clamped into it (their tile
                    // cells are never read): behind a branch per sample every
                    // load waited for the one before it
                    const int e = tid + j * DO_ROWS;
                    const int rr = min(r0 + e / DO_COLS, ah - 1), cc = min(c0 + e % DO_COLS, aw - 1);
                    const long long o = (long long)(ay + rr) * W + ax + cc;
                    const float x = cal_to_float(src[o]);
                    const float bv = has_plane ? bplane[o] : level;      // a select, not a branch
                    const float xb = hb ? x - bv : x;
                    const float t = k * dark[o];
                    vbuf[j] = xb - t;
                }
            };
            fetch(0);
            for (int c0 = 0; c0 < aw; c0 += DO_COLS) {
                const int nc = min(DO_COLS, aw - c0);
#pragma unroll
                for (int j = 0; j < DO_PER_THREAD; j++) {
                    const int e = tid + j * DO_ROWS;
                    tile[e / DO_COLS][e % DO_COLS] = vbuf[j];
                }
                __syncthreads();
                if (c0 + DO_COLS < aw) fetch(c0 + DO_COLS);      // in flight under the row sums
                if (r0 + tid < ah)
                    for (int cc = 0; cc < nc; cc++) rs_add(acc, tile[tid][cc]);
                __syncthreads();
            }
            if (r0 + tid < ah) rows[r0 + tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double n, mean, noise;
            rs_combine(rows, ah, &n, &mean, &noise);
            if (phase == 0) {
                fc = noise;
                s_k = d;
                phase = 1;
            } else {
                if (phase == 2) fc = noise;
                else fd = noise;
                if (fabs((double)c - (double)d) > 1e-3) {
                    if (fc < fd) {
                        b = d;
                        d = c;
                        fd = fc;
                        c = (float)((double)b - GR * ((double)b - (double)a));
                        s_k = c;
                        phase = 2;
                    } else {
                        a = c;
                        c = d;
                        fc = fd;
                        d = (float)((double)a + GR * ((double)b - (double)a));
                        s_k = d;
                        phase = 3;
                    }
                } else {
                    k_out[f] = (a + b) * 0.5f;
                    s_done = 1;
                }
            }
        }
    }
}

// ---- S5 ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_equalize_cfa(const float *in, float *out, int W, long long npix, int s1,
                                                      float c1, int s2, float c2) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int s = (y & 1) * 2 + (x & 1);
    const float v = in[p];
    out[p] = s == s1 ? v * c1 : (s == s2 ? v * c2 : v);
}

// ---- S6 ---------------------------------------------------------------------
__device__ __forceinline__ int dv_type(float v, float th, float tc, int has_hot, int has_cold) {
    if (has_hot && v >= th) return SGPU_HOT_PIXEL;
    if (has_cold && v < tc) return SGPU_COLD_PIXEL;
    return -1;
}

__global__ __launch_bounds__(DV_THREADS) void k_deviant_count(const float *dark, long long npix, float th, float tc,
                                                              int has_hot, int has_cold, unsigned *block_cnt) {
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * DV_CHUNK + threadIdx.x * DV_PER_THREAD;
    unsigned n = 0;
    for (int j = 0; j < DV_PER_THREAD; j++)
        if (p0 + j < npix && dv_type(dark[p0 + j], th, tc, has_hot, has_cold) >= 0) n++;
    if (n) atomicAdd(&s_cnt, n);
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = s_cnt;
}

// exclusive scan of the block counts (in place), total behind them
__global__ void k_deviant_scan(unsigned *block_cnt, int nblocks) {
    if (blockIdx.x || threadIdx.x) return;
    unsigned run = 0;
    for (int i = 0; i < nblocks; i++) {
        const unsigned c = block_cnt[i];
        block_cnt[i] = run;
        run += c;
    }
    block_cnt[nblocks] = run;
}

__global__ __launch_bounds__(DV_THREADS) void k_deviant_write(const float *dark, long long npix, float th, float tc,
                                                              int has_hot, int has_cold, const unsigned *block_off,
                                                              int *list) {
    __shared__ unsigned s_scan[DV_THREADS];
    const long long p0 = (long long)blockIdx.x * DV_CHUNK + threadIdx.x * DV_PER_THREAD;
    int ty[DV_PER_THREAD];
    unsigned n = 0;
    for (int j = 0; j < DV_PER_THREAD; j++) {
        ty[j] = p0 + j < npix ? dv_type(dark[p0 + j], th, tc, has_hot, has_cold) : -1;
        n += ty[j] >= 0;
    }
    s_scan[threadIdx.x] = n;
    __syncthreads();
    for (int off = 1; off < DV_THREADS; off <<= 1) {        // inclusive scan over the threads
        const unsigned add = threadIdx.x >= (unsigned)off ? s_scan[threadIdx.x - off] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    size_t w = (size_t)block_off[blockIdx.x] + s_scan[threadIdx.x] - n;
    for (int j = 0; j < DV_PER_THREAD; j++)
        if (ty[j] >= 0) {
            list[2 * w] = (int)(p0 + j);
            list[2 * w + 1] = ty[j];
            w++;
        }
}

// ---- S7 ---------------------------------------------------------------------
// sortnet_median_float's comparator lists (Siril sorting.c), sizes 2..8
__constant__ unsigned char cc_net[] = {
    /* 2 */ 0, 1,
    /* 3 */ 0, 1, 1, 2, 0, 1,
    /* 4 */ 0, 1, 2, 3, 0, 2, 1, 3, 1, 2,
    /* 5 */ 0, 1, 2, 3, 1, 3, 2, 4, 0, 2, 1, 4, 1, 2, 3, 4, 2, 3,
    /* 6 */ 0, 1, 2, 3, 4, 5, 0, 2, 3, 5, 1, 4, 0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 2, 3,
    /* 7 */ 1, 2, 3, 4, 5, 6, 0, 2, 4, 6, 3, 5, 2, 6, 1, 5, 0, 4, 2, 5, 0, 3, 2, 4, 1, 3, 0, 1, 2, 3, 4, 5,
    /* 8 */ 0, 1, 2, 3, 4, 5, 6, 7, 0, 2, 1, 3, 4, 6, 5, 7, 1, 2, 5, 6, 0, 4, 1, 5, 2, 6, 3, 7, 2, 4, 3, 5, 1, 2, 3,
    4, 5, 6};
__constant__ int cc_net_len[9] = {0, 0, 1, 3, 5, 9, 12, 16, 19};     // comparators per size
__constant__ int cc_net_off[9] = {0, 0, 0, 1, 4, 9, 18, 30, 46};     // first comparator of a size

// quickmedian_float (Siril sorting.c): sorting networks below 9 (the even
// sizes add the middle pair in float), Lomuto quickselect from 9 on
__device__ double cc_quickmedian(float *a, int n) {
    const int k = n / 2;
    if (n < 9) {
        if (n == 1) return a[0];
        if (n < 2) return 0.0;
        const unsigned char *p = cc_net + 2 * cc_net_off[n];
        for (int c = 0; c < cc_net_len[n]; c++) {
            const int i = p[2 * c], j = p[2 * c + 1];
            if (a[i] > a[j]) {
                const float t = a[i];
                a[i] = a[j];
                a[j] = t;
            }
        }
        return (n % 2 == 0) ? (a[k - 1] + a[k]) / 2.0 : (double)a[k];
    }
    int left = 0, right = n - 1;
    while (left < right) {
        int p = (left + right) / 2;
        const float pivot = a[p];
        a[p] = a[right];
        a[right] = pivot;
        p = left;
        for (int i = left; i < right; i++) {
            if (a[i] < pivot) {
                const float t = a[p];
                a[p] = a[i];
                a[i] = t;
                p++;
            }
        }
        a[right] = a[p];
        a[p] = pivot;
        if (p < k) left = p + 1;
        else right = p;
    }
    return (n % 2 == 0) ? ((double)a[k - 1] + a[k]) / 2.0 : (double)a[k];
}

// one list entry on one frame
__device__ void cc_fix(float *img, int W, int H, int pos, int type, int step) {
    const int y = pos / W, x = pos - y * W;
    if (type == SGPU_HOT_PIXEL) {
        double sum = 0.0;
        int n = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int yy = y + dy * step, xx = x + dx * step;
                if ((dx || dy) && yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    sum += (double)img[(long long)yy * W + xx];
                    n++;
                }
            }
        if (n) img[pos] = (float)(sum / n);
    } else {
        float a[24];
        int n = 0;
        for (int dy = -2; dy <= 2; dy++)
            for (int dx = -2; dx <= 2; dx++) {
                const int yy = y + dy * step, xx = x + dx * step;
                if ((dx || dy) && yy >= 0 && yy < H && xx >= 0 && xx < W) a[n++] = img[(long long)yy * W + xx];
            }
        if (n) img[pos] = (float)cc_quickmedian(a, n);
    }
}

__global__ __launch_bounds__(64) void k_cosmetic_level(float *frames, long long fstride, int W, int H,
                                                       const int *plan, long long first, long long cnt, int step) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= cnt) return;
    const int *e = plan + 2 * (first + i);
    cc_fix(frames + (long long)blockIdx.y * fstride, W, H, e[0], e[1], step);
}

// one lane per frame, list order
__global__ __launch_bounds__(64) void k_cosmetic_tail(float *frames, long long fstride, int W, int H,
                                                      const int *plan, long long first, long long cnt, int step) {
    if (threadIdx.x) return;
    float *img = frames + (long long)blockIdx.x * fstride;
    for (long long i = 0; i < cnt; i++) {
        const int *e = plan + 2 * (first + i);
        cc_fix(img, W, H, e[0], e[1], step);
    }
}

}  // namespace sgpu

// ===================================================================== host
namespace {

bool bad_frame_args(sgpu_context *c, int nframes, int width, int height, long frame_stride) {
    return !c || nframes < 1 || nframes > 65535 || width < 1 || height < 1 ||
           (long long)width * height >= (1LL << 31) || frame_stride < (long)width * height;
}

int region_rows(sgpu_context *c, const float *d_plane, int width, int x0, int y0, int x1, int y1, int step,
                std::vector<sgpu::RowSum> &rows) {
    const int nrows = (y1 - y0 + step - 1) / step;
    rows.assign((size_t)std::max(nrows, 0), sgpu::RowSum{0.0, 0.0, 0.0});
    if (nrows <= 0 || x1 <= x0) return SGPU_OK;
    if (int r = c->cal_rows.ensure((size_t)nrows * sizeof(sgpu::RowSum))) return r;
    hipLaunchKernelGGL(sgpu::k_row_sums, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, d_plane,
                       width, x0, y0, x1, nrows, step, (sgpu::RowSum *)c->cal_rows.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rows.data(), c->cal_rows.p, (size_t)nrows * sizeof(sgpu::RowSum), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SGPU_OK;
}

// the cosmetic launch plan of a list: entries sorted by min(level, cap), list order inside
int build_cosmetic_plan(sgpu_context *c, const std::vector<int> &list, int W, int H, int cfa) {
    const long cnt = (long)list.size() / 2;
    const int step = cfa ? 2 : 1, cap = sgpu::CC_LEVEL_CAP;
    std::vector<int> level((size_t)cnt);
    std::unordered_map<int, int> last;       // position -> level of the latest entry there
    last.reserve((size_t)cnt * 2);
    for (long i = 0; i < cnt; i++) {
        const int pos = list[2 * i], y = pos / W, x = pos - y * W;
        int lv = 0;
        for (int dy = -2; dy <= 2; dy++)
            for (int dx = -2; dx <= 2; dx++) {
                const int yy = y + dy * step, xx = x + dx * step;
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                auto it = last.find(yy * W + xx);
                if (it != last.end()) lv = std::max(lv, it->second + 1);
            }
        level[(size_t)i] = lv;
        last[pos] = lv;
    }
    std::vector<long> start((size_t)cap + 2, 0);
    for (long i = 0; i < cnt; i++) start[(size_t)std::min(level[(size_t)i], cap) + 1]++;
    for (int l = 0; l <= cap; l++) start[(size_t)l + 1] += start[(size_t)l];
    std::vector<long> fill(start.begin(), start.end() - 1);
    std::vector<int> plan((size_t)cnt * 2);
    for (long i = 0; i < cnt; i++) {
        const long w = fill[(size_t)std::min(level[(size_t)i], cap)]++;
        plan[2 * (size_t)w] = list[2 * (size_t)i];
        plan[2 * (size_t)w + 1] = list[2 * (size_t)i + 1];
    }
    if (int r = c->cal_plan.ensure(plan.size() * sizeof(int))) return r;
    HIP_TRY(hipMemcpyAsync(c->cal_plan.p, plan.data(), plan.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));       // `plan` must outlive the upload
    c->h_cal_list = list;
    c->h_cal_levels = start;
    c->cal_plan_key[0] = W;
    c->cal_plan_key[1] = H;
    c->cal_plan_key[2] = cfa ? 1 : 0;
    return SGPU_OK;
}

template <typename T>
void launch_dark_optimize(sgpu_context *c, const void *d_in, int nframes, int width, int height, long frame_stride,
                          const float *d_bias, int use_level, float level, const float *d_dark, float *d_k) {
    int ax = 0, ay = 0, aw = width, ah = height;
    if (width > 512 && height > 512) {
        ax = (width - 512) / 2;
        ay = (height - 512) / 2;
        aw = ah = 512;
    }
    const double GR = (std::sqrt(5.0) - 1.0) / 2.0;
    hipLaunchKernelGGL((sgpu::k_dark_optimize<T>), dim3((unsigned)nframes), dim3(sgpu::DO_ROWS), 0, c->stream, (const T *)d_in,
                       (long long)frame_stride, width, ax, ay, aw, ah, d_bias, use_level, level, d_dark, GR,
                       (sgpu::RowSum *)c->cal_rows.p, d_k);
}

int dark_optimize(sgpu_context *c, const void *d_in, int elem_size, int nframes, int width, int height,
                  long frame_stride, const float *d_bias, int use_level, float level, const float *d_dark,
                  float *d_k) {
    const int ah = (width > 512 && height > 512) ? 512 : height;
    if (int r = c->cal_rows.ensure((size_t)nframes * ah * sizeof(sgpu::RowSum))) return r;
    if (elem_size == 4)
        launch_dark_optimize<float>(c, d_in, nframes, width, height, frame_stride, d_bias, use_level, level, d_dark,
                                    d_k);
    else
        launch_dark_optimize<uint16_t>(c, d_in, nframes, width, height, frame_stride, d_bias, use_level, level,
                                       d_dark, d_k);
    HIP_TRY(hipGetLastError());
    return SGPU_OK;
}

template <typename T>
void launch_calibrate(sgpu_context *c, const void *d_in, float *d_out, int nframes, long long npix,
                      long frame_stride, const sgpu::CalMasters &m, bool aligned) {
    constexpr int PX = 16 / (int)sizeof(T);
    // whole 64-lane groups go through the vector kernel, the rest is the scalar tail
    const long long nlanes = aligned ? npix / (64 * PX) * 64 : 0, tail0 = nlanes * PX;
    if (nlanes)
        hipLaunchKernelGGL((sgpu::k_calibrate_vec<T>), dim3((unsigned)((nlanes + 255) / 256)), dim3(256), 0, c->stream,
                           (const T *)d_in, d_out, nlanes, (long long)frame_stride, nframes, m);
    if (tail0 < npix)
        hipLaunchKernelGGL((sgpu::k_calibrate_scalar<T>), dim3((unsigned)((npix - tail0 + 255) / 256)), dim3(256), 0,
                           c->stream, (const T *)d_in, d_out, tail0, npix, (long long)frame_stride, nframes, m);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sgpu_region_stats_device(sgpu_context *c, const float *d_plane, int width, int height, int x0, int y0,
                                        int x1, int y1, int step, long *n, double *mean, double *sigma) {
    if (!c || !d_plane || width < 1 || height < 1 || x0 < 0 || y0 < 0 || x1 > width || y1 > height || x0 > x1 ||
        y0 > y1 || (step != 1 && step != 2))
        return fail(SGPU_BAD_ARGUMENT, "region stats: bad plane, region or step");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<sgpu::RowSum> rows;
    if (int r = region_rows(c, d_plane, width, x0, y0, x1, y1, step, rows)) return r;
    double dn, m, s;
    sgpu::rs_combine(rows.data(), (int)rows.size(), &dn, &m, &s);
    if (n) *n = (long)dn;
    if (mean) *mean = m;
    if (sigma) *sigma = s;
    return SGPU_OK;
}

extern "C" int sgpu_equalize_cfa_flat_device(sgpu_context *c, const float *d_flat, float *d_out, int width,
                                             int height, int pattern_size, float coef[2], int *green_diag) {
    if (!c || !d_flat || !d_out || width < 2 || height < 2 || (long long)width * height >= (1LL << 31))
        return fail(SGPU_BAD_ARGUMENT, "equalize_cfa: bad argument");
    if (pattern_size != 2)
        return fail(SGPU_BAD_ARGUMENT, "equalize_cfa: only Bayer 2 x 2 patterns (X-Trans is not supported)");
    const int x0 = (width / 3) & ~1, x1 = (2 * width / 3) & ~1, y0 = (height / 3) & ~1, y1 = (2 * height / 3) & ~1;
    double m[4];
    for (int s = 0; s < 4; s++) {
        long n;
        double sg;
        if (int r = sgpu_region_stats_device(c, d_flat, width, height, std::min(x0 + (s & 1), x1),
                                             std::min(y0 + (s >> 1), y1), x1, y1, 2, &n, &m[s], &sg))
            return r;
    }
    int s1, s2, diag;
    float c1, c2;
    if (std::fabs(1.0 - m[0] / m[3]) < std::fabs(1.0 - m[1] / m[2])) {
        diag = 0;
        s1 = 1;
        c1 = (float)(m[0] / m[1]);
        s2 = 2;
        c2 = (float)(m[0] / m[2]);
    } else {
        diag = 1;
        s1 = 0;
        c1 = (float)(m[1] / m[0]);
        s2 = 3;
        c2 = (float)(m[1] / m[3]);
    }
    const long long npix = (long long)width * height;
    hipLaunchKernelGGL(sgpu::k_equalize_cfa, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, d_flat,
                       d_out, width, npix, s1, c1, s2, c2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (coef) {
        coef[0] = c1;
        coef[1] = c2;
    }
    if (green_diag) *green_diag = diag;
    return SGPU_OK;
}

extern "C" int sgpu_find_deviant_pixels_device(sgpu_context *c, const float *d_dark, int width, int height,
                                               double cold, double hot, int *d_list, long capacity, long *count,
                                               double stats[4]) {
    if (!c || !d_dark || !count || width < 1 || height < 1 || (long long)width * height >= (1LL << 31))
        return fail(SGPU_BAD_ARGUMENT, "find_deviant_pixels: needs a master dark (null or bad argument)");
    const long long npix = (long long)width * height;
    double tab[4] = {0, 0, 0, 0};
    long ngood = 0;
    int status = 0;
    if (int r = sgpu_norm_stats_device(c, d_dark, 1, (long)npix, (long)npix, 1, tab, &ngood, &status)) return r;
    if (status) return fail(SGPU_GENERIC_ERROR, "find_deviant_pixels: the statistics of the master dark failed");
    const double median = tab[0];
    long n;
    double mean, sigma;
    if (int r = sgpu_region_stats_device(c, d_dark, width, height, 0, 0, width, height, 1, &n, &mean, &sigma))
        return r;
    const int has_hot = hot != -1.0, has_cold = cold != -1.0;
    const float th = (float)(median + hot * sigma), tc = (float)(median - cold * sigma);
    if (stats) {
        stats[0] = median;
        stats[1] = sigma;
        stats[2] = th;
        stats[3] = tc;
    }
    const int nblocks = (int)((npix + sgpu::DV_CHUNK - 1) / sgpu::DV_CHUNK);
    if (int r = c->cal_cnt.ensure(((size_t)nblocks + 1) * sizeof(unsigned))) return r;
    unsigned *cnt = (unsigned *)c->cal_cnt.p;
    hipLaunchKernelGGL(sgpu::k_deviant_count, dim3((unsigned)nblocks), dim3(sgpu::DV_THREADS), 0, c->stream, d_dark,
                       npix, th, tc, has_hot, has_cold, cnt);
    hipLaunchKernelGGL(sgpu::k_deviant_scan, dim3(1), dim3(64), 0, c->stream, cnt, nblocks);
    HIP_TRY(hipGetLastError());
    unsigned total = 0;
    HIP_TRY(hipMemcpyAsync(&total, cnt + nblocks, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *count = (long)total;
    if (d_list && total && (long)total <= capacity) {
        hipLaunchKernelGGL(sgpu::k_deviant_write, dim3((unsigned)nblocks), dim3(sgpu::DV_THREADS), 0, c->stream,
                           d_dark, npix, th, tc, has_hot, has_cold, cnt, d_list);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SGPU_OK;
}

extern "C" int sgpu_cosmetic_correction_device(sgpu_context *c, float *d_frames, int nframes, int width, int height,
                                               long frame_stride, const int *d_list, long count, int cfa) {
    if (bad_frame_args(c, nframes, width, height, frame_stride) || !d_frames || count < 0 || (count && !d_list))
        return fail(SGPU_BAD_ARGUMENT, "cosmetic correction: bad argument");
    if (count == 0) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> list((size_t)count * 2);
    HIP_TRY(hipMemcpyAsync(list.data(), d_list, list.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool same = c->cal_plan_key[0] == width && c->cal_plan_key[1] == height &&
                      c->cal_plan_key[2] == (cfa ? 1 : 0) && c->h_cal_list == list;
    if (!same) {
        const long long npix = (long long)width * height;
        for (long i = 0; i < count; i++)
            if (list[2 * (size_t)i] < 0 || list[2 * (size_t)i] >= npix ||
                (list[2 * (size_t)i + 1] != SGPU_COLD_PIXEL && list[2 * (size_t)i + 1] != SGPU_HOT_PIXEL))
                return fail(SGPU_BAD_ARGUMENT, "cosmetic correction: list entry outside the frame or of unknown type");
        c->h_cal_list.clear();
        if (int r = build_cosmetic_plan(c, list, width, height, cfa)) return r;
    }
    const int step = cfa ? 2 : 1, cap = sgpu::CC_LEVEL_CAP;
    const int *plan = (const int *)c->cal_plan.p;
    const std::vector<long> &st = c->h_cal_levels;
    for (int l = 0; l < cap; l++) {
        const long cnt = st[(size_t)l + 1] - st[(size_t)l];
        if (cnt <= 0) break;      // levels are dense: an empty one ends them
        hipLaunchKernelGGL(sgpu::k_cosmetic_level, dim3((unsigned)((cnt + 63) / 64), (unsigned)nframes), dim3(64), 0,
                           c->stream, d_frames, (long long)frame_stride, width, height, plan, (long long)st[(size_t)l],
                           (long long)cnt, step);
    }
    const long tail = st[(size_t)cap + 1] - st[(size_t)cap];
    if (tail > 0)
        hipLaunchKernelGGL(sgpu::k_cosmetic_tail, dim3((unsigned)nframes), dim3(64), 0, c->stream, d_frames,
                           (long long)frame_stride, width, height, plan, (long long)st[(size_t)cap], (long long)tail,
                           step);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SGPU_OK;
}

extern "C" int sgpu_dark_optimize_device(sgpu_context *c, const void *d_in, int elem_size, int nframes, int width,
                                         int height, long frame_stride, const float *d_bias, int use_level,
                                         float bias_level, const float *d_dark, float *d_k, float *k_host) {
    if (bad_frame_args(c, nframes, width, height, frame_stride) || !d_in || (!d_k && !k_host))
        return fail(SGPU_BAD_ARGUMENT, "dark optimisation: bad argument");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (!d_dark) return fail(SGPU_BAD_ARGUMENT, "dark optimisation needs a master dark");
    HIP_TRY(hipSetDevice(c->device));
    if (!d_k) {
        if (int r = c->cal_k.ensure((size_t)nframes * sizeof(float))) return r;
        d_k = (float *)c->cal_k.p;
    }
    if (int r = dark_optimize(c, d_in, elem_size, nframes, width, height, frame_stride, d_bias, use_level,
                              bias_level, d_dark, d_k))
        return r;
    if (k_host) {
        HIP_TRY(hipMemcpyAsync(k_host, d_k, (size_t)nframes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SGPU_OK;
}

extern "C" int sgpu_calibrate_frames_device(sgpu_context *c, const void *d_in, float *d_out, int elem_size,
                                            int nframes, int width, int height, long frame_stride,
                                            const float *d_bias, int use_level, float bias_level,
                                            const float *d_dark, const float *d_flat, float norm, float *d_k,
                                            const int *d_list, long count, int cfa, int dark_optim) {
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (!c || !d_in || !d_out || nframes < 1 || nframes > 65535 || width < 1 || height < 1 ||
        (long long)width * height >= (1LL << 31) || count < 0)
        return fail(SGPU_BAD_ARGUMENT, "calibrate: bad argument");
    if (frame_stride < (long)width * height) return fail(SGPU_BAD_ARGUMENT, "frame_stride < width*height");
    const long long npix = (long long)width * height;
    const size_t span = (size_t)(nframes - 1) * (size_t)frame_stride + (size_t)npix;
    const char *i0 = (const char *)d_in, *i1 = i0 + span * (size_t)elem_size;
    const char *o0 = (const char *)d_out, *o1 = o0 + span * sizeof(float);
    if (i0 < o1 && o0 < i1 && !(elem_size == 4 && i0 == o0))
        return fail(SGPU_BAD_ARGUMENT, "calibrate: the output overlaps the input (in place only for float frames)");
    if (dark_optim && !d_dark) return fail(SGPU_BAD_ARGUMENT, "dark optimisation needs a master dark");
    if (d_list && count > 0 && !d_dark)
        return fail(SGPU_BAD_ARGUMENT, "cosmetic correction from the dark needs a master dark");
    HIP_TRY(hipSetDevice(c->device));
    if (dark_optim) {
        if (!d_k) {
            if (int r = c->cal_k.ensure((size_t)nframes * sizeof(float))) return r;
            d_k = (float *)c->cal_k.p;
        }
        if (int r = dark_optimize(c, d_in, elem_size, nframes, width, height, frame_stride, d_bias, use_level,
                                  bias_level, d_dark, d_k))
            return r;
    }
    sgpu::CalMasters m;
    m.bias = d_bias;
    m.dark = d_dark;
    m.flat = d_flat;
    m.k = d_dark ? d_k : nullptr;
    m.level = bias_level;
    m.norm = norm;
    m.use_level = (!d_bias && use_level) ? 1 : 0;
    const bool aligned = aligned16(d_in) && aligned16(d_out) && ((size_t)frame_stride * (size_t)elem_size) % 16 == 0 &&
                         ((size_t)frame_stride * sizeof(float)) % 16 == 0 && aligned16(d_bias) && aligned16(d_dark) &&
                         aligned16(d_flat);
    if (elem_size == 4) launch_calibrate<float>(c, d_in, d_out, nframes, npix, frame_stride, m, aligned);
    else launch_calibrate<uint16_t>(c, d_in, d_out, nframes, npix, frame_stride, m, aligned);
    HIP_TRY(hipGetLastError());
    if (d_list && count > 0)
        return sgpu_cosmetic_correction_device(c, d_out, nframes, width, height, frame_stride, d_list, count, cfa);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SGPU_OK;
}

// stars.hip -- star detection for star-based global registration (SURVEY 2
// row 12): one streaming pass over every frame finds the candidates
// (smoothing, threshold, local maximum, extents), a small kernel measures
// them with thresholded image moments.
//
// PARITY STATUS: Siril's source was not available.  The arithmetic is modelled
// on Siril's star_finder.c (threshold bg + ksigma * bgnoise, smoothed local
// maximum within `radius`, ties by raster order, roundness filter) with the
// Levenberg-Marquardt PSF fit replaced by image moments; it is specified in
// DESIGN.md 6f and restated in tests/star_ref.py, which is the contract.
// Parity with Siril itself is unpinned.
//
// Arithmetic (samples and smoothing float, moments double, no FMA):
//   table   t[k] = exp(-k^2 / 2 sigma^2), k = -K..K, K = ceil(3 sigma), over
//           the double sum, cast to float (K = 0: t = {1})
//   smooth  h = ((t0 p[x-K] + t1 p[x-K+1]) + ...), then the same down the rows
//   thr     (float)(bg + ksigma * noise)
//   candidate (interior: r+K <= x < W-(r+K), same in y): s > thr, no greater
//           smoothed value in the (2r+1)^2 window, no equal one earlier in
//           raster order
//   extents walk -x, +x, -y, +y on s: k steps while k < r, s(next) < s(cur),
//           s(next) > thr; extent min(r, k + 1)
//   moments on the raw box, v = p - bg, pixels with v > cut * A; rows summed
//           left to right from 0.0, row partials added rows ascending
//
// k_star_candidates: one 256-thread workgroup per 64 x 16 tile, frame in
// blockIdx.z.  The tile plus an (r+K) halo is loaded into LDS (coalesced
// rows), the horizontal pass writes a second plane, the vertical pass writes
// back over the first; threshold, window scan and walks read that plane.
// Candidates of a tile are at least r+1 apart (Chebyshev), so a tile has a
// fixed number of slots and its own count: no cross-workgroup atomics.
// k_star_measure: one thread per slot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sgpu_internal.h"

#pragma clang fp contract(off)

namespace sgpu {

constexpr int ST_TW = 64, ST_TH = 16;     // tile
constexpr int ST_MAXR = 16, ST_MAXK = 6;

struct StarTab {
    float t[2 * ST_MAXK + 1];
};
struct StarFrame {       // per-frame constants, computed on the host
    double bg, amin;     // background, min_amp * noise
    float thr, pad;
};
struct StarCand {        // one slot
    int x, y, ext, pad;  // ext: e0 | e1 << 8 | e2 << 16 | e3 << 24
};

__host__ __device__ constexpr int star_slots_1d(int len, int r) { return (len + r) / (r + 1); }

template <typename T, int K>
__global__ __launch_bounds__(256) void k_star_candidates(const T *in, int W, int H, long long rstride,
                                                         long long fstride, int r, StarTab tab,
                                                         const StarFrame *fp, int *tcount, StarCand *slots,
                                                         int nslots) {
    extern __shared__ float s_mem[];
    __shared__ int s_cnt;
    const int P = r + K;
    const int RW = ST_TW + 2 * P, RH = ST_TH + 2 * P;   // raw plane
    const int SW = ST_TW + 2 * r, SH = ST_TH + 2 * r;   // smoothed plane
    const int rp = RW | 1, sp = SW | 1;                 // odd pitches
    float *s_a = s_mem;                                 // raw, then smoothed
    float *s_b = s_mem + RH * rp;                       // horizontal pass
    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * ST_TW, y0 = blockIdx.y * ST_TH;
    const int tile = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * f);
    if (tid == 0) s_cnt = 0;
    // interior of the frame and its part in this tile (uniform)
    const int ix0 = max(x0, P), ix1 = min(x0 + ST_TW, W - P);
    const int iy0 = max(y0, P), iy1 = min(y0 + ST_TH, H - P);
    if (ix0 >= ix1 || iy0 >= iy1) {
        if (tid == 0) tcount[tile] = 0;
        return;
    }
    const T *fin = in + (long long)f * fstride;
    const float thr = fp[f].thr;
    // raw plane: frame rows y0-P .., columns x0-P ..; samples outside the frame are never used
    // (rr, c) of idx = tid + 256 i advance without a division per element
    const int rdq = 256 / RW, rdr = 256 - rdq * RW;
    // eight loads in flight per lane, coordinates clamped into the frame (branch-free, always a
    // valid address; what a clamped position holds is never used)
    constexpr int LD = 8;
    for (int idx = tid, rr = tid / RW, c = tid - rr * RW; idx < RH * RW; idx += 256 * LD) {
        float v[LD];
        int o[LD];
#pragma unroll
        for (int u = 0; u < LD; u++) {
            const int yy = min(max(y0 - P + rr, 0), H - 1), xx = min(max(x0 - P + c, 0), W - 1);
            v[u] = (float)fin[(long long)yy * rstride + xx];
            o[u] = idx + 256 * u < RH * RW ? rr * rp + c : -1;
            c += rdr;
            rr += rdq;
            if (c >= RW) {
                c -= RW;
                rr++;
            }
        }
#pragma unroll
        for (int u = 0; u < LD; u++)
            if (o[u] >= 0) s_a[o[u]] = v[u];
    }
    __syncthreads();
    // horizontal: h[rr][c] is column x0 - r + c of raw row rr
    const int sdq = 256 / SW, sdr = 256 - sdq * SW;
    for (int idx = tid, rr = tid / SW, c = tid - rr * SW; idx < RH * SW; idx += 256) {
        const float *p = s_a + rr * rp + c;
        float h = tab.t[0] * p[0];
#pragma unroll
        for (int j = 1; j <= 2 * K; j++) h = h + tab.t[j] * p[j];
        s_b[rr * sp + c] = h;
        c += sdr;
        rr += sdq;
        if (c >= SW) {
            c -= SW;
            rr++;
        }
    }
    __syncthreads();
    // vertical: s[rr][c] is row y0 - r + rr, column x0 - r + c
    for (int idx = tid, rr = tid / SW, c = tid - rr * SW; idx < SH * SW; idx += 256) {
        const float *p = s_b + rr * sp + c;
        float s = tab.t[0] * p[0];
#pragma unroll
        for (int j = 1; j <= 2 * K; j++) s = s + tab.t[j] * p[j * sp];
        s_a[rr * sp + c] = s;
        c += sdr;
        rr += sdq;
        if (c >= SW) {
            c -= SW;
            rr++;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < ST_TH / 4; k++) {
        const int lx = tid & 63, ly = (tid >> 6) + 4 * k;
        const int x = x0 + lx, y = y0 + ly;
        if (x < ix0 || x >= ix1 || y < iy0 || y >= iy1) continue;
        const float *c = s_a + (ly + r) * sp + (lx + r);
        const float s = *c;
        if (!(s > thr)) continue;
        // the eight neighbours first: most pixels above the threshold fail here
        bool top = !(c[-sp - 1] >= s) && !(c[-sp] >= s) && !(c[-sp + 1] >= s) && !(c[-1] >= s) && !(c[1] > s) &&
                   !(c[sp - 1] > s) && !(c[sp] > s) && !(c[sp + 1] > s);
        if (!top) continue;
        for (int dy = -r; dy <= r && top; dy++) {
            const float *row = c + dy * sp;
            for (int dx = -r; dx <= r; dx++) {
                const float n = row[dx];
                const bool earlier = dy < 0 || (dy == 0 && dx < 0);
                if (n > s || (earlier && n == s)) {
                    top = false;
                    break;
                }
            }
        }
        if (!top) continue;
        int e[4];
        const int step[4] = {-1, 1, -sp, sp};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            int kk = 0;
            const float *q = c;
            while (kk < r && q[step[d]] < q[0] && q[step[d]] > thr) {
                q += step[d];
                kk++;
            }
            e[d] = min(r, kk + 1);
        }
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < nslots) {
            StarCand cd;
            cd.x = x;
            cd.y = y;
            cd.ext = e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24);
            cd.pad = 0;
            slots[(long long)tile * nslots + slot] = cd;
        }
    }
    __syncthreads();
    if (tid == 0) tcount[tile] = min(s_cnt, nslots);
}

// candidates of every frame: one workgroup per frame
__global__ __launch_bounds__(256) void k_star_count(const int *tcount, int tiles, long long *ncand) {
    __shared__ long long s_sum[256];
    const int *tc = tcount + (long long)blockIdx.x * tiles;
    long long a = 0;
    for (int i = threadIdx.x; i < tiles; i += 256) a += tc[i];
    s_sum[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) ncand[blockIdx.x] = s_sum[0];
}

struct StarMeasureP {
    double cut, min_fwhm, max_fwhm, roundness_min, sat;
};

// one thread per slot; out: `cap` records per frame, acc[f] counts every record that asked for one
template <typename T>
__global__ __launch_bounds__(256) void k_star_measure(const T *in, long long rstride, long long fstride, int tiles,
                                                      int nslots, const int *tcount, const StarCand *slots,
                                                      const StarFrame *fp, StarMeasureP mp, int keep_all,
                                                      sgpu_star *out, unsigned cap, unsigned *acc) {
    const int f = blockIdx.z;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)tiles * nslots) return;
    const int tile = (int)(idx / nslots), slot = (int)(idx - (long long)tile * nslots);
    const long long gt = (long long)f * tiles + tile;
    if (slot >= tcount[gt]) return;
    const StarCand cd = slots[gt * nslots + slot];
    const T *fin = in + (long long)f * fstride;
    const double B = fp[f].bg;
    sgpu_star st;
    st.px = cd.x;
    st.py = cd.y;
    st.ext[0] = cd.ext & 255;
    st.ext[1] = (cd.ext >> 8) & 255;
    st.ext[2] = (cd.ext >> 16) & 255;
    st.ext[3] = (cd.ext >> 24) & 255;
    st.x = st.y = st.flux = st.fwhm_major = st.fwhm_minor = st.roundness = 0.0;
    st.npix = 0;
    const float peak = (float)fin[(long long)cd.y * rstride + cd.x];
    const double A = (double)peak - B;
    st.amp = A;
    int rej = 0;
    if (!(A >= fp[f].amin)) rej = 1;
    else if ((double)peak >= mp.sat) rej = 2;
    if (!rej) {
        const double lim = mp.cut * A;
        double S0 = 0.0, Sx = 0.0, Sy = 0.0, Sxx = 0.0, Syy = 0.0, Sxy = 0.0;
        int npix = 0;
        for (int dy = -st.ext[2]; dy <= st.ext[3]; dy++) {
            const T *row = fin + (long long)(cd.y + dy) * rstride + cd.x;
            const double ddy = (double)dy;
            double r0 = 0.0, rx = 0.0, ry = 0.0, rxx = 0.0, ryy = 0.0, rxy = 0.0;
            for (int dx = -st.ext[0]; dx <= st.ext[1]; dx++) {
                const double v = (double)(float)row[dx] - B;
                if (v > lim) {
                    const double ddx = (double)dx;
                    const double vx = v * ddx, vy = v * ddy;
                    r0 += v;
                    rx += vx;
                    ry += vy;
                    rxx += vx * ddx;
                    ryy += vy * ddy;
                    rxy += vx * ddy;
                    npix++;
                }
            }
            S0 += r0;
            Sx += rx;
            Sy += ry;
            Sxx += rxx;
            Syy += ryy;
            Sxy += rxy;
        }
        st.flux = S0;
        st.npix = npix;
        if (!(S0 > 0.0)) rej = 3;
        else {
            const double mx = Sx / S0, my = Sy / S0;
            const double a = Sxx / S0 - mx * mx, c = Syy / S0 - my * my, b = Sxy / S0 - mx * my;
            const double hd = (a - c) / 2.0;
            const double q = sqrt(hd * hd + b * b);
            const double l1 = (a + c) / 2.0 + q, l2 = (a + c) / 2.0 - q;
            st.x = (double)cd.x + mx;
            st.y = (double)cd.y + my;
            if (!(l2 > 0.0)) rej = 3;
            else {
                st.fwhm_major = 2.3548200450309493 * sqrt(l1);
                st.fwhm_minor = 2.3548200450309493 * sqrt(l2);
                st.roundness = sqrt(l2 / l1);
                if (!(st.fwhm_minor >= mp.min_fwhm)) rej = 4;
                else if (!(st.fwhm_major <= mp.max_fwhm)) rej = 5;
                else if (!(st.roundness >= mp.roundness_min)) rej = 6;
            }
        }
    }
    st.reject = rej;
    if (rej && !keep_all) return;
    const unsigned o = atomicAdd(&acc[f], 1u);
    if (o < cap) out[(size_t)f * cap + o] = st;
}

}  // namespace sgpu

using sgpu_host::fail;

extern "C" int sgpu_star_smooth_table(double sigma, float *tab, int *taps) {
    if (!tab || !taps || !(sigma >= 0.0) || !(sigma <= 2.0))
        return fail(SGPU_BAD_ARGUMENT, "star smoothing: 0 <= sigma <= 2");
    const int K = (int)std::ceil(3.0 * sigma);
    *taps = 2 * K + 1;
    if (K == 0) {
        tab[0] = 1.f;
        return SGPU_OK;
    }
    double t[2 * sgpu::ST_MAXK + 1], sum = 0.0;
    for (int k = -K; k <= K; k++) {
        t[k + K] = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
        sum += t[k + K];
    }
    for (int k = 0; k <= 2 * K; k++) tab[k] = (float)(t[k] / sum);
    return SGPU_OK;
}

extern "C" void sgpu_star_default_params(sgpu_star_params *p) {
    if (!p) return;
    p->ksigma = 1.0;
    p->smooth_sigma = 1.0;
    p->roundness_min = 0.5;
    p->min_amp = 5.0;
    p->cut = 0.1;
    p->min_fwhm = 1.0;
    p->sat = INFINITY;
    p->radius = 10;
    p->max_stars = 2000;
    p->keep_candidates = 0;
    p->reserved = 0;
}

namespace {

template <typename T>
void launch_candidates(int K, dim3 grid, size_t lds, hipStream_t st, const void *in, int W, int H, long long rs,
                       long long fs, int r, const sgpu::StarTab &tab, const sgpu::StarFrame *fp, int *tcount,
                       sgpu::StarCand *slots, int nslots) {
#define SGPU_STAR_LAUNCH(KK)                                                                                   \
    hipLaunchKernelGGL((sgpu::k_star_candidates<T, KK>), grid, dim3(256), lds, st, (const T *)in, W, H, rs, fs, \
                       r, tab, fp, tcount, slots, nslots)
    switch (K) {
        case 0: SGPU_STAR_LAUNCH(0); break;
        case 1: SGPU_STAR_LAUNCH(1); break;
        case 2: SGPU_STAR_LAUNCH(2); break;
        case 3: SGPU_STAR_LAUNCH(3); break;
        case 4: SGPU_STAR_LAUNCH(4); break;
        case 5: SGPU_STAR_LAUNCH(5); break;
        default: SGPU_STAR_LAUNCH(6); break;
    }
#undef SGPU_STAR_LAUNCH
}

bool star_before(const sgpu_star &a, const sgpu_star &b) {   // flux descending, then (row, column)
    if (a.flux != b.flux) return a.flux > b.flux;
    if (a.py != b.py) return a.py < b.py;
    return a.px < b.px;
}
bool raster_before(const sgpu_star &a, const sgpu_star &b) { return a.py != b.py ? a.py < b.py : a.px < b.px; }

constexpr size_t STAR_SLOT_BUDGET = (size_t)256 << 20;   // candidate slots of one chunk of frames

}  // namespace

extern "C" int sgpu_find_stars_device(sgpu_context *c, const void *d_frames, int elem_size, int nframes, int width,
                                      int height, long row_stride, long frame_stride, const double *bg,
                                      const double *noise, const sgpu_star_params *p, sgpu_star *stars, int *nstars,
                                      long *ncandidates) {
    if (!c || !d_frames || !bg || !noise || !p || !stars || !nstars || nframes < 1 || width < 1 || height < 1 ||
        row_stride < width || frame_stride < (long)(height - 1) * row_stride + width)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (p->radius < 1 || p->radius > sgpu::ST_MAXR) return fail(SGPU_BAD_ARGUMENT, "find_stars: 1 <= radius <= 16");
    if (!(p->smooth_sigma >= 0.0) || !(p->smooth_sigma <= 2.0))
        return fail(SGPU_BAD_ARGUMENT, "find_stars: 0 <= smooth_sigma <= 2");
    if (p->max_stars < 1) return fail(SGPU_BAD_ARGUMENT, "find_stars: max_stars >= 1");
    if (!std::isfinite(p->ksigma) || !std::isfinite(p->min_amp) || !(p->cut >= 0.0) || !(p->cut < 1.0) ||
        !(p->min_fwhm >= 0.0) || !std::isfinite(p->min_fwhm) || !(p->roundness_min >= 0.0) ||
        !(p->roundness_min <= 1.0) || std::isnan(p->sat))
        return fail(SGPU_BAD_ARGUMENT, "find_stars: parameter out of range");
    for (int f = 0; f < nframes; f++)
        if (!std::isfinite(bg[f]) || !std::isfinite(noise[f]) || noise[f] < 0.0)
            return fail(SGPU_BAD_ARGUMENT, "find_stars: bg and noise must be finite, noise >= 0");
    const int gx = (width + sgpu::ST_TW - 1) / sgpu::ST_TW, gy = (height + sgpu::ST_TH - 1) / sgpu::ST_TH;
    if (gy > 65535) return fail(SGPU_BAD_ARGUMENT, "find_stars: frame too high");

    const int r = p->radius;
    sgpu::StarTab tab;
    std::memset(&tab, 0, sizeof tab);
    int taps = 0;
    if (int rc = sgpu_star_smooth_table(p->smooth_sigma, tab.t, &taps)) return rc;
    const int K = taps / 2, P = r + K;
    c->star_cand.assign((size_t)nframes, std::vector<sgpu_star>());
    c->star_ms[0] = c->star_ms[1] = 0.f;
    for (int f = 0; f < nframes; f++) {
        nstars[f] = 0;
        if (ncandidates) ncandidates[f] = 0;
    }
    if (width <= 2 * P || height <= 2 * P) return SGPU_OK;   // no interior pixel

    const int nslots = sgpu::star_slots_1d(sgpu::ST_TW, r) * sgpu::star_slots_1d(sgpu::ST_TH, r);
    const long long tiles = (long long)gx * gy;
    if (tiles * nslots > 0x7fffffffLL) return fail(SGPU_BAD_ARGUMENT, "find_stars: frame too large");
    const size_t slot_bytes = (size_t)tiles * nslots * sizeof(sgpu::StarCand);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)nframes, STAR_SLOT_BUDGET / slot_bytes, 65535}));
    const int RW = sgpu::ST_TW + 2 * P, RH = sgpu::ST_TH + 2 * P, SW = sgpu::ST_TW + 2 * r;
    const size_t lds = ((size_t)RH * (RW | 1) + (size_t)RH * (SW | 1)) * sizeof(float);
    const sgpu::StarMeasureP mp = {p->cut, p->min_fwhm, (double)(2 * r + 1), p->roundness_min, p->sat};
    const int keep = p->keep_candidates != 0;

    HIP_TRY(hipSetDevice(c->device));
    for (int k = 0; k < 3; k++)
        if (!c->star_ev[k]) HIP_TRY(hipEventCreate(&c->star_ev[k]));
    if (int rc = c->star_tc.ensure((size_t)chunk * tiles * sizeof(int))) return rc;
    if (int rc = c->star_slots.ensure((size_t)chunk * slot_bytes)) return rc;
    // [per-frame constants][candidate totals][record counters]
    const size_t fp_bytes = (size_t)chunk * sizeof(sgpu::StarFrame);
    if (int rc = c->star_fp.ensure(fp_bytes + (size_t)chunk * (sizeof(long long) + sizeof(unsigned)))) return rc;
    sgpu::StarFrame *dfp = (sgpu::StarFrame *)c->star_fp.p;
    long long *dnc = (long long *)((char *)c->star_fp.p + fp_bytes);
    unsigned *dacc = (unsigned *)(dnc + chunk);
    unsigned cap = (unsigned)std::max(4 * (long long)p->max_stars, 64LL);   // grown when a frame needs more

    std::vector<sgpu::StarFrame> hfp((size_t)chunk);
    std::vector<long long> hnc((size_t)chunk);
    std::vector<unsigned> hacc((size_t)chunk);
    std::vector<sgpu_star> rec;
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
        const int nf = std::min(chunk, nframes - f0);
        for (int f = 0; f < nf; f++) {
            hfp[f].bg = bg[f0 + f];
            hfp[f].amin = p->min_amp * noise[f0 + f];
            hfp[f].thr = (float)(bg[f0 + f] + p->ksigma * noise[f0 + f]);
            hfp[f].pad = 0.f;
        }
        HIP_TRY(hipMemcpyAsync(dfp, hfp.data(), (size_t)nf * sizeof(sgpu::StarFrame), hipMemcpyHostToDevice,
                               c->stream));
        const char *base = (const char *)d_frames + (size_t)f0 * (size_t)frame_stride * (size_t)elem_size;
        HIP_TRY(hipEventRecord(c->star_ev[0], c->stream));
        const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)nf);
        if (elem_size == 4)
            launch_candidates<float>(K, grid, lds, c->stream, base, width, height, row_stride, frame_stride, r, tab,
                                     dfp, (int *)c->star_tc.p, (sgpu::StarCand *)c->star_slots.p, nslots);
        else
            launch_candidates<uint16_t>(K, grid, lds, c->stream, base, width, height, row_stride, frame_stride, r,
                                        tab, dfp, (int *)c->star_tc.p, (sgpu::StarCand *)c->star_slots.p, nslots);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sgpu::k_star_count, dim3((unsigned)nf), dim3(256), 0, c->stream,
                           (const int *)c->star_tc.p, (int)tiles, dnc);
        HIP_TRY(hipGetLastError());
        // measure; a record list that proves too small is grown and the measurement run again
        for (;;) {
            if (int rc = c->star_out.ensure((size_t)nf * cap * sizeof(sgpu_star))) return rc;
            HIP_TRY(hipMemsetAsync(dacc, 0, (size_t)nf * sizeof(unsigned), c->stream));
            HIP_TRY(hipEventRecord(c->star_ev[1], c->stream));
            const dim3 mg((unsigned)((tiles * nslots + 255) / 256), 1, (unsigned)nf);
            if (elem_size == 4)
                hipLaunchKernelGGL(sgpu::k_star_measure<float>, mg, dim3(256), 0, c->stream, (const float *)base,
                                   (long long)row_stride, (long long)frame_stride, (int)tiles, nslots,
                                   (const int *)c->star_tc.p, (const sgpu::StarCand *)c->star_slots.p, dfp, mp, keep,
                                   (sgpu_star *)c->star_out.p, cap, dacc);
            else
                hipLaunchKernelGGL(sgpu::k_star_measure<uint16_t>, mg, dim3(256), 0, c->stream,
                                   (const uint16_t *)base, (long long)row_stride, (long long)frame_stride, (int)tiles,
                                   nslots, (const int *)c->star_tc.p, (const sgpu::StarCand *)c->star_slots.p, dfp,
                                   mp, keep, (sgpu_star *)c->star_out.p, cap, dacc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(c->star_ev[2], c->stream));
            HIP_TRY(hipMemcpyAsync(hacc.data(), dacc, (size_t)nf * sizeof(unsigned), hipMemcpyDeviceToHost,
                                   c->stream));
            HIP_TRY(hipMemcpyAsync(hnc.data(), dnc, (size_t)nf * sizeof(long long), hipMemcpyDeviceToHost,
                                   c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const unsigned most = *std::max_element(hacc.begin(), hacc.begin() + nf);
            if (most <= cap) break;
            cap = most;
        }
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->star_ev[0], c->star_ev[1]));
        c->star_ms[0] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, c->star_ev[1], c->star_ev[2]));
        c->star_ms[1] += ms;
        for (int f = 0; f < nf; f++) {
            if (ncandidates) ncandidates[f0 + f] = (long)hnc[f];
            rec.resize(hacc[f]);
            if (hacc[f])
                HIP_TRY(hipMemcpy(rec.data(), (const sgpu_star *)c->star_out.p + (size_t)f * cap,
                                  (size_t)hacc[f] * sizeof(sgpu_star), hipMemcpyDeviceToHost));
            if (keep) {
                std::sort(rec.begin(), rec.end(), raster_before);
                c->star_cand[(size_t)(f0 + f)] = rec;
                rec.erase(std::remove_if(rec.begin(), rec.end(), [](const sgpu_star &s) { return s.reject != 0; }),
                          rec.end());
            }
            std::sort(rec.begin(), rec.end(), star_before);
            const size_t n = std::min(rec.size(), (size_t)p->max_stars);
            if (n) std::memcpy(stars + (size_t)(f0 + f) * p->max_stars, rec.data(), n * sizeof(sgpu_star));
            nstars[f0 + f] = (int)n;
        }
    }
    return SGPU_OK;
}

extern "C" int sgpu_star_last_candidates(sgpu_context *c, int frame, sgpu_star *cand, long capacity, long *count) {
    if (!c || !count || frame < 0 || (size_t)frame >= c->star_cand.size() || capacity < 0 || (capacity && !cand))
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    const std::vector<sgpu_star> &v = c->star_cand[(size_t)frame];
    *count = (long)v.size();
    if ((long)v.size() <= capacity && !v.empty()) std::memcpy(cand, v.data(), v.size() * sizeof(sgpu_star));
    return SGPU_OK;
}

extern "C" int sgpu_star_last_kernel_ms(sgpu_context *c, float ms[2]) {
    if (!c || !ms) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    ms[0] = c->star_ms[0];
    ms[1] = c->star_ms[1];
    return SGPU_OK;
}

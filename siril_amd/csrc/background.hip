// background.hip -- polynomial background extraction (`seqsubsky <seq> <degree>`,
// Siril's filters/background_extraction.c) on planes resident in HBM: the
// medians of a grid of 25 x 25 sample boxes, the selection of the boxes that
// hold sky, a least-squares polynomial of degree 1 .. 4 through them, and the
// streaming pass that subtracts (or divides by) the polynomial.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// arithmetic is specified in DESIGN.md 6i (B0-B7), lives in bkg_host.h and is
// restated in tests/bkg_ref.py; that restatement is the contract.  Parity with
// a Siril binary is unpinned.
//
// Three launches per call, nothing returns to the host between them:
//   k_bkg_box_median   one wavefront per (plane, box): the 625 samples sit in
//                      the lanes' registers as ordered keys (lanes 0-48 hold
//                      ten, the others nine) and the key of rank 312 is built
//                      bit by bit from the top, each bit from ten ballots
//   k_bkg_fit          one workgroup per plane: the medians of the K box
//                      medians and of their deviations by rank counting in
//                      LDS and the keep mask (bkg_kernels.h, shared with the
//                      spline model), the 120 + 15 normal sums one per
//                      thread (each walks the boxes in ascending k), Cholesky
//                      and the mean in thread 0; the axis moments of the mean
//                      depend on W and H alone and come from the host
//   k_bkg_apply_vec    8 WORD / 4 float pixels per lane in k_calibrate_vec's
//                      gap-free layout, non-temporal loads and stores; the
//                      five row polynomials are recomputed by the lane when
//                      its pixels cross into the next row
//   k_bkg_apply_scalar the same arithmetic one pixel per lane: the tail of W*H
//                      and every call whose pointers or stride are not 16-byte
//                      aligned
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bkg_host.h"
#include "bkg_kernels.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_bkg_host;

namespace sgpu {

typedef float bvf4 __attribute__((ext_vector_type(4)));      // nontemporal builtins take clang vectors

constexpr int BKG_SLOTS = (BKG_NS + 63) / 64;       // 10

// ---- B2 -----------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_bkg_box_median(const T *in, long long pstride, int W, BkgGrid g,
                                                        long long nbox, float *med) {
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= nbox) return;       // whole wavefronts leave
    const int lane = threadIdx.x & 63;
    const int plane = (int)(wave / g.K), k = (int)(wave - (long long)plane * g.K);
    const int bj = k / g.nx, bi = k - bj * g.nx;
    const T *src = in + (long long)plane * pstride + (long long)(bkg_cy(g, bj) - BKG_R) * W + (bkg_cx(g, bi) - BKG_R);
    uint32_t key[BKG_SLOTS];
#pragma unroll
    for (int s = 0; s < BKG_SLOTS; s++) {
        const int e = s * 64 + lane;
        const int dy = e / BKG_BOX, dx = e - dy * BKG_BOX;
        key[s] = 0;
        if (e < BKG_NS) key[s] = bkg_key(bkg_to_float(src[(long long)dy * W + dx]));
    }
    // the keys that agree with `prefix` above bit b are the candidates; the bit
    // is 0 when the wanted rank falls among those whose bit b is 0
    uint32_t prefix = 0;
    int rank = BKG_RANK;
    for (int b = 31; b >= 0; b--) {
        const uint32_t above = ~((2u << b) - 1u);
        int cnt0 = 0;
#pragma unroll
        for (int s = 0; s < BKG_SLOTS; s++) {
            const bool pred = (s * 64 + lane < BKG_NS) && ((key[s] ^ prefix) & above) == 0 && !((key[s] >> b) & 1u);
            cnt0 += __popcll(__ballot(pred));
        }
        if (rank >= cnt0) {
            rank -= cnt0;
            prefix |= 1u << b;
        }
    }
    if (lane == 0) med[wave] = bkg_median_of_key(prefix);
}

// ---- B3 - B5 --------------------------------------------------------------------
// mom: B5's axis moments Mx[0 .. 4], My[0 .. 4].  They depend on the plane's size alone, so the
// host computes them once per size (the same functions, the same bits) and keeps them on the device.

__global__ __launch_bounds__(BKG_FIT_THREADS) void k_bkg_fit(const float *med_all, BkgGrid g, int W, int H, int degree,
                                                             double tol, const double *mom, uint8_t *keep_all,
                                                             double *coef_all, double *mean_all, int *kept_all,
                                                             int *status_all) {
    extern __shared__ double s_dyn[];       // K doubles, K floats, K bytes
    const int plane = blockIdx.x, tid = threadIdx.x, K = g.K;
    double *s_d = s_dyn;
    float *s_med = reinterpret_cast<float *>(s_dyn + K);
    uint8_t *s_keep = reinterpret_cast<uint8_t *>(s_med + K);
    __shared__ double s_res[2], s_A[BKG_NCOEF * BKG_NCOEF], s_g[BKG_NCOEF], s_L[BKG_NCOEF * BKG_NCOEF], s_y[BKG_NCOEF],
        s_c[BKG_NCOEF];
    __shared__ int s_kept;
    const int kept = bkg_select_lds(med_all + (size_t)plane * K, K, tol, s_d, s_med, s_keep, s_res, &s_kept,
                                    keep_all + (size_t)plane * K);
    const int n = bkg_ncoef(degree);
    int st = kept < n ? 1 : 0;
    if (!st) {
        if (tid < BKG_NPAIR) {
            int p, q;
            bkg_pair(tid, p, q);
            if (p < n) s_A[p * BKG_NCOEF + q] = s_A[q * BKG_NCOEF + p] = bkg_normal_sum(p, q, s_med, s_keep, g, W, H);
        } else if (tid < BKG_NPAIR + BKG_NCOEF) {
            const int p = tid - BKG_NPAIR;
            if (p < n) s_g[p] = bkg_normal_sum(p, -1, s_med, s_keep, g, W, H);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double mean = 0.0;
        if (!st) st = bkg_solve(n, s_A, s_g, s_c, s_L, s_y);
        if (!st) mean = bkg_model_mean(s_c, mom, mom + 5);
        for (int p = 0; p < BKG_NCOEF; p++) coef_all[(size_t)plane * BKG_NCOEF + p] = st ? 0.0 : s_c[p];
        mean_all[plane] = mean;
        kept_all[plane] = kept;
        status_all[plane] = st;
    }
}

// ---- B6 + B7 --------------------------------------------------------------------
struct BkgAxes {
    double x0, ax, y0, ay;      // u = ((double)x - x0) * ax, v likewise
};

struct BkgModel {
    double C[25], mean;
    int status;
};

__device__ __forceinline__ void bkg_load_model(const double *coef_all, const double *mean_all, const int *status_all,
                                               int plane, BkgModel &m) {
    double c[BKG_NCOEF];
#pragma unroll
    for (int p = 0; p < BKG_NCOEF; p++) c[p] = coef_all[(size_t)plane * BKG_NCOEF + p];
#pragma unroll
    for (int i = 0; i < 5; i++)
#pragma unroll
        for (int j = 0; j < 5; j++) m.C[i * 5 + j] = i + j <= 4 ? c[(i + j) * (i + j + 1) / 2 + j] : 0.0;
    m.mean = mean_all[plane];
    m.status = status_all[plane];
}

// Lane l of a 64-lane group handles the pixels [g*64*PX + q*256 + 4*l, +4) for
// q < PX/4: k_calibrate_vec's layout, every 16-byte access of
// the group covers 1 KiB without gaps.
template <typename T>
__global__ __launch_bounds__(256) void k_bkg_apply_vec(const T *in, float *out, long long nlanes, long long pstride,
                                                       int W, BkgAxes ax, int divide, const double *coef_all,
                                                       const double *mean_all, const int *status_all) {
    constexpr int PX = 16 / (int)sizeof(T), Q = PX / 4;
    typedef uint32_t raw_t __attribute__((ext_vector_type(sizeof(T))));      // four samples
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nlanes) return;
    const int plane = blockIdx.y;
    const long long p0 = (v >> 6) * (64 * PX) + (v & 63) * 4;
    const T *src = in + (long long)plane * pstride + p0;
    float *dst = out + (long long)plane * pstride + p0;
    raw_t raw[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) raw[q] = __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(src + q * 256));
    BkgModel m;
    bkg_load_model(coef_all, mean_all, status_all, plane, m);
#pragma unroll
    for (int q = 0; q < Q; q++) {
        float x[4];
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = __uint_as_float(raw[q][j]);
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                x[2 * j] = bkg_to_float((uint16_t)(raw[q][j] & 0xffffu));
                x[2 * j + 1] = bkg_to_float((uint16_t)(raw[q][j] >> 16));
            }
        }
        bvf4 r;
        if (m.status) {
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = x[j];
        } else {
            const unsigned p = (unsigned)(p0 + q * 256);
            unsigned row = p / (unsigned)W, col = p - row * (unsigned)W;
            double rp[5];
            bkg_row_poly(m.C, ((double)(int)row - ax.y0) * ax.ay, rp);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (col == (unsigned)W) {       // the lane's pixels go on in the next row
                    col = 0;
                    row++;
                    bkg_row_poly(m.C, ((double)(int)row - ax.y0) * ax.ay, rp);
                }
                const double b = bkg_eval(rp, ((double)(int)col - ax.x0) * ax.ax);
                r[j] = bkg_correct(x[j], b, m.mean, divide);
                col++;
            }
        }
        __builtin_nontemporal_store(r, reinterpret_cast<bvf4 *>(dst + q * 256));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bkg_apply_scalar(const T *in, float *out, long long p_begin, long long p_end,
                                                          long long pstride, int W, BkgAxes ax, int divide,
                                                          const double *coef_all, const double *mean_all,
                                                          const int *status_all) {
    const long long p = p_begin + (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= p_end) return;
    const int plane = blockIdx.y;
    BkgModel m;
    bkg_load_model(coef_all, mean_all, status_all, plane, m);
    const float x = bkg_to_float(in[(long long)plane * pstride + p]);
    float r = x;
    if (!m.status) {
        const unsigned row = (unsigned)p / (unsigned)W, col = (unsigned)p - row * (unsigned)W;
        double rp[5];
        bkg_row_poly(m.C, ((double)(int)row - ax.y0) * ax.ay, rp);
        r = bkg_correct(x, bkg_eval(rp, ((double)(int)col - ax.x0) * ax.ax), m.mean, divide);
    }
    out[(long long)plane * pstride + p] = r;
}

}  // namespace sgpu

// ===================================================================== host
// the spline model's way to k_bkg_box_median (background_rbf.hip)
int sgpu::bkg_launch_box_median(sgpu_context *c, const void *d_in, int elem_size, long long pstride, int W,
                                const BkgGrid &g, long long nbox, float *d_med) {
    const dim3 grid((unsigned)((nbox + 3) / 4));
    if (elem_size == 4)
        hipLaunchKernelGGL((sgpu::k_bkg_box_median<float>), grid, dim3(256), 0, c->stream, (const float *)d_in, pstride,
                           W, g, nbox, d_med);
    else
        hipLaunchKernelGGL((sgpu::k_bkg_box_median<uint16_t>), grid, dim3(256), 0, c->stream, (const uint16_t *)d_in,
                           pstride, W, g, nbox, d_med);
    HIP_TRY(hipGetLastError());
    return SGPU_OK;
}

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int launch_subsky(sgpu_context *c, const void *d_in, float *d_out, int P, int W, int H, long pstride,
                  const sgpu_bkg_params *prm, const BkgGrid &g, float *d_med, uint8_t *d_keep, double *d_coef,
                  double *d_mean, int *d_kept, int *d_status) {
    const long long nbox = (long long)P * g.K, npix = (long long)W * H;
    c->bkg_timed = 0;
    for (hipEvent_t &e : c->bkg_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->bkg_ev[0], c->stream));
    hipLaunchKernelGGL((sgpu::k_bkg_box_median<T>), dim3((unsigned)((nbox + 3) / 4)), dim3(256), 0, c->stream,
                       (const T *)d_in, (long long)pstride, W, g, nbox, d_med);
    const size_t lds = (size_t)g.K * (sizeof(double) + sizeof(float) + 1);
    if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)sgpu::k_bkg_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipEventRecord(c->bkg_ev[1], c->stream));
    if (c->bkg_M_key[0] != W || c->bkg_M_key[1] != H) {
        c->bkg_M[0] = c->bkg_M[5] = 1.0;
        for (int i = 1; i <= 4; i++) {
            c->bkg_M[i] = bkg_axis_moment(W, i);
            c->bkg_M[5 + i] = bkg_axis_moment(H, i);
        }
        if (int r = c->bkg_mom.ensure(sizeof c->bkg_M)) return r;
        // c->bkg_M outlives the copy; an earlier call's kernel that still reads the buffer is ahead on the stream
        HIP_TRY(hipMemcpyAsync(c->bkg_mom.p, c->bkg_M, sizeof c->bkg_M, hipMemcpyHostToDevice, c->stream));
        c->bkg_M_key[0] = W;
        c->bkg_M_key[1] = H;
    }
    const double *mom = (const double *)c->bkg_mom.p;
    hipLaunchKernelGGL(sgpu::k_bkg_fit, dim3((unsigned)P), dim3(sgpu::BKG_FIT_THREADS), lds, c->stream, d_med, g, W, H,
                       prm->degree, prm->tolerance, mom, d_keep, d_coef, d_mean, d_kept, d_status);
    HIP_TRY(hipEventRecord(c->bkg_ev[2], c->stream));
    sgpu::BkgAxes ax;
    ax.x0 = (double)(W - 1) * 0.5;
    ax.ax = 1.0 / ax.x0;
    ax.y0 = (double)(H - 1) * 0.5;
    ax.ay = 1.0 / ax.y0;
    constexpr int PX = 16 / (int)sizeof(T);
    const bool aligned = aligned16(d_in) && aligned16(d_out) && ((size_t)pstride * sizeof(T)) % 16 == 0 &&
                         ((size_t)pstride * sizeof(float)) % 16 == 0;
    // whole 64-lane groups go through the vector kernel, the rest is the scalar tail
    const long long nlanes = aligned ? npix / (64 * PX) * 64 : 0, tail0 = nlanes * PX;
    const int divide = prm->divide ? 1 : 0;
    if (nlanes)
        hipLaunchKernelGGL((sgpu::k_bkg_apply_vec<T>), dim3((unsigned)((nlanes + 255) / 256), (unsigned)P), dim3(256), 0,
                           c->stream, (const T *)d_in, d_out, nlanes, (long long)pstride, W, ax, divide, d_coef, d_mean,
                           d_status);
    if (tail0 < npix)
        hipLaunchKernelGGL((sgpu::k_bkg_apply_scalar<T>), dim3((unsigned)((npix - tail0 + 255) / 256), (unsigned)P),
                           dim3(256), 0, c->stream, (const T *)d_in, d_out, tail0, npix, (long long)pstride, W, ax,
                           divide, d_coef, d_mean, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->bkg_ev[3], c->stream));
    c->bkg_timed = 1;
    return SGPU_OK;
}

}  // namespace

extern "C" int sgpu_bkg_last_kernel_ms(sgpu_context *c, float ms[3]) {
    if (!c || !ms) return fail(SGPU_BAD_ARGUMENT, "bkg_last_kernel_ms: null argument");
    ms[0] = ms[1] = ms[2] = 0.f;
    if (!c->bkg_timed) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->bkg_ev[3]));
    for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&ms[k], c->bkg_ev[k], c->bkg_ev[k + 1]));
    return SGPU_OK;
}

extern "C" void sgpu_bkg_default_params(sgpu_bkg_params *p) {
    if (!p) return;
    p->degree = 1;
    p->samples = 20;
    p->tolerance = 1.0;
    p->divide = 0;
}

extern "C" int sgpu_bkg_grid(int width, int height, int samples, int *nx, int *ny, int *dist, int *startx,
                             int *starty) {
    BkgGrid g;
    if (const char *why = bkg_grid(width, height, samples, &g)) return fail(SGPU_BAD_ARGUMENT, why);
    if (nx) *nx = g.nx;
    if (ny) *ny = g.ny;
    if (dist) *dist = g.dist;
    if (startx) *startx = g.startx;
    if (starty) *starty = g.starty;
    return SGPU_OK;
}

extern "C" int sgpu_subsky_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width,
                                         int height, long plane_stride, const sgpu_bkg_params *params, float *d_out,
                                         float *d_med, unsigned char *d_keep, double *d_coef, double *d_mean,
                                         int *d_kept, int *d_status) {
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (const char *why = bkg_check_params(params)) return fail(SGPU_BAD_ARGUMENT, why);
    BkgGrid g;
    if (const char *why = bkg_grid(width, height, params->samples, &g)) return fail(SGPU_BAD_ARGUMENT, why);
    if (!c || nplanes < 0 || nplanes > 65535 || (long long)width * height >= (1LL << 31))
        return fail(SGPU_BAD_ARGUMENT, "subsky: bad argument");
    if (plane_stride < (long)width * height) return fail(SGPU_BAD_ARGUMENT, "plane_stride < width*height");
    c->bkg_timed = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "subsky: null planes");
    const size_t span = (size_t)(nplanes - 1) * (size_t)plane_stride + (size_t)width * (size_t)height;
    const char *i0 = (const char *)d_in, *i1 = i0 + span * (size_t)elem_size;
    const char *o0 = (const char *)d_out, *o1 = o0 + span * sizeof(float);
    if (i0 < o1 && o0 < i1 && !(elem_size == 4 && i0 == o0))
        return fail(SGPU_BAD_ARGUMENT, "subsky: the output overlaps the input (in place only for float planes)");
    HIP_TRY(hipSetDevice(c->device));
    // result arrays the caller did not give live in the context
    const size_t P = (size_t)nplanes, K = (size_t)g.K;
    const size_t o_coef = 0, o_mean = o_coef + P * BKG_NCOEF * sizeof(double), o_med = o_mean + P * sizeof(double),
                 o_kept = o_med + P * K * sizeof(float), o_status = o_kept + P * sizeof(int),
                 o_keep = o_status + P * sizeof(int), total = o_keep + P * K;
    if (!d_med || !d_keep || !d_coef || !d_mean || !d_kept || !d_status) {
        if (int r = c->bkg_ws.ensure(total)) return r;
        char *ws = (char *)c->bkg_ws.p;
        if (!d_coef) d_coef = (double *)(ws + o_coef);
        if (!d_mean) d_mean = (double *)(ws + o_mean);
        if (!d_med) d_med = (float *)(ws + o_med);
        if (!d_kept) d_kept = (int *)(ws + o_kept);
        if (!d_status) d_status = (int *)(ws + o_status);
        if (!d_keep) d_keep = (unsigned char *)(ws + o_keep);
    }
    if (elem_size == 4)
        return launch_subsky<float>(c, d_in, d_out, nplanes, width, height, plane_stride, params, g, d_med, d_keep,
                                    d_coef, d_mean, d_kept, d_status);
    return launch_subsky<uint16_t>(c, d_in, d_out, nplanes, width, height, plane_stride, params, g, d_med, d_keep,
                                   d_coef, d_mean, d_kept, d_status);
}

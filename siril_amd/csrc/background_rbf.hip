// background_rbf.hip -- thin-plate-spline background extraction (`subsky
// <image> -rbf`, the RBF model of Siril's filters/background_extraction.c) on
// planes resident in HBM: the box medians and the selection of the polynomial
// path (background.hip, bkg_kernels.h), a spline phi = r^2 log r with a
// constant term through the kept boxes, smoothed on the diagonal, and a pass
// that evaluates the spline at every pixel in double and subtracts (or divides
// by) it.
//
// PARITY STATUS: Siril's sources were not available to check against.  The
// arithmetic is specified in DESIGN.md 6k (R0-R7), lives in bkg_rbf_host.h and
// is restated in tests/bkg_rbf_ref.py; that restatement is the contract.
// Parity with a Siril binary is unpinned.
//
// Launches per call, nothing returns to the host between them:
//   k_bkg_box_median       background.hip's
//   k_bkg_rbf_fit          one 1024-thread workgroup per plane, at most 256 MiB
//                          of systems per launch: the selection, the samples
//                          compacted in ascending box order by ballots, Phi one
//                          row per wavefront into the workspace, the
//                          sequential sum of |Phi| by wavefront 0 (64 elements
//                          per load, added one after the other from scalar
//                          registers) while a lane of wavefront 1 sums the
//                          medians, then the LU below
//   rbf_lu_solve           per step: the pivot as a reduction over (|a| bits,
//                          row) pairs, lowest row among equals; the pivot row
//                          staged in LDS while it is swapped in memory; every
//                          wavefront updates whole rows.  The back
//                          substitution keeps the right-hand side in LDS.
//                          Every element's chain of operations is R4's
//                          whatever the parallelisation, so the bits are too.
//   k_bkg_rbf_solve        the LU alone on caller-given systems (the test seam)
//   k_bkg_rbf_apply_vec    k_bkg_apply_vec's layout and non-temporal accesses;
//                          the plane's samples (u, v, w) sit in LDS as doubles
//                          and are read as broadcasts, a lane's four pixels
//                          share dv^2 unless they cross into the next row
//   k_bkg_rbf_apply_scalar the same arithmetic one pixel per lane: the tail of
//                          W*H and every call whose pointers or stride are not
//                          16-byte aligned
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bkg_kernels.h"
#include "bkg_rbf_host.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

using sgpu_host::fail;
using namespace sgpu_bkg_host;

namespace sgpu {

typedef float rvf4 __attribute__((ext_vector_type(4)));      // nontemporal builtins take clang vectors

constexpr int RBF_THREADS = BKG_FIT_THREADS, RBF_WAVES = RBF_THREADS / 64;
constexpr int RBF_ROW = RBF_MAX_ORDER + 1;       // doubles of a staged row of [A | rhs]

// does (key, row) beat (best, brow): the larger key, the lower row among equals
__device__ __forceinline__ bool rbf_beats(uint64_t key, int row, uint64_t best, int brow) {
    return key > best || (key == best && row < brow);
}

// ---- R4 -------------------------------------------------------------------------
// [A | rhs] of order N (row stride N + 1) in global memory, overwritten, by one workgroup of RBF_THREADS.
// x[N] in global memory: the solution, or +0 when the status returned is 2.
// s_row: RBF_ROW doubles, s_b: RBF_MAX_ORDER doubles, s_key / s_idx: RBF_WAVES each, all LDS.
__device__ __forceinline__ int rbf_lu_solve(double *aug, int N, double *x, double *s_row, double *s_b, uint64_t *s_key,
                                            int *s_idx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ld = (size_t)N + 1;
    int st = 0;
    for (int k = 0; k < N; k++) {
        uint64_t best = 0;
        int brow = 0x7FFFFFFF;
        for (int i = k + tid; i < N; i += RBF_THREADS) {
            const uint64_t key = rbf_pivot_key(aug[i * ld + k]);
            if (rbf_beats(key, i, best, brow)) {
                best = key;
                brow = i;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t lo = __shfl_xor((int)(uint32_t)best, off), hi = __shfl_xor((int)(uint32_t)(best >> 32), off);
            const uint64_t okey = ((uint64_t)hi << 32) | lo;
            const int orow = __shfl_xor(brow, off);
            if (rbf_beats(okey, orow, best, brow)) {
                best = okey;
                brow = orow;
            }
        }
        if (lane == 0) {
            s_key[wave] = best;
            s_idx[wave] = brow;
        }
        __syncthreads();
        best = s_key[0];
        brow = s_idx[0];
#pragma unroll
        for (int w = 1; w < RBF_WAVES; w++)
            if (rbf_beats(s_key[w], s_idx[w], best, brow)) {
                best = s_key[w];
                brow = s_idx[w];
            }
        const int p = brow;     // k <= p < N: thread 0 always has a row
        for (int j = k + tid; j <= N; j += RBF_THREADS) {
            const double pv = aug[p * ld + j];
            s_row[j] = pv;
            if (p != k) {
                aug[p * ld + j] = aug[k * ld + j];
                aug[k * ld + j] = pv;
            }
        }
        __syncthreads();
        const double piv = s_row[k];
        if (rbf_pivot_bad(piv)) {       // the same for every thread
            st = 2;
            break;
        }
        for (int i = k + 1 + wave; i < N; i += RBF_WAVES) {
            const double l = aug[i * ld + k] / piv;
            for (int j = k + 1 + lane; j <= N; j += 64) {
                const double t = l * s_row[j];
                aug[i * ld + j] = aug[i * ld + j] - t;
            }
        }
        __syncthreads();
    }
    if (st) {
        for (int i = tid; i < N; i += RBF_THREADS) x[i] = 0.0;
        return st;
    }
    for (int i = tid; i < N; i += RBF_THREADS) s_b[i] = aug[i * ld + N];
    __syncthreads();
    for (int i = N - 1; i >= 0; i--) {
        const double xi = s_b[i] / aug[i * ld + i];
        if (tid == 0) x[i] = xi;
        for (int j = tid; j < i; j += RBF_THREADS) {
            const double t = aug[j * ld + i] * xi;
            s_b[j] = s_b[j] - t;
        }
        __syncthreads();
    }
    return 0;
}

__global__ __launch_bounds__(RBF_THREADS) void k_bkg_rbf_solve(double *aug_all, int N, double *x_all, int *status_all) {
    __shared__ double s_row[RBF_ROW], s_b[RBF_MAX_ORDER];
    __shared__ uint64_t s_key[RBF_WAVES];
    __shared__ int s_idx[RBF_WAVES];
    const size_t sys = blockIdx.x;
    const int st = rbf_lu_solve(aug_all + sys * (size_t)N * ((size_t)N + 1), N, x_all + sys * (size_t)N, s_row, s_b,
                                s_key, s_idx);
    if (threadIdx.x == 0) status_all[sys] = st;
}

// ---- R0 - R5 --------------------------------------------------------------------
// Plane plane0 + blockIdx.x; its system lives at aug_ws + blockIdx.x * aug_stride.
// samp_all: per plane K doubles u, then K doubles v, of the samples in kept order.
__global__ __launch_bounds__(RBF_THREADS) void k_bkg_rbf_fit(const float *med_all, BkgGrid g, RbfAxes ax, double tol,
                                                             double lam_rel, int plane0, double *aug_ws,
                                                             size_t aug_stride, uint8_t *keep_all, double *samp_all,
                                                             double *weights_all, double *mean_all, int *kept_all,
                                                             int *status_all) {
    __shared__ double s_d[RBF_MAX_ORDER], s_u[RBF_MAX_SAMPLES], s_v[RBF_MAX_SAMPLES], s_z[RBF_MAX_SAMPLES], s_row[RBF_ROW],
        s_res[2], s_sum, s_mean;
    __shared__ float s_med[RBF_MAX_SAMPLES];
    __shared__ uint8_t s_keep[RBF_MAX_SAMPLES];
    __shared__ uint64_t s_key[RBF_WAVES];
    __shared__ int s_idx[RBF_WAVES], s_wcnt[RBF_WAVES], s_kept;
    const int plane = plane0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = g.K;
    const int n = bkg_select_lds(med_all + (size_t)plane * K, K, tol, s_d, s_med, s_keep, s_res, &s_kept,
                                 keep_all + (size_t)plane * K);
    // the kept boxes in ascending k: K <= 1024, a box per thread
    const bool kp = tid < K && s_keep[tid];
    const unsigned long long mask = __ballot(kp);
    if (lane == 0) s_wcnt[wave] = __popcll(mask);
    __syncthreads();
    if (kp) {
        int idx = __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) idx += s_wcnt[w];
        const int bj = tid / g.nx, bi = tid - bj * g.nx;
        const double u = rbf_u(bkg_cx(g, bi), ax), v = rbf_v(bkg_cy(g, bj), ax);
        s_u[idx] = u;
        s_v[idx] = v;
        s_z[idx] = (double)s_med[tid];
        samp_all[(size_t)plane * 2 * K + idx] = u;
        samp_all[(size_t)plane * 2 * K + K + idx] = v;
    }
    __syncthreads();
    double *wout = weights_all + (size_t)plane * (RBF_MAX_SAMPLES + 1);
    if (n == 0) {
        for (int i = tid; i <= RBF_MAX_SAMPLES; i += RBF_THREADS) wout[i] = 0.0;
        if (tid == 0) {
            mean_all[plane] = 0.0;
            kept_all[plane] = 0;
            status_all[plane] = 1;
        }
        return;
    }
    // R3: Phi, the border and the right-hand side
    const int N = n + 1;
    const size_t ld = (size_t)N + 1;
    double *aug = aug_ws + (size_t)blockIdx.x * aug_stride;
    for (int i = wave; i < n; i += RBF_WAVES) {
        const double ui = s_u[i], vi = s_v[i];
        for (int j = lane; j < n; j += 64) aug[i * ld + j] = rbf_phi(ui - s_u[j], vi - s_v[j]);
        if (lane == 0) {
            aug[i * ld + n] = 1.0;
            aug[i * ld + N] = s_z[i];
        }
    }
    for (int j = tid; j <= N; j += RBF_THREADS) aug[n * ld + j] = j < n ? 1.0 : 0.0;
    __syncthreads();
    if (wave == 0) {
        // the sum of |Phi|, row-major and sequential: 64 elements per load, added in order; the +0 that
        // pad a row's last load leave the sum as it is (it is never negative)
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
            const double *row = aug + i * ld;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const double a = j0 + lane < n ? fabs(row[j0 + lane]) : 0.0;
                const int lo = (int)(uint32_t)rbf_bits(a), hi = (int)(uint32_t)(rbf_bits(a) >> 32);
#pragma unroll
                for (int l = 0; l < 64; l++) {
                    const uint32_t ql = (uint32_t)__builtin_amdgcn_readlane(lo, l), qh = (uint32_t)__builtin_amdgcn_readlane(hi, l);
                    acc = acc + rbf_from_bits(((uint64_t)qh << 32) | ql);
                }
            }
        }
        if (lane == 0) s_sum = acc;
    } else if (tid == 64) {     // R5
        double s = 0.0;
        for (int i = 0; i < n; i++) s = s + s_z[i];
        s_mean = s / (double)n;
    }
    __syncthreads();
    const double mean_abs = s_sum / ((double)n * (double)n);
    const double lam = lam_rel * mean_abs;
    for (int i = tid; i < n; i += RBF_THREADS) aug[i * ld + i] = aug[i * ld + i] + lam;
    __syncthreads();
    const int st = rbf_lu_solve(aug, N, wout, s_row, s_d, s_key, s_idx);
    for (int i = N + tid; i <= RBF_MAX_SAMPLES; i += RBF_THREADS) wout[i] = 0.0;
    if (tid == 0) {
        mean_all[plane] = st ? 0.0 : s_mean;
        kept_all[plane] = n;
        status_all[plane] = st;
    }
}

// ---- R6 + R7 --------------------------------------------------------------------
// the plane's samples (u, v, w) into LDS, three doubles per sample; 0 samples for a plane that failed
__device__ __forceinline__ int rbf_load_samples(int plane, int K, const double *samp_all, const double *weights_all,
                                                const int *kept_all, const int *status_all, double *s_samp) {
    const int n = status_all[plane] ? 0 : kept_all[plane];
    const double *su = samp_all + (size_t)plane * 2 * K, *sv = su + K;
    const double *sw = weights_all + (size_t)plane * (RBF_MAX_SAMPLES + 1);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        s_samp[3 * i] = su[i];
        s_samp[3 * i + 1] = sv[i];
        s_samp[3 * i + 2] = sw[i];
    }
    __syncthreads();
    return n;
}

// acc[j] of R6 for NP pixels (u[j], v[j]); ONE_ROW: every v[j] is v[0], and dv^2 is computed once per sample
template <int NP, bool ONE_ROW>
__device__ __forceinline__ void rbf_accumulate(const double *s_samp, int n, const double *u, const double *v,
                                               double *acc) {
#pragma unroll
    for (int j = 0; j < NP; j++) acc[j] = 0.0;
    for (int i = 0; i < n; i++) {
        const double su = s_samp[3 * i], sv = s_samp[3 * i + 1], sw = s_samp[3 * i + 2];       // broadcasts
        const double dv0 = v[0] - sv;
        const double dv02 = dv0 * dv0;
#pragma unroll
        for (int j = 0; j < NP; j++) {
            double dv2 = dv02;
            if (!ONE_ROW) {
                const double dv = v[j] - sv;
                dv2 = dv * dv;
            }
            const double du = u[j] - su;
            const double du2 = du * du;
            const double t = sw * rbf_phi(du2 + dv2);
            acc[j] = acc[j] + t;
        }
    }
}

// Lane l of a 64-lane group handles the pixels [g*64*PX + q*256 + 4*l, +4) for
// q < PX/4: k_bkg_apply_vec's layout.
template <typename T>
__global__ __launch_bounds__(256) void k_bkg_rbf_apply_vec(const T *in, float *out, long long nlanes, long long pstride,
                                                           int W, RbfAxes ax, int divide, int K, const double *samp_all,
                                                           const double *weights_all, const double *mean_all,
                                                           const int *kept_all, const int *status_all) {
    extern __shared__ double s_samp[];      // 3 K doubles
    constexpr int PX = 16 / (int)sizeof(T), Q = PX / 4;
    typedef uint32_t raw_t __attribute__((ext_vector_type(sizeof(T))));      // four samples
    const int plane = blockIdx.y;
    const int n = rbf_load_samples(plane, K, samp_all, weights_all, kept_all, status_all, s_samp);
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nlanes) return;
    const long long p0 = (v >> 6) * (64 * PX) + (v & 63) * 4;
    const T *src = in + (long long)plane * pstride + p0;
    float *dst = out + (long long)plane * pstride + p0;
    raw_t raw[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) raw[q] = __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(src + q * 256));
    const int status = status_all[plane];
    const double c0 = weights_all[(size_t)plane * (RBF_MAX_SAMPLES + 1) + n], mean = mean_all[plane];
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
        rvf4 r;
        if (status) {
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = x[j];
        } else {
            const unsigned p = (unsigned)(p0 + q * 256);
            const unsigned row = p / (unsigned)W, col = p - row * (unsigned)W;
            double u[4], vv[4], acc[4];
            if (col + 3 < (unsigned)W) {
#pragma unroll
                for (int j = 0; j < 4; j++) u[j] = rbf_u((int)col + j, ax);
                vv[0] = rbf_v((int)row, ax);
                rbf_accumulate<4, true>(s_samp, n, u, vv, acc);
            } else {        // the lane's pixels go on in the next row (W >= 25: at most once)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned cj = col + j;
                    const bool next = cj >= (unsigned)W;
                    u[j] = rbf_u((int)(next ? cj - (unsigned)W : cj), ax);
                    vv[j] = rbf_v((int)(next ? row + 1 : row), ax);
                }
                rbf_accumulate<4, false>(s_samp, n, u, vv, acc);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = bkg_correct(x[j], acc[j] + c0, mean, divide);
        }
        __builtin_nontemporal_store(r, reinterpret_cast<rvf4 *>(dst + q * 256));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bkg_rbf_apply_scalar(const T *in, float *out, long long p_begin, long long p_end,
                                                              long long pstride, int W, RbfAxes ax, int divide, int K,
                                                              const double *samp_all, const double *weights_all,
                                                              const double *mean_all, const int *kept_all,
                                                              const int *status_all) {
    extern __shared__ double s_samp[];      // 3 K doubles
    const int plane = blockIdx.y;
    const int n = rbf_load_samples(plane, K, samp_all, weights_all, kept_all, status_all, s_samp);
    const long long p = p_begin + (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= p_end) return;
    const float x = bkg_to_float(in[(long long)plane * pstride + p]);
    float r = x;
    if (!status_all[plane]) {
        const unsigned row = (unsigned)p / (unsigned)W, col = (unsigned)p - row * (unsigned)W;
        double u[1], vv[1], acc[1];
        u[0] = rbf_u((int)col, ax);
        vv[0] = rbf_v((int)row, ax);
        rbf_accumulate<1, true>(s_samp, n, u, vv, acc);
        r = bkg_correct(x, acc[0] + weights_all[(size_t)plane * (RBF_MAX_SAMPLES + 1) + n], mean_all[plane], divide);
    }
    out[(long long)plane * pstride + p] = r;
}

}  // namespace sgpu

// ===================================================================== host
namespace {

constexpr size_t RBF_WS_BYTES = (size_t)256 << 20;      // the systems of one k_bkg_rbf_fit launch

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int launch_subsky_rbf(sgpu_context *c, const void *d_in, float *d_out, int P, int W, int H, long pstride,
                      const BkgGrid &g, double tol, double lam_rel, int divide, float *d_med, uint8_t *d_keep,
                      double *d_samp, double *d_weights, double *d_mean, int *d_kept, int *d_status) {
    const long long nbox = (long long)P * g.K, npix = (long long)W * H;
    // the planes of a launch are bounded, not the workspace per plane: (K + 1)(K + 2) doubles each
    const size_t per = ((size_t)g.K + 1) * ((size_t)g.K + 2);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)P, RBF_WS_BYTES / (per * sizeof(double))));
    if (int r = c->rbf_ws.ensure((size_t)chunk * per * sizeof(double))) return r;
    for (hipEvent_t &e : c->rbf_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->rbf_ev[0], c->stream));
    if (int r = sgpu::bkg_launch_box_median(c, d_in, (int)sizeof(T), (long long)pstride, W, g, nbox, d_med)) return r;
    HIP_TRY(hipEventRecord(c->rbf_ev[1], c->stream));
    const RbfAxes ax = rbf_axes(W, H);
    for (int p0 = 0; p0 < P; p0 += chunk)
        hipLaunchKernelGGL(sgpu::k_bkg_rbf_fit, dim3((unsigned)std::min(chunk, P - p0)), dim3(sgpu::RBF_THREADS), 0,
                           c->stream, d_med, g, ax, tol, lam_rel, p0, (double *)c->rbf_ws.p, per, d_keep, d_samp,
                           d_weights, d_mean, d_kept, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->rbf_ev[2], c->stream));
    constexpr int PX = 16 / (int)sizeof(T);
    const bool aligned = aligned16(d_in) && aligned16(d_out) && ((size_t)pstride * sizeof(T)) % 16 == 0 &&
                         ((size_t)pstride * sizeof(float)) % 16 == 0;
    // whole 64-lane groups go through the vector kernel, the rest is the scalar tail
    const long long nlanes = aligned ? npix / (64 * PX) * 64 : 0, tail0 = nlanes * PX;
    const size_t lds = (size_t)g.K * 3 * sizeof(double);
    if (nlanes)
        hipLaunchKernelGGL((sgpu::k_bkg_rbf_apply_vec<T>), dim3((unsigned)((nlanes + 255) / 256), (unsigned)P), dim3(256),
                           lds, c->stream, (const T *)d_in, d_out, nlanes, (long long)pstride, W, ax, divide, g.K, d_samp,
                           d_weights, d_mean, d_kept, d_status);
    if (tail0 < npix)
        hipLaunchKernelGGL((sgpu::k_bkg_rbf_apply_scalar<T>), dim3((unsigned)((npix - tail0 + 255) / 256), (unsigned)P),
                           dim3(256), lds, c->stream, (const T *)d_in, d_out, tail0, npix, (long long)pstride, W, ax,
                           divide, g.K, d_samp, d_weights, d_mean, d_kept, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->rbf_ev[3], c->stream));
    c->rbf_timed = 1;
    return SGPU_OK;
}

}  // namespace

extern "C" int sgpu_bkg_rbf_check(int width, int height, int samples, double tolerance, double smooth) {
    BkgGrid g;
    if (const char *why = rbf_check(width, height, samples, tolerance, smooth, &g)) return fail(SGPU_BAD_ARGUMENT, why);
    return SGPU_OK;
}

extern "C" int sgpu_bkg_rbf_last_kernel_ms(sgpu_context *c, float ms[4]) {
    if (!c || !ms) return fail(SGPU_BAD_ARGUMENT, "bkg_rbf_last_kernel_ms: null argument");
    ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    if (!c->rbf_timed) return SGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->rbf_ev[3]));
    for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&ms[k], c->rbf_ev[k], c->rbf_ev[k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms[3], c->rbf_ev[0], c->rbf_ev[3]));
    return SGPU_OK;
}

extern "C" int sgpu_bkg_rbf_solve_device(sgpu_context *c, int nsys, int order, double *d_aug, double *d_x,
                                         int *d_status) {
    if (!c || nsys < 0 || nsys > 65535) return fail(SGPU_BAD_ARGUMENT, "bkg_rbf_solve: bad argument");
    if (order < 1 || order > RBF_MAX_ORDER) return fail(SGPU_BAD_ARGUMENT, "bkg_rbf_solve: order must be 1 .. 1025");
    if (nsys == 0) return SGPU_OK;
    if (!d_aug || !d_x || !d_status) return fail(SGPU_BAD_ARGUMENT, "bkg_rbf_solve: null argument");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(sgpu::k_bkg_rbf_solve, dim3((unsigned)nsys), dim3(sgpu::RBF_THREADS), 0, c->stream, d_aug, order,
                       d_x, d_status);
    HIP_TRY(hipGetLastError());
    return SGPU_OK;
}

extern "C" int sgpu_subsky_rbf_planes_device(sgpu_context *c, const void *d_in, int elem_size, int nplanes, int width,
                                             int height, long plane_stride, int samples, double tolerance,
                                             double smooth, int divide, float *d_out, float *d_med,
                                             unsigned char *d_keep, double *d_weights, double *d_mean, int *d_kept,
                                             int *d_status, double *lam_rel_out) {
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    BkgGrid g;
    if (const char *why = rbf_check(width, height, samples, tolerance, smooth, &g)) return fail(SGPU_BAD_ARGUMENT, why);
    if (!c || nplanes < 0 || nplanes > 65535 || (long long)width * height >= (1LL << 31))
        return fail(SGPU_BAD_ARGUMENT, "subsky -rbf: bad argument");
    if (plane_stride < (long)width * height) return fail(SGPU_BAD_ARGUMENT, "plane_stride < width*height");
    const double lam_rel = rbf_lam_rel(smooth);
    if (lam_rel_out) *lam_rel_out = lam_rel;
    c->rbf_timed = 0;
    if (nplanes == 0) return SGPU_OK;
    if (!d_in || !d_out) return fail(SGPU_BAD_ARGUMENT, "subsky -rbf: null planes");
    const size_t span = (size_t)(nplanes - 1) * (size_t)plane_stride + (size_t)width * (size_t)height;
    const char *i0 = (const char *)d_in, *i1 = i0 + span * (size_t)elem_size;
    const char *o0 = (const char *)d_out, *o1 = o0 + span * sizeof(float);
    if (i0 < o1 && o0 < i1 && !(elem_size == 4 && i0 == o0))
        return fail(SGPU_BAD_ARGUMENT, "subsky -rbf: the output overlaps the input (in place only for float planes)");
    HIP_TRY(hipSetDevice(c->device));
    // the samples' coordinates, and the result arrays the caller did not give, live in the context
    const size_t P = (size_t)nplanes, K = (size_t)g.K;
    const size_t o_samp = 0, o_w = o_samp + P * 2 * K * sizeof(double),
                 o_mean = o_w + P * (RBF_MAX_SAMPLES + 1) * sizeof(double), o_med = o_mean + P * sizeof(double),
                 o_kept = o_med + P * K * sizeof(float), o_status = o_kept + P * sizeof(int),
                 o_keep = o_status + P * sizeof(int), total = o_keep + P * K;
    if (int r = c->rbf_res.ensure(total)) return r;
    char *ws = (char *)c->rbf_res.p;
    double *d_samp = (double *)(ws + o_samp);
    if (!d_weights) d_weights = (double *)(ws + o_w);
    if (!d_mean) d_mean = (double *)(ws + o_mean);
    if (!d_med) d_med = (float *)(ws + o_med);
    if (!d_kept) d_kept = (int *)(ws + o_kept);
    if (!d_status) d_status = (int *)(ws + o_status);
    if (!d_keep) d_keep = (unsigned char *)(ws + o_keep);
    if (elem_size == 4)
        return launch_subsky_rbf<float>(c, d_in, d_out, nplanes, width, height, plane_stride, g, tolerance, lam_rel,
                                        divide ? 1 : 0, d_med, d_keep, d_samp, d_weights, d_mean, d_kept, d_status);
    return launch_subsky_rbf<uint16_t>(c, d_in, d_out, nplanes, width, height, plane_stride, g, tolerance, lam_rel,
                                       divide ? 1 : 0, d_med, d_keep, d_samp, d_weights, d_mean, d_kept, d_status);
}

// bkg_kernels.h -- what the two background models share on the device
// (background.hip: the polynomial of DESIGN.md 6i; background_rbf.hip: the
// thin-plate spline of 6k): the selection of the sample boxes (B3) as a device
// function of one 1024-thread workgroup, and the launch of the box-median
// kernel (B2), which lives in background.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bkg_host.h"

#pragma clang fp contract(off)

struct sgpu_context;

namespace sgpu {

constexpr int BKG_FIT_THREADS = 1024;

// k_bkg_box_median<WORD or float> over nbox = nplanes * g.K boxes on the context's stream
int bkg_launch_box_median(sgpu_context *c, const void *d_in, int elem_size, long long pstride, int W,
                          const sgpu_bkg_host::BkgGrid &g, long long nbox, float *d_med);

// The elements of ranks r0 and r1 of a[0 .. K) (ascending, ties by index) -> res[0], res[1]:
// every thread counts, for each of its elements (one per 1024 boxes), the elements that sort before it.
__device__ __forceinline__ void bkg_rank_select(const double *a, int K, int r0, int r1, double *res) {
    for (int i = threadIdx.x; i < K; i += BKG_FIT_THREADS) {       // whole wavefronts without an element skip the walk
        const double x = a[i];
        int cnt = 0;
        for (int j = 0; j < K; j++) {
            const double v = a[j];      // one address for the wavefront: a broadcast
            cnt += (int)(v < x) | ((int)(v == x) & (int)(j < i));
        }
        if (cnt == r0) res[0] = x;
        if (cnt == r1) res[1] = x;
    }
    __syncthreads();
}

__device__ __forceinline__ double bkg_lds_median(const double *a, int K, double *res) {
    const bool odd = K & 1;
    bkg_rank_select(a, K, odd ? K / 2 : K / 2 - 1, K / 2, res);
    const double m = odd ? res[0] : (res[0] + res[1]) * 0.5;
    __syncthreads();        // res and a are free again
    return m;
}

// B3 of one plane by one workgroup of BKG_FIT_THREADS: the medians of the K box medians and of their
// deviations by rank counting in LDS, the keep mask (s_keep, and keep_out in global memory) and the
// number kept, which every thread returns.  s_d: K doubles, s_med: K floats, s_keep: K bytes,
// s_res: 2 doubles, s_kept: one int, all LDS; s_d and s_res are free again on return.
__device__ __forceinline__ int bkg_select_lds(const float *med, int K, double tol, double *s_d, float *s_med,
                                              uint8_t *s_keep, double *s_res, int *s_kept, uint8_t *keep_out) {
    using namespace sgpu_bkg_host;
    const int tid = threadIdx.x;
    if (tid == 0) *s_kept = 0;
    for (int k = tid; k < K; k += BKG_FIT_THREADS) {
        const float m = med[k];
        s_med[k] = m;
        s_d[k] = (double)m;
    }
    __syncthreads();
    const double m = bkg_lds_median(s_d, K, s_res);
    for (int k = tid; k < K; k += BKG_FIT_THREADS) s_d[k] = fabs((double)s_med[k] - m);
    __syncthreads();
    const double mad = bkg_lds_median(s_d, K, s_res);
    const double T = m + tol * mad;
    int mine = 0;
    for (int k = tid; k < K; k += BKG_FIT_THREADS) {
        const uint8_t kp = bkg_keep(s_med[k], T) ? 1 : 0;
        s_keep[k] = kp;
        keep_out[k] = kp;
        mine += kp;
    }
    if (mine) atomicAdd(s_kept, mine);
    __syncthreads();
    return *s_kept;
}

}  // namespace sgpu

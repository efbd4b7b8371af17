// psf_fit.hip -- Gaussian / Moffat PSF fit of found stars (DESIGN.md 6g,
// restated in tests/psf_ref.py): Levenberg-Marquardt in double on the raw box
// of every star, thousands of small independent fits in one launch.
//
// PARITY STATUS: Siril's source was not available.  The fit is modelled on
// Siril's psf.c (a damped least-squares fit of an elliptical profile to the
// box around a detected star); its arithmetic is the specification in
// DESIGN.md 6g.  Parity with Siril itself is unpinned.
//
// k_psf_fit: one 64-lane workgroup (one wavefront) per star, the stars of all
// frames in one launch; the frame comes from the job record, so the launch
// does not depend on how the stars spread over the frames.  The box is read
// from memory once into LDS (at most 33^2 floats; a sample left out of the fit
// is stored as NaN); lane l owns samples l, l + 64, ... (at most 18).  An
// evaluation accumulates, per lane, the packed lower triangle of J^T J, J^T r
// and chi^2 (36 + 8 + 1 doubles at 8 parameters) in registers; the wavefront
// adds them in a fixed butterfly (lane ^ 32, ^ 16, ... ^ 1), after which every
// lane holds the same bits, so the Cholesky solve and the accept / reject
// decision run redundantly and identically in every lane.  The sums of the
// current point wait in LDS while a trial point is evaluated.  Nothing is
// written to memory before the fit ends; there are no atomics; the record of
// a star depends on its job alone.
//
// SGPU_PSF_REDUCE_LDS=1 builds the A/B variant whose wavefront sum is a tree
// in LDS (same pairing, hence the same bits) instead of cross-lane shuffles.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "psf_host.h"
#include "sgpu_internal.h"

#pragma clang fp contract(off)

#ifndef SGPU_PSF_REDUCE_LDS
#define SGPU_PSF_REDUCE_LDS 0
#endif

namespace sgpu {

using sgpu_psf_host::PsfJob;

constexpr int PSF_MAXN = (2 * sgpu_psf_host::PSF_MAXR + 1) * (2 * sgpu_psf_host::PSF_MAXR + 1);
constexpr double PSF_MU0 = 1e-3, PSF_MU_MIN = 1e-12, PSF_MU_MAX = 1e10, PSF_CONV = 1e-12;

struct PsfP {
    double min_fwhm, max_fwhm, roundness_min, sat;
    int max_iter, pad;
};

__host__ __device__ constexpr int psf_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // j <= i

// J^T J (packed lower triangle), J^T r and chi^2 of this lane's samples at the point p
// (B, A, x0, y0, a, b, c, beta); true when a model value is not finite
template <int PROFILE, int NP, int NT>
__device__ inline bool psf_eval(const float *s_val, int n, int side, int b, int lane, const double (&p)[8],
                                double (&acc)[NT]) {
    constexpr int NTRI = NP * (NP + 1) / 2;
#pragma unroll
    for (int k = 0; k < NT; k++) acc[k] = 0.0;
    bool nonfinite = false;
    const double B = p[0], A = p[1], x0 = p[2], y0 = p[3], a = p[4], bq = p[5], c = p[6], beta = p[7];
    const int dq = 64 / side, dr = 64 - dq * side;
    for (int i = lane, r = lane / side, cc = lane - r * side; i < n; i += 64) {
        const float sv = s_val[i];
        if (sv == sv) {
            const double u = (double)(cc - b) - x0, v = (double)(r - b) - y0;
            const double Q = a * u * u + 2.0 * bq * u * v + c * v * v;
            double J[NP], E, g;
            if constexpr (PROFILE == SGPU_PSF_GAUSSIAN) {
                E = exp(-Q / 2.0);
                g = -A * E / 2.0;
            } else {
                const double q1 = 1.0 + Q;
                E = pow(q1, -beta);
                g = -beta * A * E / q1;
                if constexpr (NP == 8) J[7] = -A * E * log(q1);
            }
            const double f = B + A * E;
            nonfinite |= !isfinite(f);
            const double res = (double)sv - f;
            J[0] = 1.0;
            J[1] = E;
            J[2] = g * (-2.0 * a * u - 2.0 * bq * v);
            J[3] = g * (-2.0 * bq * u - 2.0 * c * v);
            J[4] = g * u * u;
            J[5] = 2.0 * g * u * v;
            J[6] = g * v * v;
#pragma unroll
            for (int i2 = 0; i2 < NP; i2++) {
#pragma unroll
                for (int j2 = 0; j2 <= i2; j2++) acc[psf_tri(i2, j2)] += J[i2] * J[j2];
                acc[NTRI + i2] += J[i2] * res;
            }
            acc[NT - 1] += res * res;
        }
        cc += dr;
        r += dq;
        if (cc >= side) {
            cc -= side;
            r++;
        }
    }
    return nonfinite;
}

// sum over the wavefront, the same bits in every lane: pairs (l, l ^ 32), then ^ 16, ... ^ 1
template <int NT>
__device__ inline void psf_reduce(double (&acc)[NT], double *s_red, int lane) {
#if SGPU_PSF_REDUCE_LDS
#pragma unroll
    for (int k = 0; k < NT; k++) s_red[k * 64 + lane] = acc[k];
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (lane < s) {
#pragma unroll
            for (int k = 0; k < NT; k++) s_red[k * 64 + lane] += s_red[k * 64 + lane + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NT; k++) acc[k] = s_red[k * 64];
    __syncthreads();
#else
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int k = 0; k < NT; k++) acc[k] += __shfl_xor(acc[k], m, 64);
    }
#endif
}

// (J^T J + mu diag(J^T J)) x = J^T r by Cholesky; false at a non-positive or non-finite pivot
template <int NP>
__device__ inline bool psf_solve(const double *s_cur, double mu, double (&x)[NP]) {
    constexpr int NTRI = NP * (NP + 1) / 2;
    double L[NTRI], y[NP];
#pragma unroll
    for (int k = 0; k < NTRI; k++) L[k] = s_cur[k];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const double d = L[psf_tri(i, i)];
        L[psf_tri(i, i)] = d + mu * d;
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        double d = L[psf_tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[psf_tri(j, k)] * L[psf_tri(j, k)];
        if (!(d > 0.0) || !isfinite(d)) ok = false;
        const double ljj = sqrt(d);
        L[psf_tri(j, j)] = ljj;
#pragma unroll
        for (int i = j + 1; i < NP; i++) {
            double s = L[psf_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[psf_tri(i, k)] * L[psf_tri(j, k)];
            L[psf_tri(i, j)] = s / ljj;
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        double s = s_cur[NTRI + i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[psf_tri(i, k)] * y[k];
        y[i] = s / L[psf_tri(i, i)];
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < NP; k++) s -= L[psf_tri(k, i)] * x[k];
        x[i] = s / L[psf_tri(i, i)];
    }
    return ok;
}

template <int NP>
__device__ inline bool psf_valid(const double (&p)[8]) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < NP; k++) fin = fin && isfinite(p[k]);
    return fin && p[1] > 0.0 && p[4] > 0.0 && p[6] > 0.0 && p[4] * p[6] - p[5] * p[5] > 0.0 &&
           p[7] >= sgpu_psf_host::PSF_BETA_MIN && p[7] <= sgpu_psf_host::PSF_BETA_MAX;
}

__device__ inline bool psf_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

template <typename T, int PROFILE, int NP>
__global__ __launch_bounds__(64) void k_psf_fit(const T *in, long long rstride, long long fstride, const PsfJob *jobs,
                                                PsfP pp, sgpu_psf *out) {
    constexpr int NTRI = NP * (NP + 1) / 2, NT = NTRI + NP + 1;
    __shared__ float s_val[PSF_MAXN];
    __shared__ double s_cur[NT];
#if SGPU_PSF_REDUCE_LDS
    __shared__ double s_red[NT * 64];
#else
    double *s_red = nullptr;
#endif
    const int lane = threadIdx.x;
    const PsfJob job = jobs[blockIdx.x];
    const int b = job.b, side = 2 * b + 1, n = side * side;

    // the box: one read of every sample; the host checked that it lies inside the frame
    int nused = 0;
    bool bad = false;
    {
        const T *box = in + (long long)job.frame * fstride + (long long)(job.py - b) * rstride + (job.px - b);
        const int dq = 64 / side, dr = 64 - dq * side;
        for (int i = lane, r = lane / side, cc = lane - r * side; i < n; i += 64) {
            const float v = (float)box[(long long)r * rstride + cc];
            bad |= !isfinite(v);
            const bool use = !((double)v >= pp.sat);
            s_val[i] = use ? v : NAN;
            nused += use;
            cc += dr;
            r += dq;
            if (cc >= side) {
                cc -= side;
                r++;
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) nused += __shfl_xor(nused, m, 64);
    bad = __any(bad) != 0;
    nused = bad ? 0 : nused;
    __syncthreads();

    double p[8], pn[8];
    pn[0] = job.bg;
    pn[1] = job.amp;
    pn[2] = job.x0;
    pn[3] = job.y0;
    pn[4] = job.lam;
    pn[5] = 0.0;
    pn[6] = job.lam;
    pn[7] = PROFILE == SGPU_PSF_MOFFAT ? job.beta : 1.0;   // a Gaussian has no beta: any value in range
#pragma unroll
    for (int k = 0; k < 8; k++) p[k] = pn[k];
    int status = (bad || nused < NP + 1) ? 3 : -1, it = 0;
    double chi2 = 0.0, mu = PSF_MU0;
    bool first = true, solved = true;
    while (psf_uniform(status < 0)) {
        // the trial point (the start, the first time round)
        bool ok = psf_uniform(solved && psf_valid<NP>(pn));
        double chi2n = 0.0;
        if (ok) {
            double acc[NT];
            const bool nf = psf_eval<PROFILE, NP, NT>(s_val, n, side, b, lane, pn, acc);
            psf_reduce<NT>(acc, s_red, lane);
            chi2n = acc[NT - 1];
            ok = psf_uniform(!__any(nf) && (first || chi2n <= chi2));
            if (ok) {
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < NT; k++) s_cur[k] = acc[k];
                }
                __syncthreads();
            }
        }
        if (first) {
            if (!ok) status = 3;
        } else if (ok) {
            mu = fmax(mu / 10.0, PSF_MU_MIN);
            it++;
            if (chi2 - chi2n <= PSF_CONV * chi2) status = 0;
            else if (it >= pp.max_iter) status = 1;
        } else {
            mu = 10.0 * mu;
            if (mu > PSF_MU_MAX) status = 2;
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < 8; k++) p[k] = pn[k];
            chi2 = chi2n;
        }
        first = false;
        if (psf_uniform(status < 0)) {
            double d[NP];
            solved = psf_solve<NP>(s_cur, mu, d);
#pragma unroll
            for (int k = 0; k < NP; k++) pn[k] = p[k] + d[k];
        }
    }

    if (lane != 0) return;
    sgpu_psf rec;
    const double a = p[4], bq = p[5], c = p[6];
    const double beta = PROFILE == SGPU_PSF_MOFFAT ? p[7] : 0.0;
    rec.x = (double)job.px + p[2];
    rec.y = (double)job.py + p[3];
    rec.bkg = p[0];
    rec.amp = p[1];
    rec.fwhm_major = rec.fwhm_minor = rec.roundness = rec.angle = 0.0;
    if (a > 0.0 && c > 0.0) {
        const double k = PROFILE == SGPU_PSF_MOFFAT ? 2.0 * sqrt(pow(2.0, 1.0 / beta) - 1.0) : sgpu_psf_host::PSF_FWHM_K;
        const double hd = (a - c) / 2.0;
        const double q = sqrt(hd * hd + bq * bq);
        const double l1 = (a + c) / 2.0 + q, l2 = (a + c) / 2.0 - q;
        rec.fwhm_major = l2 > 0.0 ? k / sqrt(l2) : 0.0;
        rec.fwhm_minor = l1 > 0.0 ? k / sqrt(l1) : 0.0;
        rec.roundness = rec.fwhm_major > 0.0 ? rec.fwhm_minor / rec.fwhm_major : 0.0;
        const double t = 0.5 * atan2(2.0 * bq, a - c) * (180.0 / 3.14159265358979323846);
        rec.angle = t <= 0.0 ? t + 90.0 : t - 90.0;
    }
    rec.beta = beta;
    rec.rmse = status == 3 ? 0.0 : sqrt(chi2 / (double)(nused - NP));
    rec.a = a;
    rec.b = bq;
    rec.c = c;
    rec.nused = nused;
    rec.iterations = it;
    if (status == 0) {
        const double half = (double)b / 2.0;
        if (fabs(p[2]) > half || fabs(p[3]) > half) status = 4;
        else if (rec.fwhm_minor < pp.min_fwhm || rec.fwhm_major > pp.max_fwhm) status = 5;
        else if (rec.roundness < pp.roundness_min) status = 6;
    }
    rec.status = status;
    rec.reserved = 0;
    out[blockIdx.x] = rec;
}

}  // namespace sgpu

using sgpu_host::fail;

extern "C" void sgpu_psf_default_params(sgpu_psf_params *p) {
    if (!p) return;
    p->beta = 0.0;
    p->min_fwhm = 1.0;
    p->roundness_min = 0.5;
    p->sat = INFINITY;
    p->profile = SGPU_PSF_GAUSSIAN;
    p->radius = 10;
    p->max_iter = 50;
    p->reserved = 0;
}

namespace {

template <typename T>
void launch_psf(int profile, bool free_beta, unsigned njobs, hipStream_t st, const void *in, long long rs, long long fs,
                const sgpu::PsfJob *jobs, const sgpu::PsfP &pp, sgpu_psf *out) {
    const dim3 grid(njobs), block(64);
    if (profile == SGPU_PSF_GAUSSIAN)
        hipLaunchKernelGGL((sgpu::k_psf_fit<T, SGPU_PSF_GAUSSIAN, 7>), grid, block, 0, st, (const T *)in, rs, fs, jobs, pp,
                           out);
    else if (free_beta)
        hipLaunchKernelGGL((sgpu::k_psf_fit<T, SGPU_PSF_MOFFAT, 8>), grid, block, 0, st, (const T *)in, rs, fs, jobs, pp,
                           out);
    else
        hipLaunchKernelGGL((sgpu::k_psf_fit<T, SGPU_PSF_MOFFAT, 7>), grid, block, 0, st, (const T *)in, rs, fs, jobs, pp,
                           out);
}

}  // namespace

extern "C" int sgpu_fit_stars_device(sgpu_context *c, const void *d_frames, int elem_size, int nframes, int width,
                                     int height, long row_stride, long frame_stride, const double *bg,
                                     const sgpu_star *stars, const int *nstars, int max_stars,
                                     const sgpu_psf_params *p, sgpu_psf *psf) {
    if (!c || !d_frames || !bg || !stars || !nstars || !p || !psf || nframes < 1 || width < 1 || height < 1 ||
        max_stars < 1 || row_stride < width || frame_stride < (long)(height - 1) * row_stride + width)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (elem_size != 2 && elem_size != 4) return fail(SGPU_BAD_ARGUMENT, "element size must be 2 or 4");
    if (const char *why = sgpu_psf_host::psf_check_params(p)) return fail(SGPU_BAD_ARGUMENT, why);
    std::vector<sgpu::PsfJob> jobs;
    if (const char *why = sgpu_psf_host::psf_flatten(stars, nstars, nframes, max_stars, width, height, bg, p, jobs))
        return fail(SGPU_BAD_ARGUMENT, why);
    c->psf_ms = 0.f;
    if (jobs.empty()) return SGPU_OK;

    const size_t nj = jobs.size();
    const sgpu::PsfP pp = {p->min_fwhm, (double)(2 * p->radius + 1), p->roundness_min, p->sat, p->max_iter, 0};
    HIP_TRY(hipSetDevice(c->device));
    for (int k = 0; k < 2; k++)
        if (!c->psf_ev[k]) HIP_TRY(hipEventCreate(&c->psf_ev[k]));
    if (int rc = c->psf_jobs.ensure(nj * sizeof(sgpu::PsfJob))) return rc;
    if (int rc = c->psf_out.ensure(nj * sizeof(sgpu_psf))) return rc;
    HIP_TRY(hipMemcpyAsync(c->psf_jobs.p, jobs.data(), nj * sizeof(sgpu::PsfJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->psf_ev[0], c->stream));
    if (elem_size == 4)
        launch_psf<float>(p->profile, sgpu_psf_host::psf_free_beta(p), (unsigned)nj, c->stream, d_frames, row_stride,
                          frame_stride, (const sgpu::PsfJob *)c->psf_jobs.p, pp, (sgpu_psf *)c->psf_out.p);
    else
        launch_psf<uint16_t>(p->profile, sgpu_psf_host::psf_free_beta(p), (unsigned)nj, c->stream, d_frames,
                             row_stride, frame_stride, (const sgpu::PsfJob *)c->psf_jobs.p, pp,
                             (sgpu_psf *)c->psf_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->psf_ev[1], c->stream));
    std::vector<sgpu_psf> rec(nj);
    HIP_TRY(hipMemcpyAsync(rec.data(), c->psf_out.p, nj * sizeof(sgpu_psf), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->psf_ms, c->psf_ev[0], c->psf_ev[1]));
    size_t j = 0;
    for (int f = 0; f < nframes; f++) {
        if (nstars[f])
            std::memcpy(psf + (size_t)f * (size_t)max_stars, rec.data() + j, (size_t)nstars[f] * sizeof(sgpu_psf));
        j += (size_t)nstars[f];
    }
    return SGPU_OK;
}

extern "C" int sgpu_psf_last_kernel_ms(sgpu_context *c, float *ms) {
    if (!c || !ms) return fail(SGPU_BAD_ARGUMENT, "bad argument");
    *ms = c->psf_ms;
    return SGPU_OK;
}

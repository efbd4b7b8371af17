// psf_host.h -- the host side of the PSF fit that needs no
// device: parameter checks, the box of every star, the isotropic start and the
// flat job list with its per-star frame index.  Plain C++ (no HIP header), so
// it also compiles into a stand-alone program (tests/hostsim/psf_host_main.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/sirilgpu.h"

namespace sgpu_psf_host {

constexpr int PSF_MAXR = 16;
constexpr double PSF_FWHM_K = 2.3548200450309493;
constexpr double PSF_BETA0 = 2.5, PSF_BETA_MIN = 0.5, PSF_BETA_MAX = 10.0;

// one star of the launch: 64 bytes, read by every lane of its wavefront
struct PsfJob {
    double bg, amp, x0, y0;   // start: B, A, centre offsets from (px, py)
    double lam, beta;         // start: a = c = lam; beta (start or fixed value, 0 for a Gaussian)
    int frame, px, py, b;     // frame index, box centre, box half-size
};

inline double psf_moffat_k(double beta) { return 2.0 * std::sqrt(std::pow(2.0, 1.0 / beta) - 1.0); }

inline bool psf_free_beta(const sgpu_psf_params *p) { return p->profile == SGPU_PSF_MOFFAT && !(p->beta > 0.0); }

// nullptr when the parameters are in range, else what is wrong
inline const char *psf_check_params(const sgpu_psf_params *p) {
    if (p->profile != SGPU_PSF_GAUSSIAN && p->profile != SGPU_PSF_MOFFAT) return "fit_stars: unknown profile";
    if (p->radius < 1 || p->radius > PSF_MAXR) return "fit_stars: 1 <= radius <= 16";
    if (p->max_iter < 1 || p->max_iter > 1000) return "fit_stars: 1 <= max_iter <= 1000";
    if (p->profile == SGPU_PSF_MOFFAT && p->beta > 0.0 && !(p->beta >= PSF_BETA_MIN && p->beta <= PSF_BETA_MAX))
        return "fit_stars: a fixed beta lies in 0.5 .. 10";
    if (std::isnan(p->beta) || !(p->min_fwhm >= 0.0) || !std::isfinite(p->min_fwhm) || !(p->roundness_min >= 0.0) ||
        !(p->roundness_min <= 1.0) || std::isnan(p->sat))
        return "fit_stars: parameter out of range";
    return nullptr;
}

// The stars of all frames (stars[f * max_stars + s], s < nstars[f]) as one job
// list, frame after frame.  nullptr, or what is wrong (jobs is then undefined).
inline const char *psf_flatten(const sgpu_star *stars, const int *nstars, int nframes, int max_stars, int width,
                               int height, const double *bg, const sgpu_psf_params *p, std::vector<PsfJob> &jobs) {
    jobs.clear();
    size_t total = 0;
    for (int f = 0; f < nframes; f++) {
        if (nstars[f] < 0 || nstars[f] > max_stars) return "fit_stars: nstars outside 0 .. max_stars";
        if (!std::isfinite(bg[f])) return "fit_stars: bg must be finite";
        total += (size_t)nstars[f];
    }
    if (total > 0x7fffffffu) return "fit_stars: too many stars";
    jobs.reserve(total);
    const bool moffat = p->profile == SGPU_PSF_MOFFAT;
    const double beta = !moffat ? 0.0 : (p->beta > 0.0 ? p->beta : PSF_BETA0);
    const double k = moffat ? psf_moffat_k(beta) : PSF_FWHM_K;
    for (int f = 0; f < nframes; f++)
        for (int s = 0; s < nstars[f]; s++) {
            const sgpu_star &st = stars[(size_t)f * (size_t)max_stars + (size_t)s];
            int e = st.ext[0];
            for (int d = 1; d < 4; d++) e = st.ext[d] > e ? st.ext[d] : e;
            if (e < 0 || e > PSF_MAXR) return "fit_stars: star extent outside 0 .. 16";
            PsfJob j;
            j.b = e + 2 < p->radius ? e + 2 : p->radius;
            if (st.px < j.b || st.py < j.b || st.px >= width - j.b || st.py >= height - j.b)
                return "fit_stars: the box of a star leaves the frame";
            j.frame = f;
            j.px = st.px;
            j.py = st.py;
            j.bg = bg[f];
            j.amp = st.amp;
            j.x0 = st.x - (double)st.px;
            j.y0 = st.y - (double)st.py;
            const double f0 = std::sqrt(st.fwhm_major * st.fwhm_minor);
            j.lam = f0 > 0.0 ? (k / f0) * (k / f0) : NAN;   // a record without a width is not fitted (status 3)
            j.beta = beta;
            jobs.push_back(j);
        }
    return nullptr;
}

}  // namespace sgpu_psf_host

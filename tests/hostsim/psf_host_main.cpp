// psf_host_main.cpp -- stand-alone driver of the PSF fit's host side
// (siril_amd/csrc/psf_host.h: parameter checks, boxes, starts, the flat job
// list and its frame table), for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all psf_host_main.cpp -o psf_host_main
// Exit status 0 and "psf host ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siril_amd/csrc/psf_host.h"

using namespace sgpu_psf_host;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);  \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static sgpu_psf_params defaults() {
    sgpu_psf_params p;
    std::memset(&p, 0, sizeof p);
    p.min_fwhm = 1.0;
    p.roundness_min = 0.5;
    p.sat = INFINITY;
    p.profile = SGPU_PSF_GAUSSIAN;
    p.radius = 10;
    p.max_iter = 50;
    return p;
}

static sgpu_star star(int px, int py, int e0, int e1, int e2, int e3, double fwhm) {
    sgpu_star s;
    std::memset(&s, 0, sizeof s);
    s.px = px;
    s.py = py;
    s.x = px + 0.25;
    s.y = py - 0.125;
    s.amp = 0.5;
    s.fwhm_major = fwhm * 2.0;
    s.fwhm_minor = fwhm / 2.0;
    s.ext[0] = e0;
    s.ext[1] = e1;
    s.ext[2] = e2;
    s.ext[3] = e3;
    return s;
}

int main() {
    // parameter checks
    sgpu_psf_params p = defaults();
    CHECK(psf_check_params(&p) == nullptr);
    for (int bad = 0; bad < 9; bad++) {
        sgpu_psf_params q = defaults();
        switch (bad) {
            case 0: q.profile = 2; break;
            case 1: q.radius = 0; break;
            case 2: q.radius = 17; break;
            case 3: q.max_iter = 0; break;
            case 4: q.profile = SGPU_PSF_MOFFAT; q.beta = 0.25; break;
            case 5: q.profile = SGPU_PSF_MOFFAT; q.beta = 11.0; break;
            case 6: q.min_fwhm = -1.0; break;
            case 7: q.roundness_min = 1.5; break;
            default: q.sat = NAN; break;
        }
        CHECK(psf_check_params(&q) != nullptr);
    }
    p.profile = SGPU_PSF_MOFFAT;
    CHECK(psf_check_params(&p) == nullptr && psf_free_beta(&p));
    p.beta = 3.0;
    CHECK(psf_check_params(&p) == nullptr && !psf_free_beta(&p));

    // three frames of 97 x 53 with 2, 0 and 3 stars in lists of max_stars = 3
    const int W = 97, H = 53, MS = 3;
    std::vector<sgpu_star> stars((size_t)3 * MS);
    const int nstars[3] = {2, 0, 3};
    const double bg[3] = {0.05, 0.06, 0.07};
    stars[0] = star(20, 15, 4, 5, 3, 2, 3.5);        // b = min(10, 5 + 2) = 7
    stars[1] = star(10, 10, 8, 8, 8, 9, 3.5);        // b = 10: the box touches column 0 and row 0
    stars[6] = star(86, 42, 9, 9, 9, 9, 3.5);        // b = 10: the box touches the last column and row
    stars[7] = star(50, 25, 0, 0, 0, 0, 0.0);        // no width: lam is NaN (status 3 on the device)
    stars[8] = star(30, 30, 16, 1, 1, 1, 2.0);
    std::vector<PsfJob> jobs;
    p = defaults();
    CHECK(psf_flatten(stars.data(), nstars, 3, MS, W, H, bg, &p, jobs) == nullptr);
    CHECK(jobs.size() == 5);
    if (jobs.size() == 5) {
        const int frame[5] = {0, 0, 2, 2, 2}, b[5] = {7, 10, 10, 2, 10};
        for (int j = 0; j < 5; j++) {
            CHECK(jobs[j].frame == frame[j] && jobs[j].b == b[j] && jobs[j].bg == bg[frame[j]]);
            CHECK(jobs[j].px - jobs[j].b >= 0 && jobs[j].px + jobs[j].b < W);
            CHECK(jobs[j].py - jobs[j].b >= 0 && jobs[j].py + jobs[j].b < H);
            CHECK(jobs[j].x0 == 0.25 && jobs[j].y0 == -0.125 && jobs[j].amp == 0.5 && jobs[j].beta == 0.0);
        }
        CHECK(jobs[0].lam == (PSF_FWHM_K / 3.5) * (PSF_FWHM_K / 3.5));
        CHECK(std::isnan(jobs[3].lam));
    }
    // Moffat: the start scales with 2 sqrt(2^(1/beta) - 1); the fixed beta travels with the job
    p.profile = SGPU_PSF_MOFFAT;
    p.beta = 3.0;
    CHECK(psf_flatten(stars.data(), nstars, 3, MS, W, H, bg, &p, jobs) == nullptr && jobs.size() == 5);
    if (jobs.size() == 5) {
        const double k = 2.0 * std::sqrt(std::pow(2.0, 1.0 / 3.0) - 1.0);
        CHECK(jobs[0].beta == 3.0 && jobs[0].lam == (k / 3.5) * (k / 3.5));
    }
    p.beta = 0.0;
    CHECK(psf_flatten(stars.data(), nstars, 3, MS, W, H, bg, &p, jobs) == nullptr && jobs[4].beta == PSF_BETA0);
    // a smaller radius caps every box
    p = defaults();
    p.radius = 3;
    CHECK(psf_flatten(stars.data(), nstars, 3, MS, W, H, bg, &p, jobs) == nullptr);
    for (const PsfJob &j : jobs) CHECK(j.b == (j.px == 50 ? 2 : 3));
    // boxes that leave the frame, one edge at a time; bad lists
    p = defaults();
    const int off[4][2] = {{9, 20}, {87, 20}, {40, 9}, {40, 43}};
    for (int k = 0; k < 4; k++) {
        std::vector<sgpu_star> one(1, star(off[k][0], off[k][1], 8, 8, 8, 8, 3.5));
        const int n1[1] = {1};
        CHECK(psf_flatten(one.data(), n1, 1, 1, W, H, bg, &p, jobs) != nullptr);
    }
    {
        std::vector<sgpu_star> one(1, star(40, 25, 17, 1, 1, 1, 3.5));
        const int n1[1] = {1}, over[1] = {2}, neg[1] = {-1}, none[1] = {0};
        const double nanbg[1] = {NAN};
        CHECK(psf_flatten(one.data(), n1, 1, 1, W, H, bg, &p, jobs) != nullptr);       // extent out of range
        one[0] = star(40, 25, 3, 3, 3, 3, 3.5);
        CHECK(psf_flatten(one.data(), over, 1, 1, W, H, bg, &p, jobs) != nullptr);
        CHECK(psf_flatten(one.data(), neg, 1, 1, W, H, bg, &p, jobs) != nullptr);
        CHECK(psf_flatten(one.data(), n1, 1, 1, W, H, nanbg, &p, jobs) != nullptr);
        CHECK(psf_flatten(one.data(), none, 1, 1, W, H, bg, &p, jobs) == nullptr && jobs.empty());
        CHECK(psf_flatten(one.data(), n1, 1, 1, W, H, bg, &p, jobs) == nullptr && jobs.size() == 1);
    }
    if (failures) return 1;
    std::printf("psf host ok\n");
    return 0;
}

"""The PSF fit's restatement (tests/psf_ref.py) on planted
stars: it converges on every one well inside the iteration cap, recovers
position and width, returns the planted parameters of a noise-free star, and
ends with the documented status for a NaN in the box and for an elongated
star.  No GPU: this pins the contract the GPU fit is compared against."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as PR  # noqa: E402
import psf_scenes as PS  # noqa: E402
import star_ref as SR  # noqa: E402

SEEDS = {"gaussian": 11, "moffat": 12}
# Measured on the restatement with these seeds (200 stars per profile):
#             accepted steps   centre error px      FWHM error (worse axis)
#                    max       median    max        median    max
MEASURED = {"gaussian": (8, 0.00699, 0.1120, 0.00343, 0.0351),
            "moffat": (28, 0.00834, 0.0949, 0.00585, 0.0597)}


@pytest.fixture(scope="module", params=["gaussian", "moffat"])
def fits(request):
    profile = request.param
    stars = PS.planted(profile, 200, SEEDS[profile])
    recs = [PR.fit_star(s["img"], s["star"], PS.BG, profile, radius=16, roundness_min=0.0) for s in stars]
    return profile, stars, recs


def test_planted_stars_converge_and_are_recovered(fits):
    profile, stars, recs = fits
    assert min(s["b"] for s in stars) <= 4 and max(s["b"] for s in stars) == 16
    assert all(r["status"] == 0 for r in recs)
    its = [r["iterations"] for r in recs]
    assert max(its) < 50                                            # the cap is never reached
    ce = np.array([math.hypot(r["x"] - (s["star"]["px"] + s["cx"] - round(s["cx"])),
                              r["y"] - (s["star"]["py"] + s["cy"] - round(s["cy"]))) for r, s in zip(recs, stars)])
    fe = np.array([max(abs(r["fwhm_major"] / s["fwhm_major"] - 1), abs(r["fwhm_minor"] / s["fwhm_minor"] - 1))
                   for r, s in zip(recs, stars)])
    print(f"{profile}: steps max {max(its)}, centre median {np.median(ce):.5f} max {ce.max():.5f} px, "
          f"fwhm median {np.median(fe):.5f} max {fe.max():.5f}")
    m_its, m_cmed, m_cmax, m_fmed, m_fmax = MEASURED[profile]
    assert max(its) == m_its
    assert np.median(ce) < 2 * m_cmed and ce.max() < 2 * m_cmax
    assert np.median(fe) < 2 * m_fmed and fe.max() < 2 * m_fmax
    if profile == "moffat":
        assert all(PR.BETA_MIN <= r["beta"] <= PR.BETA_MAX for r in recs)
    for r, s in zip(recs, stars):
        assert r["nused"] == (2 * s["b"] + 1) ** 2
        assert 0 < r["roundness"] <= 1 and -90 < r["angle"] <= 90 and r["rmse"] < 2 * PS.NOISE


@pytest.mark.parametrize("profile,beta", [("gaussian", None), ("moffat", None), ("moffat", 2.5)])
def test_noise_free_star_returns_the_planted_parameters(profile, beta):
    """No noise, float64 samples, b = 8: the least-squares minimum is the
    planted point itself (chi^2 = 0 there), and the fit reaches it to 1e-9."""
    for s in PS.planted(profile, 40, 21, noise=0.0, dtype=np.float64):
        if s["b"] == 8:
            break
    assert s["b"] == 8
    r = PR.fit_star(s["img"], s["star"], PS.BG, profile, beta, radius=16, roundness_min=0.0)
    assert r["status"] == 0 and r["nused"] == 17 * 17
    x0, y0 = s["cx"] - round(s["cx"]), s["cy"] - round(s["cy"])
    rel = lambda got, want: abs(got - want) / abs(want)
    assert rel(r["x"] - s["star"]["px"], x0) < 1e-9 and rel(r["y"] - s["star"]["py"], y0) < 1e-9
    for k, want in (("bkg", PS.BG), ("amp", s["amp"]), ("a", s["a"]), ("b", s["b_"]), ("c", s["c"]),
                    ("fwhm_major", s["fwhm_major"]), ("fwhm_minor", s["fwhm_minor"])):
        assert rel(r[k], want) < 1e-9, k
    if profile == "moffat":
        assert rel(r["beta"], 2.5) < 1e-9
    # the angle is the direction of the major axis (the eigenvector of the smaller eigenvalue)
    t = math.radians(r["angle"])
    l2 = s["a"] * math.cos(t) ** 2 + 2 * s["b_"] * math.cos(t) * math.sin(t) + s["c"] * math.sin(t) ** 2
    assert rel(l2, (PR.FWHM_K if profile == "gaussian" else PR.moffat_k(2.5)) ** 2 / s["fwhm_major"] ** 2) < 1e-9


@pytest.fixture(scope="module")
def scene_candidates():
    fr = PS.scene_97x53(np.float32)[0]
    bg, noise, prm = PS.units(np.float32, PS.SCENE)
    return fr, SR.find_stars(fr, bg, noise, **prm)[1]


def _at(cand, x, y):
    return cand[(cand["px"] == x) & (cand["py"] == y)][0]


@pytest.mark.parametrize("profile,beta", [("gaussian", None), ("moffat", 3.0)])
def test_status_of_the_scene_cases(scene_candidates, profile, beta):
    """The scene's stars are Gaussians, so the Moffat runs with beta fixed: a
    free beta runs towards the Gaussian limit and stops at its bound of 10
    (status 1 after 50 steps)."""
    fr, cand = scene_candidates
    # the NaN inside the box of the star at (20, 15): nothing is fitted
    a = _at(cand, 20, 15)
    b = PR.half_size(a["ext"], 6)
    assert abs(PS.NAN_AT[0] - 20) <= b and abs(PS.NAN_AT[1] - 15) <= b
    r = PR.fit_star(fr, a, PS.BG, profile, beta, radius=6, sat=0.9)
    assert r["status"] == 3 and r["iterations"] == 0
    # the 2.5 : 1 star: the fit converges and the roundness test rejects it
    r = PR.fit_star(fr, _at(cand, 55, 36), PS.BG, profile, beta, radius=6, sat=0.9)
    assert r["status"] == 6 and 0.3 < r["roundness"] < 0.5 and abs(r["angle"]) < 5
    r = PR.fit_star(fr, _at(cand, 55, 36), PS.BG, profile, beta, radius=6, sat=0.9, roundness_min=0.3)
    assert r["status"] == 0
    # a plain star is accepted; a saturated sample is left out of the fit
    p = _at(cand, 41, 13)
    r = PR.fit_star(fr, p, PS.BG, profile, beta, radius=6, sat=0.9)
    assert r["status"] == 0 and abs(r["x"] - 40.7) < 0.02 and abs(r["y"] - 13.2) < 0.02
    r2 = PR.fit_star(fr, p, PS.BG, profile, beta, radius=6, sat=0.2)
    assert 0 < r2["nused"] < r["nused"]
    # too few samples left: nothing is fitted
    assert PR.fit_star(fr, p, PS.BG, profile, beta, radius=6, sat=PS.BG - 1.0)["status"] == 3
    with pytest.raises(ValueError):
        PR.fit_star(fr[:16], p, PS.BG, profile, beta, radius=6)           # the box leaves the frame

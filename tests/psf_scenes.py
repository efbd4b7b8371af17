"""Scenes of the PSF-fit tests (no test in here): the 97 x 53 two-frame scene
of the star-finder test (the same recipe, restated), the one-star 120 x 80
frame, the three 256 x 192 registration frames, and seeded planted stars with
their find_stars-style records."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as PR  # noqa: E402
import star_ref as SR  # noqa: E402

BG, NOISE = 0.05, 0.002
ADU = 60000.0
SCENE = dict(radius=6, sat=0.9)           # finder parameters of the 97 x 53 scene
NAN_AT = (24, 19)                         # inside the box of the star at (20, 15)


def gauss(img, cx, cy, amp, sx=1.5, sy=None):
    sy = sx if sy is None else sy
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    img += amp * np.exp(-((xx - cx) ** 2 / (2 * sx * sx) + (yy - cy) ** 2 / (2 * sy * sy)))


def scene_97x53(dtype, seed=3):
    out = []
    w, h = 97, 53
    for f in range(2):
        rng = np.random.default_rng(seed + f)
        img = BG + rng.normal(0, NOISE, (h, w))
        k = 1.0 - 0.2 * f
        gauss(img, 20.3, 14.6, 0.5 * k)
        gauss(img, 40.7, 13.2, 0.3 * k)
        gauss(img, 64.1, 16.1, 0.4 * k)
        gauss(img, 62.9, 26.2, 0.4 * k)
        gauss(img, 20.1, 34.0, 0.5 * k)
        gauss(img, 24.0, 36.2, 0.3 * k)
        gauss(img, 55.0, 36.0, 0.5 * k, 2.5, 1.0)        # 2.5 : 1 elongated
        gauss(img, 4.2, 25.0, 0.5 * k)
        gauss(img, 80.2, 38.3, 0.2 * k)
        img[22, 34] += 0.5
        img[29:32, 44:47] = 1.0
        if dtype == np.uint16:
            out.append(np.clip(np.rint(img * ADU), 0, 65535).astype(np.uint16))
        else:
            a = img.astype(np.float32)
            if f == 0:
                a[NAN_AT[1], NAN_AT[0]] = np.nan
            out.append(a)
    return np.stack(out)


def units(dtype, prm):
    """(bg, noise, params) in the sample units of dtype."""
    prm = dict(prm)
    if dtype == np.uint16:
        if "sat" in prm:
            prm["sat"] = prm["sat"] * ADU
        return BG * ADU, NOISE * ADU, prm
    return BG, NOISE, prm


def scene_one_star(dtype, seed=9):
    """120 x 80, one sigma = 3 star: at radius 16 its box is 33 x 33."""
    img = BG + np.random.default_rng(seed).normal(0, NOISE, (80, 120))
    gauss(img, 60.3, 40.4, 0.5, 3.0)
    if dtype == np.uint16:
        return np.clip(np.rint(img * ADU), 0, 65535).astype(np.uint16)[None]
    return img.astype(np.float32)[None]


# ---- registration frames (recipe of the star registration test, seed 1) ------
RW, RH, RN = 256, 192, 3
RSEED = 1


def register_truth():
    W, H = RW, RH
    cx, cy = (W - 1) / 2, (H - 1) / 2
    c, s = np.cos(np.deg2rad(1.5)), np.sin(np.deg2rad(1.5))
    R = np.array([[c, -s, cx - c * cx + s * cy + 2.3], [s, c, cy - s * cx - c * cy - 1.6], [0, 0, 1.0]])
    c, s = np.cos(np.deg2rad(-1.0)), np.sin(np.deg2rad(-1.0))
    P = np.array([[c, -s, cx - c * cx + s * cy - 1.7], [s, c, cy - s * cx - c * cy + 2.4], [2e-5, -1.5e-5, 1.0]])
    return [np.eye(3), R, P]


def register_scene():
    """(frames float32 [3, 192, 256], truth Hs)."""
    W, H = RW, RH
    rng = np.random.default_rng(RSEED)
    pts = []
    while len(pts) < 30:
        p = rng.uniform([24, 24], [W - 24, H - 24])
        if all(np.hypot(*(p - q)) >= 14 for q in pts):
            pts.append(p)
    ref_td = np.array(pts)
    amps = rng.uniform(0.1, 0.6, 30)
    Hs = register_truth()
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for f in range(RN):
        td = SR.apply_H(np.linalg.inv(Hs[f]), ref_td)
        img = BG + np.random.default_rng(RSEED + 100 + f).normal(0, NOISE, (H, W))
        for (x, y), a in zip(td, amps):
            img += a * np.exp(-((xx - x) ** 2 + (yy - ((H - 1) - y)) ** 2) / (2 * 1.5 ** 2))
        frames.append(img.astype(np.float32))
    frames = np.stack(frames)
    frames.setflags(write=False)
    return frames, Hs


# ---- planted stars -----------------------------------------------------------
def planted(profile, n, seed, S=41, noise=NOISE, dtype=np.float32, beta=2.5):
    """n seeded stars, each on its own S x S frame: sigma 0.8-3 px (the
    geometric mean of the axes; a Moffat has the FWHM of that Gaussian), axis
    ratio 0.4-1 at a random angle, amplitude 0.05-0.5 over BG.  The box
    half-size b is drawn from 3-16, but not below twice the major sigma: the
    finder's extents follow a star down to the threshold (about 2.5 sigma at
    the faintest amplitude here), so it never hands over a box that cuts the
    core of the star it found.  Returns dicts with the frame, the moment
    record (star_ref.measure on an extent of b - 2) and the planted truth."""
    rng = np.random.default_rng(seed)
    k = PR.FWHM_K if profile == "gaussian" else PR.moffat_k(beta)
    out = []
    yy, xx = np.mgrid[0:S, 0:S]
    for _ in range(n):
        sig, q, th = rng.uniform(0.8, 3.0), rng.uniform(0.4, 1.0), rng.uniform(-math.pi / 2, math.pi / 2)
        sM, sm = sig / math.sqrt(q), sig * math.sqrt(q)
        b = int(rng.integers(max(3, math.ceil(2 * sM)), 17))
        amp = rng.uniform(0.05, 0.5)
        cx, cy = S // 2 + rng.uniform(-0.5, 0.5), S // 2 + rng.uniform(-0.5, 0.5)
        ct, st = math.cos(th), math.sin(th)
        lM, lm = (k / (PR.FWHM_K * sM)) ** 2, (k / (PR.FWHM_K * sm)) ** 2
        a = lM * ct * ct + lm * st * st
        c = lM * st * st + lm * ct * ct
        bb = (lM - lm) * ct * st
        u, v = xx - cx, yy - cy
        Q = a * u * u + 2 * bb * u * v + c * v * v
        E = np.exp(-Q / 2) if profile == "gaussian" else (1 + Q) ** -beta
        img = BG + amp * E
        if noise:
            img = img + rng.normal(0, noise, (S, S))
        img = img.astype(dtype)
        px, py = int(round(cx)), int(round(cy))
        rec = SR._records([SR.measure(img, px, py, (b - 2,) * 4, BG, NOISE, radius=16, roundness_min=0.0,
                                      min_fwhm=0.0)])[0]
        out.append(dict(img=img, b=b, star=rec, cx=cx, cy=cy, amp=amp, a=a, b_=bb, c=c, beta=beta,
                        fwhm_major=k / math.sqrt(lM), fwhm_minor=k / math.sqrt(lm)))
    return out

"""PSF fit on the GPU (sgpu_fit_stars_device) against the numpy restatement
(tests/psf_ref.py): the 97 x 53 two-frame scene of the star
finder test (float32 and WORD; Gaussian, Moffat with free beta, Moffat with
beta fixed at 3), a frame of planted Moffat stars, boxes of 49 and of 1089
samples, lists of 0, 1 and 5 stars, bit-identical repeats and reorderings,
bad arguments.

Tolerance.  Status must be equal; values are compared within 100 x the
rounding floor of the restatement itself: every case is fitted twice on the
CPU, the second time with the samples summed in reversed order, and the
largest difference over all cases of this module is the floor.  Measured:
2.0e-9 relative (fwhm, amp, bkg, beta, a, b, c) and 2.1e-10 px, both from the
WORD scene at radius 3, where a 7 x 7 box cuts the stars' wings and the fit is
poorly conditioned; the other cases stay below 3e-13 and 4e-15 px (a position
x = px + x0 is rounded to ulp(x) <= 2^-46 = 1.4e-14 px for x < 128, which is
the least the position floor can be).  Hence 2.0e-7 relative and 2.1e-8 px,
capped at 1e-6 either way: four orders below the fit's own error, so a wrong
derivative or a dropped sample cannot hide.  The device's exp / pow / log
differ from numpy's by an ulp, which is what the factor 100 is
for.  `iterations` may differ by one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as PR  # noqa: E402
import psf_scenes as PS  # noqa: E402
import star_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint16]
BAD_ARGUMENT = -21
FITS = [("gaussian", None), ("moffat", None), ("moffat", 3.0)]
POS_QUANTUM = 2.0 ** -46
CAP = 1e-6
REL_FIELDS = ("fwhm_major", "fwhm_minor", "amp", "bkg", "beta", "a", "c")


def _moffat_scene():
    """97 x 53, five Moffat stars (beta 2.5, one of them 1.6 : 1): the free-beta fit converges on these."""
    img = PS.BG + np.random.default_rng(17).normal(0, PS.NOISE, (53, 97))
    yy, xx = np.mgrid[0:53, 0:97]
    for cx, cy, amp, w, q in ((20.3, 15.6, 0.5, 1.6, 1.0), (45.7, 14.2, 0.3, 2.0, 1.0), (70.1, 17.1, 0.4, 1.3, 1.0),
                              (30.9, 36.2, 0.4, 2.4, 1.6), (62.2, 35.3, 0.2, 1.8, 1.0)):
        img += amp * (1 + ((xx - cx) / (w * q)) ** 2 + ((yy - cy) / w) ** 2) ** -2.5
    return img.astype(np.float32)[None]


def _inputs():
    """name -> (frames, bg, star lists per frame, fit parameters); computed once."""
    out = {}
    for dt in DTYPES:
        fr = PS.scene_97x53(dt)
        bg, noise, prm = PS.units(dt, PS.SCENE)
        lists = []
        for f in range(2):
            cand = SR.find_stars(fr[f], bg, noise, **prm)[1]
            lists.append(cand[(cand["reject"] == 0) | (cand["reject"] == 6)])      # the 2.5 : 1 star included
        out["scene-" + np.dtype(dt).name] = (fr, bg, lists, dict(radius=6, sat=prm["sat"]))
        out["r3-" + np.dtype(dt).name] = (fr, bg, lists, dict(radius=3, sat=prm["sat"]))
        one = PS.scene_one_star(dt)
        bg1, noise1, _ = PS.units(dt, {})
        star = SR.find_stars(one[0], bg1, noise1, radius=16)[0]
        assert len(star) == 1
        star["ext"] = 14                                   # the walks stop near 10 px; 14 + 2 makes the box 33 x 33
        out["r16-" + np.dtype(dt).name] = (one, bg1, [star], dict(radius=16))
    mf = _moffat_scene()
    out["moffat-planted"] = (mf, PS.BG, [SR.find_stars(mf[0], PS.BG, PS.NOISE, radius=8)[0]], dict(radius=8))
    return out


_cache = {}


def _case(name, profile, beta):
    """(inputs, restatement forward, restatement with reversed sums)."""
    if "inputs" not in _cache:
        _cache["inputs"] = _inputs()
    key = (name, profile, beta)
    if key not in _cache:
        fr, bg, lists, prm = _cache["inputs"][name]
        _cache[key] = tuple([PR.fit_stars(fr[f], lists[f], bg, profile, beta, reverse=rev, **prm)
                             for f in range(len(fr))] for rev in (False, True))
    return _cache["inputs"][name], _cache[key][0], _cache[key][1]


NAMES = ["scene-float32", "scene-uint16", "r3-float32", "r3-uint16", "r16-float32", "r16-uint16", "moffat-planted"]
CASES = [(n, p, b) for n in NAMES for p, b in FITS]


def _diffs(a, b):
    """(largest position difference, largest relative difference) of two PSF arrays."""
    if not len(a):
        return 0.0, 0.0
    pos = max(np.abs(a["x"] - b["x"]).max(), np.abs(a["y"] - b["y"]).max())
    rel = 0.0
    for k in REL_FIELDS:
        m = a[k] != 0
        if m.any():
            rel = max(rel, float((np.abs(a[k] - b[k])[m] / np.abs(a[k][m])).max()))
    rel = max(rel, float((np.abs(a["b"] - b["b"]) / np.sqrt(np.abs(a["a"] * a["c"]))).max()))
    return float(pos), rel


@pytest.fixture(scope="module")
def tolerance():
    """(px, relative): 100 x the restatement's own rounding floor over every case of the module."""
    pos = rel = 0.0
    for name, profile, beta in CASES:
        _, fwd, rev = _case(name, profile, beta)
        for a, b in zip(fwd, rev):
            assert np.array_equal(a["status"], b["status"])
            d = _diffs(a, b)
            pos, rel = max(pos, d[0]), max(rel, d[1])
    print(f"restatement floor: {pos:.3g} px, {rel:.3g} relative")
    assert rel > 0
    return min(100 * max(pos, POS_QUANTUM), CAP), min(100 * rel, CAP)


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _gpu(fr):
    import torch
    fr = np.ascontiguousarray(fr).copy()
    return torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()


def _fit(ctx, name, profile, beta, lists=None, d=None, **over):
    from siril_amd import registration as Rg
    fr, bg, own, prm = _case(name, profile, beta)[0]
    d = _gpu(fr) if d is None else d
    return Rg.fit_stars(d, own if lists is None else lists, ctx=ctx, bg=bg, profile=profile, beta=beta,
                        **dict(prm, **over))


def _close(got, want, tol):
    assert got.dtype == want.dtype and len(got) == len(want)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["nused"], want["nused"])
    dit = np.abs(got["iterations"] - want["iterations"])
    assert (dit <= 1).all(), f"iterations differ by {dit.max()}"
    pos, rel = _diffs(want, got)
    print(f"  vs restatement: {pos:.3g} px, {rel:.3g} relative, iterations differ by {dit.max() if len(dit) else 0}")
    assert pos <= tol[0] and rel <= tol[1], (pos, rel, tol)
    m = want["roundness"] < 0.9                          # the axis of a round star has no direction
    assert np.allclose(got["angle"][m], want["angle"][m], rtol=0, atol=1e-6)
    assert np.allclose(got["rmse"], want["rmse"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,profile,beta", CASES)
def test_fit_matches_the_restatement(ctx, tolerance, name, profile, beta):
    (fr, _, lists, prm), want, _ = _case(name, profile, beta)
    got = _fit(ctx, name, profile, beta)
    assert len(got) == len(fr)
    for f in range(len(fr)):
        _close(got[f], want[f], tolerance)
    st = np.concatenate([w["status"] for w in want])
    nu = np.concatenate([w["nused"] for w in want])
    if name.startswith("scene") and (profile, beta) != ("moffat", None):
        assert (st == 0).sum() >= 10 and (st == 6).sum() == 2          # plain stars, and the 2.5 : 1 star twice
        assert ((st == 3).sum() == 1) == (name == "scene-float32")      # the NaN in a box (float frames only)
    if name.startswith("r3"):
        assert (nu[st != 3] == 49).all()                               # 49 samples: lanes 49..63 idle
    if name.startswith("r16"):
        assert list(nu) == [1089]                                      # 18 samples in lane 0, 17 in the others
        assert abs(want[0]["x"][0] - 60.3) < 0.02 and abs(want[0]["y"][0] - 40.4) < 0.02
        if profile == "gaussian":                                      # the planted star is a Gaussian
            assert list(st) == [0] and abs(want[0]["fwhm_major"][0] / (3.0 * PR.FWHM_K) - 1) < 0.02
    if name == "moffat-planted":
        assert len(st) == 5 and (st == 0).all()                        # also with beta free
        if beta is None and profile == "moffat":
            assert np.all(np.abs(want[0]["beta"] - 2.5) < 0.3) and want[0]["iterations"].max() < 50


@pytest.mark.parametrize("count", [0, 1, 5])
@pytest.mark.parametrize("profile,beta", FITS)
def test_short_lists(ctx, tolerance, count, profile, beta):
    """0, 1 and 5 stars in the first frame, none in the second; the record of
    a star is what it is in the full list, bit for bit."""
    (fr, _, lists, _), want, _ = _case("scene-uint16", profile, beta)
    full = _fit(ctx, "scene-uint16", profile, beta)
    empty = lists[1][:0]
    got = _fit(ctx, "scene-uint16", profile, beta, lists=[lists[0][:count], empty])
    assert len(got[0]) == count and len(got[1]) == 0
    assert got[0].tobytes() == full[0][:count].tobytes()
    _close(got[0], want[0][:count], tolerance)
    got = _fit(ctx, "scene-uint16", profile, beta, lists=[empty, lists[1][:count]])
    assert len(got[0]) == 0 and got[1].tobytes() == full[1][:count].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("profile,beta", FITS)
def test_repeatable_and_independent_of_the_list_order(ctx, dtype, profile, beta):
    name = "scene-" + np.dtype(dtype).name
    fr, _, lists, _ = _case(name, profile, beta)[0]
    d = _gpu(fr)
    a = _fit(ctx, name, profile, beta, d=d)
    b = _fit(ctx, name, profile, beta, d=d)
    r = _fit(ctx, name, profile, beta, d=d, lists=[s[::-1].copy() for s in lists])
    for f in range(2):
        assert len(a[f]) >= 7 and a[f].tobytes() == b[f].tobytes()
        assert r[f][::-1].tobytes() == a[f].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_window(ctx, dtype):
    """A window of larger frames (row and frame strides) equals its contiguous copy."""
    name = "scene-" + np.dtype(dtype).name
    fr = _case(name, "gaussian", None)[0][0]
    big = np.zeros((2, 53 + 9, 97 + 14), fr.dtype)
    big[:] = 7
    big[:, 4:57, 6:103] = fr
    win = _gpu(big)[:, 4:57, 6:103]
    assert not win.is_contiguous()
    a = _fit(ctx, name, "gaussian", None, d=win)
    b = _fit(ctx, name, "gaussian", None, d=win.contiguous())
    for f in range(2):
        assert a[f].tobytes() == b[f].tobytes() and (a[f]["status"] == 0).any()


def test_bad_arguments(ctx):
    from siril_amd import registration as Rg
    from siril_amd._lib import SgpuError
    fr, bg, lists, prm = _case("scene-float32", "gaussian", None)[0]
    d = _gpu(fr)
    outside = [lists[0][:1].copy(), lists[1][:0]]
    outside[0]["px"] = 3                                   # the box (b >= 3) leaves the frame on the left
    for kw, stars in ((dict(profile=7), lists), (dict(radius=0), lists), (dict(radius=17), lists),
                      (dict(max_iter=0), lists), (dict(profile="moffat", beta=11.0), lists),
                      (dict(roundness_min=2.0), lists), (dict(), outside)):
        with pytest.raises(SgpuError) as e:
            Rg.fit_stars(d, stars, ctx=ctx, bg=bg, **dict(dict(radius=6), **kw))
        assert e.value.code == BAD_ARGUMENT, kw
    with pytest.raises(ValueError):
        Rg.fit_stars(d, lists, ctx=ctx, bg=bg, profile="lorentzian")
    with pytest.raises(TypeError):
        Rg.fit_stars(d, lists, ctx=ctx, bg=bg, ksigma=1.0)
    assert Rg.psf_last_kernel_ms(ctx) >= 0.0
    assert Rg.PSF_DTYPE == PR.PSF_DTYPE and Rg.PSF_DTYPE.itemsize == 120

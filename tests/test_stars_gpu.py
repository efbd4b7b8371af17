"""Star finder on the GPU (sgpu_find_stars_device): candidates, extents and
every field of every accepted star bit for bit against the numpy restatement
(tests/star_ref.py), float32 and WORD frames, N = 2, fixed bg / noise.

Shapes (width x height): 97x53 (tiles that do not divide, two tile columns,
four tile rows), 40x30 (at r = 10, K = 3 an interior of 14 x 4 pixels) and
20x20 (no interior: zero stars, no error)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import star_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint16]
BAD_ARGUMENT = -21
BG, NOISE = 0.05, 0.002
ADU = 60000.0
SCENE = dict(radius=6, sat=0.9)           # the planted scene's parameters (K = 3: margin 9)
NAN_AT = (24, 19)                         # inside star A's box, more than K from its peak row and column


def _gauss(img, cx, cy, amp, sx=1.5, sy=None):
    sy = sx if sy is None else sy
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    img += amp * np.exp(-((xx - cx) ** 2 / (2 * sx * sx) + (yy - cy) ** 2 / (2 * sy * sy)))


def _scene(w, h, dtype, seed=3):
    """Two frames; the planted cases of frame 0 are asserted on the restatement."""
    out = []
    for f in range(2):
        rng = np.random.default_rng(seed + f)
        img = BG + rng.normal(0, NOISE, (h, w))
        k = 1.0 - 0.2 * f
        if (w, h) == (97, 53):
            _gauss(img, 20.3, 14.6, 0.5 * k)                 # A: plain star, peak (20, 15)
            _gauss(img, 40.7, 13.2, 0.3 * k)                 # B: plain star
            _gauss(img, 64.1, 16.1, 0.4 * k)                 # tile corner: pixel (64, 16) opens tile (1, 1)
            _gauss(img, 62.9, 26.2, 0.4 * k)                 # tile edge: column 63 closes tile column 0
            _gauss(img, 20.1, 34.0, 0.5 * k)                 # two stars closer than r: one candidate
            _gauss(img, 24.0, 36.2, 0.3 * k)
            _gauss(img, 55.0, 36.0, 0.5 * k, 2.5, 1.0)       # 2.5 : 1 elongated: roundness
            _gauss(img, 4.2, 25.0, 0.5 * k)                  # inside the border margin: never a candidate
            _gauss(img, 80.2, 38.3, 0.2 * k)
            img[22, 34] += 0.5                               # lone hot pixel: zero variance
            img[29:32, 44:47] = 1.0                          # 3 x 3 flat top, saturated (after the noise: exact ties)
        elif (w, h) == (40, 30):
            _gauss(img, 20.2, 14.8, 0.5 * k)
        else:
            _gauss(img, w / 2, h / 2, 0.5 * k)
        if dtype == np.uint16:
            out.append(np.clip(np.rint(img * ADU), 0, 65535).astype(np.uint16))
        else:
            a = img.astype(np.float32)
            if (w, h) == (97, 53) and f == 0:
                a[NAN_AT[1], NAN_AT[0]] = np.nan
            out.append(a)
    return np.stack(out)


def _units(dtype, prm):
    """(bg, noise, params) in the sample units of dtype."""
    prm = dict(prm)
    if dtype == np.uint16:
        if "sat" in prm:
            prm["sat"] = prm["sat"] * ADU
        return BG * ADU, NOISE * ADU, prm
    return BG, NOISE, prm


_frames, _refs = {}, {}


def _get_frames(w, h, dtype):
    key = (w, h, np.dtype(dtype).name)
    if key not in _frames:
        _frames[key] = _scene(w, h, dtype)
        _frames[key].setflags(write=False)
    return _frames[key]


def _ref(w, h, dtype, prm):
    """Restatement of both frames, computed once per (shape, type, parameters)."""
    key = (w, h, np.dtype(dtype).name, tuple(sorted(prm.items())))
    if key not in _refs:
        bg, noise, p = _units(dtype, prm)
        _refs[key] = [SR.find_stars(fr, bg, noise, **p) for fr in _get_frames(w, h, dtype)]
    return _refs[key]


def _gpu(fr):
    import torch
    fr = fr.copy()                                 # the cached scenes are read-only
    return torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _same(a, b, fields=None):
    fields = fields or a.dtype.names
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in fields)


def _compare(got_stars, got_details, ref, f):
    stars, cand = ref
    g = got_details["candidates"][f]
    assert int(got_details["ncandidates"][f]) == len(cand) == len(g)
    always = ("px", "py", "ext", "reject", "amp")
    assert _same(g, cand, always), "candidates / extents / reject codes"
    m3 = cand["reject"] == 3
    assert _same(g[m3], cand[m3], ("flux", "npix"))
    full = (cand["reject"] == 0) | (cand["reject"] >= 4)
    assert _same(g[full], cand[full]), "measured fields"
    assert len(got_stars[f]) == len(stars)
    assert got_stars[f].tobytes() == stars.tobytes(), "accepted stars, order included"


def _run(ctx, w, h, dtype, prm, d=None):
    from siril_amd import registration as Rg
    bg, noise, p = _units(dtype, prm)
    d = _gpu(_get_frames(w, h, dtype)) if d is None else d
    det = {}
    stars = Rg.find_stars(d, ctx=ctx, bg=bg, noise=noise, details=det, **p)
    return stars, det


def _at(cand, x, y):
    m = (cand["px"] == x) & (cand["py"] == y)
    return cand[m][0] if m.any() else None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sigma", [1.0, 0.0])
def test_planted_cases_end_as_described(dtype, sigma):
    """On the restatement alone (frame 0 of the 97x53 scene): without this
    the bit-exact comparison below could pass vacuously."""
    prm = dict(SCENE, smooth_sigma=sigma)
    stars, cand = _ref(97, 53, dtype, prm)[0]
    r, P = prm["radius"], prm["radius"] + int(math.ceil(3 * sigma))
    inbox = lambda x0, x1, y0, y1: cand[(cand["px"] >= x0) & (cand["px"] <= x1) & (cand["py"] >= y0) & (cand["py"] <= y1)]
    # plain stars are accepted, centroids within 0.1 px of where they were planted
    for cx, cy in ((40.7, 13.2), (64.1, 16.1), (62.9, 26.2), (80.2, 38.3)):
        c = _at(cand, int(round(cx)), int(round(cy)))
        assert c is not None and c["reject"] == 0, (cx, cy)
        assert abs(c["x"] - cx) < 0.1 and abs(c["y"] - cy) < 0.1
    assert _at(cand, 64, 16) is not None and _at(cand, 63, 26) is not None     # tile corner, tile edge
    # the hot pixel: a candidate when smoothing lets it through, rejected for zero variance
    hot = _at(cand, 34, 22)
    assert hot is not None and hot["reject"] == 3 and hot["npix"] == 1
    # flat top: exactly one candidate, saturated; with no smoothing the first pixel in raster order
    flat = inbox(44, 46, 29, 31)
    assert len(flat) == 1 and flat[0]["reject"] == 2
    assert (flat[0]["px"], flat[0]["py"]) == ((44, 29) if sigma == 0.0 else (45, 30))
    # two stars closer than r: only the brighter is a candidate (no other within r of it)
    close = inbox(20 - r, 20 + r, 34 - r, 34 + r)
    assert len(close) == 1 and (close[0]["px"], close[0]["py"]) == (20, 34)
    # elongated: rejected by roundness
    el = _at(cand, 55, 36)
    assert el is not None and el["reject"] == 6 and el["roundness"] < 0.5
    # the star in the border margin is never a candidate; every candidate is interior
    assert len(inbox(0, P - 1, 0, 52)) == 0
    assert cand["px"].min() >= P and cand["px"].max() < 97 - P and cand["py"].min() >= P and cand["py"].max() < 53 - P
    # star A: accepted; in the float frame the NaN lies inside its box and is skipped
    a = _at(cand, 20, 15)
    assert a is not None and a["reject"] == 0
    if dtype == np.float32:
        assert a["ext"][1] >= NAN_AT[0] - 20 and a["ext"][3] >= NAN_AT[1] - 15
        assert np.isnan(_get_frames(97, 53, dtype)[0, NAN_AT[1], NAN_AT[0]])
    assert len(stars) >= 5 and np.all(np.diff(stars["flux"]) <= 0)


CASES = [((97, 53), dict(SCENE)), ((97, 53), dict(SCENE, smooth_sigma=0.0)), ((97, 53), dict()),
         ((40, 30), dict()), ((20, 20), dict()),
         # parameter edges
         ((97, 53), dict(radius=1, sat=0.9)), ((97, 53), dict(radius=16)), ((97, 53), dict(SCENE, smooth_sigma=2.0)),
         ((97, 53), dict(radius=1, smooth_sigma=0.0, ksigma=3.0)), ((97, 53), dict(SCENE, max_stars=3)),
         # more candidates than the first record list holds: it is grown and the measurement run again
         ((97, 53), dict(radius=1, smooth_sigma=0.0, max_stars=3))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,prm", CASES)
def test_find_stars_bit_exact(ctx, shape, prm, dtype):
    w, h = shape
    stars, det = _run(ctx, w, h, dtype, prm)
    ref = _ref(w, h, dtype, prm)
    for f in range(2):
        _compare(stars, det, ref[f], f)
    if shape == (20, 20):
        assert all(len(s) == 0 for s in stars) and not det["ncandidates"].any()
    elif shape == (40, 30):
        assert all(len(s) == 1 for s in stars)                    # the 14 x 4 interior holds the planted star
    else:
        assert all(len(c) > 0 for c in det["candidates"])
    if "max_stars" in prm:
        full = _ref(w, h, dtype, {k: v for k, v in prm.items() if k != "max_stars"})
        for f in range(2):
            assert len(full[f][0]) > prm["max_stars"] == len(stars[f])     # cut after the sort
            assert stars[f].tobytes() == full[f][0][:prm["max_stars"]].tobytes()


def test_find_stars_bad_arguments(ctx):
    from siril_amd import registration as Rg
    from siril_amd._lib import SgpuError
    d = _gpu(_get_frames(40, 30, np.float32))
    for bad in (dict(radius=0), dict(radius=17), dict(smooth_sigma=-0.1), dict(smooth_sigma=2.5),
                dict(smooth_sigma=math.nan), dict(max_stars=0), dict(cut=1.5), dict(roundness_min=-1.0)):
        with pytest.raises(SgpuError) as e:
            Rg.find_stars(d, ctx=ctx, bg=BG, noise=NOISE, **bad)
        assert e.value.code == BAD_ARGUMENT, bad
    with pytest.raises(SgpuError) as e:
        Rg.find_stars(d, ctx=ctx, bg=BG, noise=-1.0)
    assert e.value.code == BAD_ARGUMENT


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_stars_strided_window(ctx, dtype):
    """A window of larger frames (row and frame strides) equals its contiguous copy."""
    import torch
    fr = _get_frames(97, 53, dtype)
    big = np.zeros((2, 53 + 9, 97 + 14), fr.dtype)
    big[:] = 7                                     # samples around the window must not be read as part of it
    big[:, 4:57, 6:103] = fr
    win = _gpu(big)[:, 4:57, 6:103]
    assert not win.is_contiguous()
    a, da = _run(ctx, 97, 53, dtype, SCENE, d=win)
    b, db = _run(ctx, 97, 53, dtype, SCENE, d=win.contiguous())
    for f in range(2):
        assert a[f].tobytes() == b[f].tobytes() and len(a[f]) > 0
        assert da["candidates"][f].tobytes() == db["candidates"][f].tobytes()
        _compare(a, da, _ref(97, 53, dtype, SCENE)[f], f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_stars_deterministic(ctx, dtype):
    d = _gpu(_get_frames(97, 53, dtype))
    prm = dict(radius=1, smooth_sigma=0.0)         # the most candidates: every tile appends many
    a, da = _run(ctx, 97, 53, dtype, prm, d=d)
    b, db = _run(ctx, 97, 53, dtype, prm, d=d)
    for f in range(2):
        assert a[f].tobytes() == b[f].tobytes() and len(a[f]) > 0
        assert da["candidates"][f].tobytes() == db["candidates"][f].tobytes()
    assert np.array_equal(da["ncandidates"], db["ncandidates"])


def test_default_background_and_smooth_table(ctx):
    """bg / noise default to the frame median and bgnoise; the smoothing
    table is the restatement's."""
    from siril_amd import registration as Rg
    for sigma in (0.0, 0.5, 1.0, 1.7, 2.0):
        assert Rg.star_smooth_table(sigma).tobytes() == SR.smooth_table(sigma).tobytes()
    fr = _get_frames(97, 53, np.uint16)
    d = _gpu(fr)
    bg, noise = Rg.frame_background(d, ctx)
    assert np.allclose(bg, [np.median(f) for f in fr], atol=1.0) and np.all(noise > 0)
    stars = Rg.find_stars(d, ctx=ctx, radius=6)
    for f in range(2):
        want, _ = SR.find_stars(fr[f], bg[f], noise[f], radius=6)
        assert stars[f].tobytes() == want.tobytes() and len(want) >= 5

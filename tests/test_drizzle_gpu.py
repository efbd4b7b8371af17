"""Drizzle on the GPU (sgpu_drizzle_frames_device): every pixel of the image and
of the weight plane bit-exact against the sequential scatter restated from
DESIGN.md 6h (tests/drizzle_ref.py), for float32 and WORD frames, no pixel
left out, and staged + direct tiles == the tile count.

The kernel's output tile is 22 x 11.  A 45 x 23 input gives outputs of 90 x 46
(scale 2), 68 x 35 (1.5), 45 x 23 (1) and 23 x 12 (0.5): each spans at least
two tiles each way and divides by neither tile side.  N = 3 frames, each with
its own homography; the float32 and the WORD frames of a case share one pass
of the restatement (the weights depend on the maps only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_ref as DR  # noqa: E402
from warp_ref import rotation_H, translation_H  # noqa: E402

pytestmark = pytest.mark.gpu

TW, TH = 22, 11
BAD_ARGUMENT = -21
SCALES = [2.0, 1.5, 1.0, 0.5]
PIXFRACS = [1.0, 0.7, 0.5]
KERNELS = ["square", "turbo", "point"]
PERSPECTIVE = np.array([[1.01, 0.02, -1.2], [-0.015, 0.99, 0.8], [2e-4, -1e-4, 1.0]])


def _mirror_H(w):
    return np.array([[-1.0, 0, w - 1.25], [0, 1, 0.5], [0, 0, 1]])


def _mapset(name, w, h):
    if name == "shift":       # identity; a quarter pixel (holes at scale 2, pixfrac 0.5); another sub-pixel shift
        return np.stack([np.eye(3), translation_H(0.25, 0.25), translation_H(-1.4, 0.7)])
    if name == "warp":        # 1.5 degree rotation plus shift; perspective; mirror (jaco < 0)
        return np.stack([rotation_H(w, h, 1.5, 0.8, -0.6), PERSPECTIVE, _mirror_H(w)])
    if name == "outside":     # frame 1 maps wholly outside the output
        return np.stack([np.eye(3), translation_H(500.0, 300.0), rotation_H(w, h, 1.5, 0.8, -0.6)])
    raise KeyError(name)


def _frames(w, h, n=3, seed=3):
    rng = np.random.default_rng(seed + w + 7 * h)
    f = (rng.random((n, h, w)) * 60000).astype(np.float32)
    return f, f.astype(np.uint16)


def _gpu(fr):
    import torch
    return torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()


def _tiles(ow, oh, n=3):
    return n * ((ow + TW - 1) // TW) * ((oh + TH - 1) // TH)


_refs = {}


def _reference(w, h, Hs, key, ref_index, scale, pixfrac, kernel, pw=None, n=3):
    """([float image, WORD image], weights) of the restatement, computed once per case."""
    k = (w, h, key, ref_index, scale, pixfrac, kernel, pw is not None, n)
    if k not in _refs:
        ff, fw = _frames(w, h, n)
        _refs[k] = DR.drizzle_frames([ff, fw], Hs, ref_index, scale, pixfrac, DR.KERNELS[kernel], pw)
    return _refs[k]


def _check(ctx, w, h, Hs, key, ref_index, scale, pixfrac, kernel, pw=None, n=3):
    """Both dtypes of one case against the restatement; returns (images, weights, tiles)."""
    import torch
    from siril_amd import registration as Rg
    (rf, rw), rcnt = _reference(w, h, Hs, key, ref_index, scale, pixfrac, kernel, pw, n)
    ow, oh = DR.output_size(w, h, scale)
    assert Rg.drizzle_output_size(w, h, scale) == (ow, oh)
    dpw = None if pw is None else torch.from_numpy(pw).cuda()
    tiles = None
    for fr, ref in zip(_frames(w, h, n), (rf, rw)):
        img, cnt = Rg.drizzle_frames(_gpu(fr), Hs, ref_index, scale, pixfrac, kernel, pixel_weights=dpw, ctx=ctx)
        tiles = Rg.drizzle_last_tiles(ctx)
        assert sum(tiles) == _tiles(ow, oh, n)
        img, cnt = img.cpu().numpy(), cnt.cpu().numpy()
        assert img.shape == cnt.shape == (n, oh, ow)
        assert np.array_equal(cnt.view(np.uint32), rcnt.view(np.uint32)), \
            ("weights", fr.dtype, int((cnt.view(np.uint32) != rcnt.view(np.uint32)).sum()))
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), \
            ("image", fr.dtype, int((img.view(np.uint32) != ref.view(np.uint32)).sum()))
    return (rf, rw), rcnt, tiles


@pytest.fixture(scope="module")
def ctx():
    from siril_amd import stacking as S
    c = S.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("ref_index", [0, 2])
@pytest.mark.parametrize("mapset", ["shift", "warp", "outside"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("pixfrac", PIXFRACS)
@pytest.mark.parametrize("scale", SCALES)
def test_drizzle_45x23(ctx, scale, pixfrac, kernel, mapset, ref_index):
    """Every scale x pixfrac x kernel x map set x reference index on 45 x 23,
    float32 and WORD."""
    w, h = 45, 23
    (rf, rw), rcnt, tiles = _check(ctx, w, h, _mapset(mapset, w, h), mapset, ref_index, scale, pixfrac, kernel)
    assert rcnt.max() > 0
    if mapset == "outside" and ref_index == 0:
        assert not rcnt[1].any() and not rf[1].any() and not rw[1].any()
    if mapset == "shift" and ref_index == 0 and scale == 2.0 and pixfrac == 0.5 and kernel == "square":
        # the quarter-pixel frame's drops cover every other output pixel exactly: the rest are holes,
        # exactly 0 in both planes (the comparison above holds the GPU to the same)
        holes = rcnt[1] == 0
        assert holes[2:-2, 2:-2].mean() > 0.5
        assert not rf[1][holes].any() and not rw[1][holes].any()
    if scale >= 1.0:
        assert tiles[1] == 0       # an ordinary case stages every tile


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scale,pixfrac", [(2.0, 0.7), (1.0, 1.0), (0.5, 0.5), (1.5, 1.0)])
@pytest.mark.parametrize("shape", [(70, 5), (64, 1)])
def test_drizzle_thin_frames(ctx, shape, scale, pixfrac, kernel):
    """70 x 5 and 64 x 1: the candidate window is clipped on both sides at once."""
    w, h = shape
    _check(ctx, w, h, _mapset("warp", w, h), "warp", 0, scale, pixfrac, kernel)
    _check(ctx, w, h, _mapset("shift", w, h), "shift", 2, scale, pixfrac, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scale,pixfrac", [(2.0, 0.7), (1.0, 1.0)])
def test_drizzle_pixel_weights(ctx, scale, pixfrac, kernel):
    """A pixel-weight plane with exact zeros and values in (0, 2]."""
    w, h = 45, 23
    rng = np.random.default_rng(11)
    pw = rng.uniform(0.01, 2.0, (h, w)).astype(np.float32)
    pw[rng.random((h, w)) < 0.15] = 0.0
    pw[3, 4] = 2.0
    assert (pw == 0).sum() > 50 and pw.max() == 2.0 and pw[pw > 0].min() > 0
    _check(ctx, w, h, _mapset("warp", w, h), "warp", 0, scale, pixfrac, kernel, pw=pw)


@pytest.mark.parametrize("kernel", KERNELS)
def test_drizzle_direct_path(ctx, kernel):
    """Scale 0.25 on 100 x 48 (output 25 x 12): the staged patch holds 608
    input pixels, and the candidate box of a full 22 x 11 tile is about
    (88 + 3) x (44 + 3) of them, that of the 3-pixel-wide tile beside it about
    15 x 47 and that of the 1-pixel-high tile below about 91 x 7: all three take
    the direct path, the 3 x 1 corner tile (15 x 7) is staged."""
    w, h = 100, 48
    _, _, tiles = _check(ctx, w, h, _mapset("warp", w, h), "warp", 0, 0.25, 1.0, kernel)
    assert tiles[1] > 0 and tiles[0] > 0


def test_drizzle_out_planes_overwritten_and_deterministic(ctx):
    """out= / out_weights= pre-filled with NaN are fully overwritten (holes and
    a frame mapped outside included), and two calls give identical bits."""
    import torch
    from siril_amd import registration as Rg
    w, h = 45, 23
    Hs = _mapset("outside", w, h)
    Hs[2] = translation_H(0.25, 0.25)
    d = _gpu(_frames(w, h)[0])
    ow, oh = DR.output_size(w, h, 2.0)
    out = torch.full((3, oh, ow), float("nan"), device="cuda")
    outw = torch.full((3, oh, ow), float("nan"), device="cuda")
    a, b = Rg.drizzle_frames(d, Hs, 0, 2.0, 0.5, "square", out=out, out_weights=outw, ctx=ctx)
    assert a is out and b is outw
    assert not torch.isnan(out).any() and not torch.isnan(outw).any()
    assert not out[1].any() and not outw[1].any() and (outw[2] == 0).any()
    c, e = Rg.drizzle_frames(d, Hs, 0, 2.0, 0.5, "square", ctx=ctx)
    assert torch.equal(c.view(torch.int32), out.view(torch.int32))
    assert torch.equal(e.view(torch.int32), outw.view(torch.int32))


def test_drizzle_refusals(ctx):
    import torch
    from siril_amd import SgpuError
    from siril_amd import registration as Rg
    w, h = 45, 23
    d = _gpu(_frames(w, h)[0])
    Hs = _mapset("shift", w, h)
    for kw in (dict(scale=0.05), dict(scale=4.5), dict(pixfrac=0.0), dict(pixfrac=1.5), dict(kernel=7)):
        with pytest.raises(SgpuError) as e:
            Rg.drizzle_frames(d, Hs, 0, ctx=ctx, **kw)
        assert e.value.code == BAD_ARGUMENT
    with pytest.raises(ValueError):
        Rg.drizzle_frames(d, Hs, 0, kernel="gaussian", ctx=ctx)
    bad = Hs.copy()
    bad[1] = np.array([[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]])     # W vanishes at x = 20
    with pytest.raises(SgpuError) as e:
        Rg.drizzle_frames(d, bad, 0, ctx=ctx)
    assert e.value.code == BAD_ARGUMENT
    bad[1] = 0.0
    with pytest.raises(SgpuError) as e:
        Rg.drizzle_frames(d, bad, 0, ctx=ctx)
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(ValueError):
        Rg.drizzle_frames(d, Hs, 0, out=torch.empty((3, h, w), device="cuda"), scale=2.0, ctx=ctx)
    with pytest.raises(ValueError):
        Rg.drizzle_frames(d, Hs, 0, pixel_weights=torch.ones((w, h), device="cuda"), ctx=ctx)


@pytest.mark.parametrize("rt", [0, 5])
def test_drizzle_then_stack(ctx, oracle, rt):
    """End to end: 8 dithered 45 x 23 frames drizzled at scale 2, pixfrac 0.7,
    then stacked with the weight planes as the stack's drizzle weights, without
    rejection and Winsorized: equal to the oracle's stack of the same planes."""
    from siril_amd import registration as Rg
    from siril_amd import stacking as S
    w, h, n = 45, 23, 8
    rng = np.random.default_rng(21)
    scene = (rng.random((h, w)) * 0.5 + 0.2).astype(np.float32)
    fr = np.stack([scene + rng.normal(0, 0.01, (h, w)).astype(np.float32) for _ in range(n)]).astype(np.float32)
    dith = rng.uniform(-1.5, 1.5, (n, 2))
    dith[0] = 0
    Hs = np.stack([translation_H(dx, dy) for dx, dy in dith])
    img, wts = Rg.drizzle_frames(_gpu(fr), Hs, 0, 2.0, 0.7, "square", ctx=ctx)
    img, wts = img.cpu().numpy(), wts.cpu().numpy()
    assert (wts == 0).any() and (wts > 0).mean() > 0.5
    res = ctx.stack(img, S.StackingArgs(S.Rejection(rt), (3.0, 3.0)), drizzle=wts)
    ref = oracle.stack_rows(img, rt, (3.0, 3.0), nthreads=8, drizz=wts)
    assert np.array_equal(res.result.view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(res.rejmap_low, ref[1]) and np.array_equal(res.rejmap_high, ref[2])

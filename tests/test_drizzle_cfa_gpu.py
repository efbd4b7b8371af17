"""CFA drizzle on the GPU (sgpu_drizzle_cfa_frames_device, drizzle_frames(cfa=)):
every pixel of the three image planes and of the three weight planes bit-exact
against tests/drizzle_cfa_ref.py -- the unchanged mono restatement run once per
colour under the pixel weights w * [colour == c] -- for float32 and WORD frames,
no pixel left out, and against three masked calls of the mono drizzle_frames on
the GPU.

The kernel's output tile is 22 x 11.  A 37 x 29 input gives outputs of 37 x 29
(scale 1) and 74 x 58 (scale 2), a 64 x 40 input one of 26 x 16 at scale 0.4:
each spans at least two tiles each way and divides by neither tile side, and
neither input side is a multiple of 2 and 6 at once (37 and 29 of neither).
Three frames per call, the reference last: a 1.5 degree rotation with a
fractional shift, a mirrored map (jaco < 0) and the identity -- two frames
would leave one map beside the reference's identity.  The float32 and the WORD
frames of a case share one pass of the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_cfa_ref as CR  # noqa: E402
import drizzle_ref as DR  # noqa: E402
from warp_ref import rotation_H  # noqa: E402

pytestmark = pytest.mark.gpu

TW, TH = 22, 11
BAD_ARGUMENT = -21
KERNELS = ["square", "turbo", "point"]
N = 3


def _maps(w, h):
    return np.stack([rotation_H(w, h, 1.5, 0.8, -0.6), np.array([[-1.0, 0, w - 1.25], [0, 1, 0.5], [0, 0, 1]]),
                     np.eye(3)])


def _frames(w, h):
    rng = np.random.default_rng(5 + w + 7 * h)
    f = (rng.random((N, h, w)) * 60000).astype(np.float32)
    return f, f.astype(np.uint16)


def _weights(w, h):
    """A pixel-weight plane with exact zeros and values in (0, 2]."""
    rng = np.random.default_rng(13 + w)
    pw = rng.uniform(0.01, 2.0, (h, w)).astype(np.float32)
    pw[rng.random((h, w)) < 0.15] = 0.0
    pw[3, 4] = 2.0
    assert (pw == 0).sum() > 50 and pw.max() == 2.0
    return pw


def _gpu(fr):
    import torch
    return torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()


def _bits(a):
    return a.view(np.uint32)


_refs = {}


def _reference(w, h, scale, pixfrac, kernel, pattern, use_pw):
    """([float images, WORD images], weights), each [N, 3, oh, ow]: computed once per case, never changed."""
    k = (w, h, scale, pixfrac, kernel, pattern, use_pw)
    if k not in _refs:
        _refs[k] = CR.drizzle_frames_cfa(list(_frames(w, h)), _maps(w, h), N - 1, scale, pixfrac, DR.KERNELS[kernel],
                                         pattern, _weights(w, h) if use_pw else None)
    return _refs[k]


def _check(ctx, w, h, scale, pixfrac, kernel, pattern, use_pw):
    """Both dtypes of one case against the restatement and against three masked
    mono calls on the GPU; returns the tile counters (staged, direct)."""
    import torch
    from siril_amd import registration as Rg
    (rf, rw), rcnt = _reference(w, h, scale, pixfrac, kernel, pattern, use_pw)
    ow, oh = DR.output_size(w, h, scale)
    Hs = _maps(w, h)
    pw = _weights(w, h) if use_pw else None
    dpw = None if pw is None else torch.from_numpy(pw).cuda()
    col = CR.colour_plane(pattern, w, h)
    tiles = None
    for fr, ref in zip(_frames(w, h), (rf, rw)):
        d = _gpu(fr)
        img, cnt = Rg.drizzle_frames(d, Hs, N - 1, scale, pixfrac, kernel, pixel_weights=dpw, ctx=ctx, cfa=pattern)
        tiles = Rg.drizzle_last_tiles(ctx)
        assert sum(tiles) == N * ((ow + TW - 1) // TW) * ((oh + TH - 1) // TH)
        assert tuple(img.shape) == tuple(cnt.shape) == (N, 3, oh, ow)
        himg, hcnt = img.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(_bits(hcnt), _bits(rcnt)), \
            ("weights", fr.dtype, int((_bits(hcnt) != _bits(rcnt)).sum()))
        assert np.array_equal(_bits(himg), _bits(ref)), ("image", fr.dtype, int((_bits(himg) != _bits(ref)).sum()))
        for c in range(3):                                # what a user had to do before: one masked call per colour
            m = (col == c).astype(np.float32)
            mi, mc = Rg.drizzle_frames(d, Hs, N - 1, scale, pixfrac, kernel, ctx=ctx,
                                       pixel_weights=torch.from_numpy(m if pw is None else pw * m).cuda())
            assert torch.equal(mi.view(torch.int32), img[:, c].view(torch.int32)), ("masked image", c)
            assert torch.equal(mc.view(torch.int32), cnt[:, c].view(torch.int32)), ("masked weights", c)
    assert rcnt.max() > 0
    return tiles


@pytest.fixture(scope="module")
def ctx():
    from siril_amd import stacking as S
    c = S.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("pattern,use_pw", [("RGGB", False), ("BGGR", True), ("GBRG", False), ("GRBG", True),
                                            (CR.XTRANS, True)])
def test_cfa_drizzle_every_pattern(ctx, pattern, use_pw, kernel):
    """37 x 29 at scale 1: the four Bayer strings and an X-Trans one."""
    tiles = _check(ctx, 37, 29, 1.0, 1.0, kernel, pattern, use_pw)
    assert tiles[0] > 0 and tiles[1] == 0             # an ordinary case stages every tile


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("pattern,use_pw", [("RGGB", True), (CR.XTRANS, False)])
def test_cfa_drizzle_scale2_pixfrac_half(ctx, pattern, use_pw, kernel):
    """37 x 29 at scale 2, pixfrac 0.5: 74 x 58, drops smaller than an output pixel's footprint."""
    tiles = _check(ctx, 37, 29, 2.0, 0.5, kernel, pattern, use_pw)
    assert tiles[0] > 0 and tiles[1] == 0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("pattern,use_pw", [("GRBG", False), (CR.XTRANS, True)])
def test_cfa_drizzle_direct_path(ctx, pattern, use_pw, kernel):
    """64 x 40 at scale 0.4 (output 26 x 16): the candidate box of a full
    22 x 11 tile is about (55 + 3) x (28 + 3) input pixels, more than the 608
    staged ones, so it takes the direct path (the header's CFA gather); the
    4 x 5 corner tile's box (about 13 x 16) is staged."""
    tiles = _check(ctx, 64, 40, 0.4, 1.0, kernel, pattern, use_pw)
    assert tiles[1] > 0 and tiles[0] > 0


def test_cfa_drizzle_absent_colour(ctx):
    """A pattern without blue: the blue channel is 0 with weight 0 everywhere."""
    from siril_amd import registration as Rg
    w, h = 37, 29
    img, cnt = Rg.drizzle_frames(_gpu(_frames(w, h)[0]), _maps(w, h), N - 1, 1.0, 1.0, "square", ctx=ctx, cfa="RGGR")
    assert not img[:, 2].any() and not cnt[:, 2].any() and cnt[:, 0].any() and cnt[:, 1].any()


@pytest.mark.parametrize("kernel", KERNELS)
def test_cfa_drizzle_strides_through_the_c_entry(ctx, kernel):
    """out_plane_stride and out_frame_stride above their minima, through the
    C entry: the planes land where the strides say, bit-equal to the
    restatement, and every float between and after them keeps its NaN."""
    import torch
    from siril_amd import _lib
    from siril_amd.registration import _cfa_args, _drizzle_params
    w, h, scale, pixfrac, pattern = 37, 29, 2.0, 0.5, "RGGB"
    (rf, _), rcnt = _reference(w, h, scale, pixfrac, kernel, pattern, True)
    ow, oh = DR.output_size(w, h, scale)
    ps, fs = ow * oh + 5, 3 * (ow * oh + 5) + 11
    d = _gpu(_frames(w, h)[0])
    dpw = torch.from_numpy(_weights(w, h)).cuda()
    out = torch.full((N * fs + 7,), float("nan"), device="cuda")
    outw = torch.full((N * fs + 7,), float("nan"), device="cuda")
    pat, dim = _cfa_args(pattern)
    H = np.ascontiguousarray(_maps(w, h).reshape(N, 9))
    p = _drizzle_params(scale, pixfrac, kernel)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def call(plane_stride, frame_stride, pattern_bytes=pat, pattern_dim=dim):
        return _lib.lib().sgpu_drizzle_cfa_frames_device(
            ctx.h, C.c_void_p(d.data_ptr()), 4, N, w, h, h * w, C.c_void_p(dpw.data_ptr()),
            pattern_bytes.ctypes.data_as(C.c_void_p), pattern_dim, H.ctypes.data_as(C.c_void_p), N - 1, C.byref(p),
            C.c_void_p(out.data_ptr()), C.c_void_p(outw.data_ptr()), plane_stride, frame_stride)

    # refused before anything is launched: strides below their minima, a bad pattern
    assert call(ow * oh - 1, fs) == BAD_ARGUMENT
    assert call(ps, 3 * ps - 1) == BAD_ARGUMENT
    assert call(ps, fs, np.array([0, 1, 3, 2], np.uint8)) == BAD_ARGUMENT
    assert call(ps, fs, np.zeros(9, np.uint8), 3) == BAD_ARGUMENT
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(outw).all())
    assert call(ps, fs) == 0
    for got, want in ((out.cpu().numpy(), rf), (outw.cpu().numpy(), rcnt)):
        used = np.zeros(got.size, bool)
        for f in range(N):
            for c in range(3):
                o = f * fs + c * ps
                assert np.array_equal(_bits(got[o:o + ow * oh]), _bits(want[f, c].ravel())), (f, c)
                used[o:o + ow * oh] = True
        assert np.isnan(got[~used]).all() and not np.isnan(got[used]).any()


def test_cfa_drizzle_refusals(ctx):
    import torch
    from siril_amd import SgpuError
    from siril_amd import registration as Rg
    w, h = 37, 29
    d = _gpu(_frames(w, h)[0])
    Hs = _maps(w, h)
    with pytest.raises(SgpuError) as e:                       # an entry of 3
        Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa=np.array([0, 1, 3, 2], np.uint8))
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(SgpuError) as e:                       # a letter that is no colour compiles to 3
        Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGXB")
    assert e.value.code == BAD_ARGUMENT
    with pytest.raises(ValueError):                           # dim = 3
        Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa=np.zeros(9, np.uint8))
    with pytest.raises(ValueError):
        Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGGBR")
    for shape in ((N, h, w), (N, 3, h, w + 1), (N, 1, h, w)):  # wrongly shaped out / out_weights
        with pytest.raises(ValueError):
            Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGGB", out=torch.empty(shape, device="cuda"))
        with pytest.raises(ValueError):
            Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGGB", out_weights=torch.empty(shape, device="cuda"))
    with pytest.raises(ValueError):                           # and the CFA shape is wrong without cfa=
        Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, out=torch.empty((N, 3, h, w), device="cuda"))
    for kw in (dict(scale=0.05), dict(pixfrac=0.0), dict(kernel=7)):   # the mono refusals hold
        with pytest.raises(SgpuError) as e:
            Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGGB", **kw)
        assert e.value.code == BAD_ARGUMENT
    out = torch.full((N, 3, h, w), float("nan"), device="cuda")
    a, b = Rg.drizzle_frames(d, Hs, N - 1, ctx=ctx, cfa="RGGB", out=out)
    assert a is out and not torch.isnan(out).any() and tuple(b.shape) == (N, 3, h, w)

"""Frame warp on the GPU (sgpu_warp_frames_device): every case bit-exact
against the numpy restatement of the specification (tests/warp_ref.py), for
float32 and WORD frames, no pixel left out.

Shapes (width x height): 97x53 (tiles that do not divide, two tile columns,
four tile rows), 70x5 (fewer rows than the 8 Lanczos taps: the reflection
iterates) and 64x1 (len == 1).  N = 3 frames, each with its own homography."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as WR  # noqa: E402
from warp_ref import perspective_H, rotation_H, translation_H  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(97, 53), (70, 5), (64, 1)]
DTYPES = [np.float32, np.uint16]
MODES = [(0, False), (1, False), (3, False), (2, False), (2, True), (4, False), (4, True)]
BAD_ARGUMENT = -21


def _frames(w, h, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((3, h, w)) * 60000).astype(dtype)


def _star_frames(w, h, dtype):
    """Background 1000 with isolated single-pixel stars of 60000."""
    fr = np.full((3, h, w), 1000, dtype)
    for f in range(3):
        for y in range(0, h, 6):
            fr[f, y, 5 + f + (y % 4):w - 4:9] = 60000
    return fr


def _gpu(fr):
    import torch
    return torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()


def _host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


def _tiles(w, h, n=3):
    return n * ((w + 63) // 64) * ((h + 15) // 16)


_tables = {}


def _table(interp):
    from siril_amd import registration as Rg
    if interp not in _tables:
        _tables[interp] = Rg.warp_table(interp)
    return _tables[interp]


def _check(ctx, fr, d, Hs, ref_index, interp, clamp):
    """Run one warp, compare every pixel with the restatement; returns
    (output, dilated clamp masks of the restatement, (staged, direct))."""
    from siril_amd import registration as Rg
    n, h, w = fr.shape
    out = _host(Rg.warp_frames(d, Hs, ref_index, interp, clamp, ctx=ctx), fr.dtype)
    tiles = Rg.warp_last_tiles(ctx)
    assert sum(tiles) == _tiles(w, h, n)
    M = Rg.warp_inverse_maps(Hs, ref_index, h)
    ref, dil = WR.warp_frames(fr, M, interp, _table(interp), _table(1), clamp)
    bits = np.uint32 if fr.dtype == np.float32 else np.uint16
    assert np.array_equal(out.view(bits), ref.view(bits)), (interp, clamp, int((out != ref).sum()))
    return out, dil, tiles


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _case_Hs(case, w, h):
    dy = 0.4 if h <= 5 else -4.1          # keep part of a thin frame inside itself
    if case == "subpixel":                # (0.25, -0.5) relative to the reference frame
        return [translation_H(2.25, 0.5), translation_H(2, 1), translation_H(-1.75, 1.53125)]
    if case == "rotation":
        return [rotation_H(w, h, 1.5, 2.3, dy), translation_H(1, 0), rotation_H(w, h, -1.5, -0.7, dy / 2)]
    if case == "perspective":
        P = perspective_H(w, h)
        P[1, 2] += 1.3 + dy / 4
        return [P, translation_H(0, 0), np.linalg.inv(P)]
    raise KeyError(case)


def _direct_Hs(case, w, h):
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    if case == "rot90_quarter":           # about the centre; the 0.4 keeps a 1-row frame's centre inside
        return [np.array([[0, -0.25, cx + 0.25 * cy + 0.4], [0.25, 0, cy - 0.25 * cx], [0, 0, 1.0]]), np.eye(3),
                np.array([[0, 0.25, cx - 0.25 * cy - 0.4], [-0.25, 0, cy + 0.25 * cx], [0, 0, 1.0]])]
    if case == "w_crosses_zero":          # W = 1 - x / 32: exactly 0 on column 32
        return [np.array([[1, 0, 0], [0, 1, 0], [1 / 32.0, 0, 1.0]]), np.eye(3),
                np.array([[1, 0, 0.5], [0, 1, 0], [1 / 48.0, 1 / 64.0, 1.0]])]
    raise KeyError(case)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_warp_integer_translations_are_shifts(ctx, w, h, dtype):
    """Identity and integer translations, every interpolation, clamp on and
    off: bit-equal to shift_frames with the shifts of apply_reg_shifts."""
    from siril_amd import registration as Rg
    fr = _frames(w, h, dtype, 11)
    d = _gpu(fr)
    Hs = [Rg.set_shifts(0, 0), Rg.set_shifts(3, 0 if h == 1 else -2), Rg.set_shifts(-5, 0 if h == 1 else 1)]
    for ref_index in (0, 2):
        sx, sy = Rg.apply_reg_shifts(Hs, ref_index)
        want = _host(Rg.shift_frames(d, sx, sy, ctx=ctx), dtype)
        assert want.any()
        for interp in range(5):
            for clamp in (False, True):
                out, _, _ = _check(ctx, fr, d, Hs, ref_index, interp, clamp)
                assert np.array_equal(out, want), (interp, clamp)


@pytest.mark.parametrize("case", ["subpixel", "rotation", "perspective"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_warp_resampling(ctx, w, h, dtype, case):
    """Sub-pixel translation, 1.5 degree rotation plus shift, mild
    perspective: every interpolation, clamp on and off where it applies.  The
    rotation's tiles have compact footprints: the staged path must have run."""
    fr = _frames(w, h, dtype, 12)
    d = _gpu(fr)
    Hs = _case_Hs(case, w, h)
    for interp, clamp in MODES:
        out, _, (staged, direct) = _check(ctx, fr, d, Hs, 1, interp, clamp)
        assert out.any()
        if case == "rotation":
            assert staged > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_warp_clamp_not_vacuous(ctx, w, h, dtype):
    """Stars on a flat background make the cubic and Lanczos kernels
    undershoot: the restatement's dilated mask is non-empty, clamp on differs
    from clamp off, both match the restatement."""
    fr = _star_frames(w, h, dtype)
    d = _gpu(fr)
    Hs = _case_Hs("rotation", w, h)
    for interp in (2, 4):
        on, dil, _ = _check(ctx, fr, d, Hs, 1, interp, True)
        off, none, _ = _check(ctx, fr, d, Hs, 1, interp, False)
        assert dil.any() and not none.any()
        assert not np.array_equal(on, off)
        assert np.array_equal(on[~dil], off[~dil])


@pytest.mark.parametrize("case", ["rot90_quarter", "w_crosses_zero"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_warp_direct_path(ctx, w, h, dtype, case):
    """Tiles whose source footprint cannot be staged gather from global
    memory, with the same bits: a 90 degree rotation at scale 0.25 (a 66x18
    tile reads a 72x264 source region) and a perspective whose W crosses zero
    inside the frame (W == 0 exactly on column 32: the w = 0 rule)."""
    fr = _frames(w, h, dtype, 13)
    d = _gpu(fr)
    Hs = _direct_Hs(case, w, h)
    for interp, clamp in MODES:
        out, _, (staged, direct) = _check(ctx, fr, d, Hs, 1, interp, clamp)
        assert direct > 0
        assert out.any()


def test_warp_refusals(ctx):
    """Interpolation 5 (NONE), in place, a singular homography: SGPU_BAD_ARGUMENT."""
    from siril_amd import registration as Rg
    from siril_amd._lib import SgpuError
    fr = _frames(70, 5, np.float32, 14)
    d = _gpu(fr)
    Hs = _case_Hs("subpixel", 70, 5)
    sing = [H.copy() for H in Hs]
    sing[2] = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]])
    for kwargs in (dict(Hs=Hs, interpolation=5), dict(Hs=Hs, interpolation=4, out=d),
                   dict(Hs=sing, interpolation=4)):
        with pytest.raises(SgpuError) as e:
            Rg.warp_frames(d, ref_index=1, ctx=ctx, **kwargs)
        assert e.value.code == BAD_ARGUMENT

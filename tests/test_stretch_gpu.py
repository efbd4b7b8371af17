"""The stretch kernel (siril_amd/csrc/stretch.hip) against the restatement
(tests/stretch_ref.py), bit for bit: NaN at the same places and every other
sample equal as uint32, no tolerance anywhere (NaN payloads are not compared).

A lane handles four consecutive samples and a block 1024, so the shapes are the
smallest at which that goes wrong: 1 x 1 and 3 x 1 (less than one vector), 5 x 7
at N = 2, C = 3 (35 samples per plane: every other plane starts 4 bytes off a
16-byte boundary, so the planes have heads and tails and, read three together,
fall back to single samples), 71 x 97 (odd, several blocks), 64 x 64 (aligned,
an exact multiple) and 1 x 4097 (one past four blocks).  Every scene holds 0 and
1, LP, SP and HP with their float32 neighbours, samples below 0 and above 1, one
NaN in one channel of one pixel, pixels whose channels pass 1 under a luminance
model, a black pixel, and as WORD planes 0 and 65535.  References are computed
once per (scene, parameters) and shared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
# (N, H, W)
SHAPES = ((1, 1, 1), (1, 1, 3), (2, 7, 5), (1, 97, 71), (1, 64, 64), (1, 1, 4097))
LP, SP, HP = 0.02, 0.1, 0.8
BS = (-5.0, -1.5, -1.0, -0.5, 0.0, 0.5, 3.0, 15.0)


def _dev(a):
    import torch
    a = np.array(a)         # a copy: the shared scenes are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _scene(n, c, h, w, word=False):
    """[n, c, h, w] (c = 0: [n, h, w])."""
    nch = max(c, 1)
    rng = np.random.RandomState(100 * h + w + 7 * nch + word)
    x = (rng.rand(n, nch, h * w) ** 3).astype(F)
    edges = [F(v) for v in (LP, SP, HP)]
    special = [F(0), F(1)] + edges + [np.nextafter(e, F(d)) for e in edges for d in (-1, 2)] + [F(-0.25), F(1.5)]
    # one-, two- and three-channel candidates for clipping under a luminance model, and a black pixel
    pixels = [(0.95, 0.02, 0.02), (0.9, 0.85, 0.01), (0.99, 0.98, 0.97), (0.0, 0.0, 0.0), (0.02, 0.9, 0.05)]
    npix = h * w
    for i in range(n):
        for ch in range(nch):
            for k, v in enumerate(special):
                # every plane gets the specials, shifted so that small planes see different ones
                x[i, ch, (k + 3 * ch + i) % npix if npix < 16 else k + ch] = v
        if npix >= 35:
            for k, px in enumerate(pixels):
                x[i, :, 20 + 3 * k] = px[:nch]
    if word:
        x = np.rint(np.clip(x, 0, 1) * 65535.0).astype(np.uint16)
        x[:, :, 0] = 0
        x[:, :, npix - 1] = 65535
    else:
        x[0, min(1, nch - 1), (npix - 1) // 2] = np.nan
    return _readonly(x.reshape((n, nch, h, w) if c else (n, h, w)))


def _key(p):
    return tuple(getattr(p, f) for f in R.Params.__dataclass_fields__)


@functools.lru_cache(maxsize=None)
def _want_cached(n, c, h, w, word, key):
    return _readonly(R.stretch(R.Params(*key), _scene(n, c, h, w, word)))


def _want(n, c, h, w, word, p):
    return _want_cached(n, c, h, w, word, _key(p))


def _blk(p):
    from siril_amd._lib import StretchParams
    return StretchParams(p.function, p.model, p.clipmode, p.mask, p.lo, p.m, p.hi, p.D, p.B, p.LP, p.SP, p.HP, p.beta,
                         p.offset, p.BP)


def _same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.float32 and R.float32_bits_equal(got, want), \
        (int((got.view(np.uint32) != np.asarray(want).view(np.uint32)).sum()), got.size)


def _check(n, c, h, w, word, p):
    from siril_amd import stretch as ST
    got = ST.stretch(_dev(_scene(n, c, h, w, word)), _blk(p)).cpu().numpy()
    want = _want(n, c, h, w, word, p)
    _same(got, want)
    return want


def _ght(fn, D, B=0.0, **kw):
    return R.Params(fn, D=D, B=B, LP=LP, SP=SP, HP=HP, **kw)


def _functions():
    ps = [R.Params(R.MTF, lo=0.02, m=0.2, hi=0.8), R.Params(R.MTF, lo=0.0, m=0.7, hi=1.0),
          R.Params(R.LINEAR, BP=0.1), R.Params(R.ASINH, beta=100.0, offset=0.02), R.Params(R.ASINH, beta=1.0),
          R.Params(R.ASINH, beta=1000.0, model=R.HUMAN), _ght(R.GHT, 0.0, 3.0)]
    for D in (1.0, 10.0):
        ps += [_ght(fn, D, B) for fn in (R.GHT, R.INVGHT) for B in BS]
        ps += [_ght(fn, D) for fn in (R.MODASINH, R.INVMODASINH)]
    ps += [R.Params(R.GHT, D=10.0, B=0.0, LP=0.0, SP=0.0, HP=1.0),       # exp's argument reaches -22 026
           R.Params(R.INVGHT, D=10.0, B=0.0, LP=0.0, SP=0.0, HP=1.0),
           R.Params(R.GHT, D=4.0, B=2.0, LP=0.5, SP=0.5, HP=0.5)]
    return ps


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("c", (0, 3))
def test_every_function_and_regime(shape, c):
    n, h, w = shape
    for p in _functions():
        want = _check(n, c, h, w, False, p)
        finite = want[~np.isnan(want)]
        assert finite.size == 0 or (finite.min() >= 0.0 and finite.max() <= 1.0)
        assert int(np.isnan(want).sum()) == (3 if R.joint(p, max(c, 1)) else 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_word_input(shape):
    n, h, w = shape
    for c in (0, 3):
        for p in (R.Params(R.MTF, lo=0.02, m=0.2, hi=0.8), R.Params(R.LINEAR, BP=0.1), R.Params(R.ASINH, beta=50.0),
                  _ght(R.GHT, 6.0, 3.0), _ght(R.INVGHT, 2.0, -1.5), _ght(R.MODASINH, 5.0, model=R.HUMAN),
                  _ght(R.GHT, 6.0, 3.0, model=R.EVEN, clipmode=R.RESCALE)):
            want = _check(n, c, h, w, True, p)
            assert not np.isnan(want).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_colour_models_and_clip_modes(shape):
    n, h, w = shape
    for model in (R.HUMAN, R.EVEN):
        for mode in (R.CLIP, R.RESCALE, R.RGBBLEND):
            for p in (_ght(R.GHT, 6.0, 3.0, model=model, clipmode=mode), _ght(R.MODASINH, 6.0, model=model, clipmode=mode),
                      _ght(R.INVGHT, 2.0, -1.5, model=model, clipmode=mode)):
                want = _check(n, 3, h, w, False, p)
                assert int(np.isnan(want).sum()) == 3
                if h * w >= 35 and p.function == R.GHT:
                    # the scene's bright pixels pass 1 in one and in two channels before the clip mode acts
                    x = R.clip01(R.widen(_scene(n, 3, h, w)[0].reshape(3, -1)))
                    c, regime = R.coeffs(p)
                    L = R.lum(p, x)
                    with np.errstate(all="ignore"):
                        s = x * np.where(L == 0.0, 0.0, R.T(c, regime, L) / L)[None]
                    over = (s > 1.0).sum(0)
                    assert {1, 2} <= set(over.tolist()) and (L == 0.0).any()


def test_channel_mask_passes_bits_through():
    for n, h, w in SHAPES[2:4]:
        for word in (False, True):
            for p in (_ght(R.GHT, 6.0, 3.0, model=R.HUMAN, mask=5), _ght(R.GHT, 6.0, 3.0, mask=2),
                      R.Params(R.MTF, lo=0.02, m=0.2, hi=0.8, mask=6)):
                want = _check(n, 3, h, w, word, p)
                x = _scene(n, 3, h, w, word)
                for ch in range(3):
                    if not p.mask >> ch & 1:
                        keep = x[:, ch].astype(F) if not word else (x[:, ch].astype(np.float64) / 65535.0).astype(F)
                        assert R.float32_bits_equal(want[:, ch], keep)
                # on one plane the mask is not read
                _check(n, 0, h, w, word, p)


def test_out_given_and_refusals():
    import torch
    from siril_amd import stretch as ST
    n, h, w = SHAPES[2]
    p = _ght(R.GHT, 6.0, 3.0, model=R.HUMAN)
    x = _dev(_scene(n, 3, h, w))
    out = torch.full(x.shape, 7.0, dtype=torch.float32, device=x.device)
    assert ST.stretch(x, _blk(p), out=out) is out
    _same(out.cpu().numpy(), _want(n, 3, h, w, False, p))
    assert ST.ght(x, 6.0, 3.0, LP, SP, HP, model="human", out=out) is out
    _same(out.cpu().numpy(), _want(n, 3, h, w, False, p))
    with pytest.raises(ValueError):
        ST.stretch(x, _blk(p), out=out[:1])
    with pytest.raises(RuntimeError):
        ST.stretch(x, _blk(p), out=x)                                  # the output overlaps the input
    with pytest.raises(RuntimeError):
        ST.stretch(x, [_blk(p)] * 4)                                    # neither 1, N nor N*C blocks
    with pytest.raises(RuntimeError):
        ST.stretch(x, [_blk(p)] * (n * 3))                              # a luminance model per plane
    with pytest.raises(RuntimeError):
        ST.mtf(x, 0.5, 0.5, 0.5)
    with pytest.raises(ValueError):
        ST.mtf(x.double(), 0.0, 0.5, 1.0)


def test_a_parameter_block_per_image_and_per_plane():
    from siril_amd import stretch as ST
    n, h, w = SHAPES[2]
    x = _scene(n, 3, h, w)
    per_image = [_ght(R.GHT, 6.0, 3.0, model=R.HUMAN), _ght(R.INVGHT, 2.0, -1.5)]
    got = ST.stretch(_dev(x), [_blk(p) for p in per_image]).cpu().numpy()
    for i, p in enumerate(per_image):
        _same(got[i:i + 1], R.stretch(p, x[i:i + 1]))
    per_plane = [R.Params(R.MTF, lo=0.01 * k, m=0.1 + 0.1 * k, hi=1.0 - 0.02 * k) for k in range(n * 3)]
    per_plane[4] = _ght(R.GHT, 10.0, 0.0)
    got = ST.stretch(_dev(x), [_blk(p) for p in per_plane]).cpu().numpy()
    for k, p in enumerate(per_plane):
        i, ch = divmod(k, 3)
        _same(got[i, ch][None], R.stretch(p, x[i, ch][None]))


def _auto_scene(n, c, h, w, word):
    """Distinct samples in every plane, none of them 0: a level per channel (channel 1 above 0.5) and a spread of
    0.1, so that the shadows clip saturates nowhere."""
    rng = np.random.RandomState(h * w + c + word)
    nch, npix = max(c, 1), h * w
    k = np.stack([rng.permutation(npix) for _ in range(n * nch)]).reshape(n, nch, npix)
    level = np.array([0.3, 0.62, 0.4])[:nch][None, :, None]
    if word:
        x = (np.rint(level * 65535.0).astype(np.int64) + k * max(1, 6553 // npix)).astype(np.uint16)
    else:
        x = (level + 0.1 * k / npix).astype(F)
    return x.reshape((n, nch, h, w) if c else (n, h, w))


@pytest.mark.parametrize("word", (False, True))
@pytest.mark.parametrize("linked", (False, True))
def test_autostretch(word, linked):
    from siril_amd import stretch as ST
    for n, c, h, w in ((2, 3, 7, 5), (1, 0, 97, 71), (1, 3, 97, 71)):
        x = _auto_scene(n, c, h, w, word)
        planes = x.reshape(n * max(c, 1), -1)
        assert planes.shape[1] % 2 == 1 and (planes != 0).all()
        # WORD planes: norm_stats' median and MAD are exact order statistics, numpy's medians.  float planes: its median
        # and MAD are Siril's histogram percentile with interpolation, which is no order statistic; the reference
        # is that rule restated in numpy (tests/test_normalization.py), so that the comparison stays one of the stretch.
        if word:
            med = np.median(planes, axis=1)
            mad = np.median(np.abs(planes.astype(np.int64) - med[:, None].astype(np.int64)), axis=1)
            med, mad = med / 65535.0, mad / 65535.0
        else:
            from test_normalization import np_percentile_half
            med32 = [np_percentile_half(p) for p in planes]
            mad = np.array([float(np_percentile_half(np.abs(p - m))) for p, m in zip(planes, med32)])
            med = np.array([float(m) for m in med32])
            assert np.abs(med - np.median(planes, axis=1)).max() <= 0.1 / planes.shape[1]    # within a histogram bin
        assert all(len(np.unique(p)) == len(p) for p in planes)          # no ties at the median
        for clip, target in ((-2.8, 0.25), (-1.5, 0.3)):
            want_params = R.autostretch_params(med, mad, n, max(c, 1), linked, clip, target)
            got, used = ST.autostretch(_dev(x), linked=linked, shadows_clip=clip, target_bg=target)
            assert np.array_equal(used.view(np.uint64), want_params.view(np.uint64))
            if c == 3 and not linked:
                assert used[1, 0] == 0.0 and used[1, 2] < 1.0 and used[0, 2] == 1.0     # plane 1 is inverted
            got = got.cpu().numpy()
            for k, (lo, m, hi) in enumerate(want_params):
                _same(got.reshape(planes.shape[0], -1)[k], R.stretch(R.Params(R.MTF, lo=lo, m=m, hi=hi), planes[k]))


def test_coefficient_blocks_equal_the_restatement():
    from siril_amd import stretch as ST
    ps = _functions()
    for B in BS:
        for D in (0.1, 1.0, 3.0, 6.0, 10.0):
            for lp, sp, hp in ((0, 0, 1), (.02, .1, .8), (0, .3, .3), (.25, .25, 1), (.1, .5, .9), (0, 1, 1), (.5, .5, .5)):
                ps.append(R.Params(R.GHT, D=D, B=B, LP=lp, SP=sp, HP=hp))
                ps.append(R.Params(R.INVMODASINH, D=D, LP=lp, SP=sp, HP=hp))
    for p in ps:
        assert np.array_equal(ST.coeffs(_blk(p)).view(np.uint64), R.coeffs(p)[0].view(np.uint64)), p


def test_kernel_time_is_reported():
    from siril_amd import stretch as ST
    from siril_amd.stacking import Context
    ctx = Context(0)
    n, h, w = SHAPES[3]
    x = _dev(_scene(n, 3, h, w))
    ST.stretch(x, [_blk(_ght(R.GHT, 6.0, 3.0))], ctx=ctx)
    ms, launches = ST.last_kernel_ms(ctx)
    assert ms > 0.0 and launches == 1
    ST.stretch(x, [_blk(R.Params(R.MTF, m=0.1 + 0.1 * k)) for k in range(3)], ctx=ctx)
    assert ST.last_kernel_ms(ctx)[1] == 3
    ctx.close()

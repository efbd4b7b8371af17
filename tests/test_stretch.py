"""Properties of the stretches' restatement (tests/stretch_ref.py)
and of the command parsers (siril_amd/stretch.py); no GPU.

The grid is every B in {-5, -1.5, -1, -0.5, 0, 0.5, 3, 15} and modasinh, every
D_user in {0.1, 1, 3, 6, 10} and seven (LP, SP, HP), 315 transfers on 10^5
points each.  Measured with this restatement over that grid:

  against libm (np.log / np.exp / np.power / np.arcsinh in the same formulas):
  largest difference in double 4.55e-15; after rounding to float32 3.2e-6 % of
  the samples (1 of 31.5 million) are one ulp apart and none more.  The bound
  ulp32(value) + 2^-40 is derived, not measured: exp and log here are good to a few 1e-16 relative, pow
  multiplies that by |p log a| <= 13 on the forward side, and the
  normalisation by 1/(S(1) - S(0)) keeps the error in double orders of
  magnitude under a float32 ulp (6e-8 relative), so the two float32 results are
  the same or neighbours; 2^-40 covers the cancellation next to T = 0, where an
  ulp of the value says nothing.

  the inverse: the largest |T(Tinv(y)) - y| in double, y = float32(T(x)), is
  7.7e-13 (B = 0.5, D_user = 10, LP = 0, SP = HP = 1); the bound asserted is 16
  times that, 1.23e-11.  A measurement above 1e-11 would be a defect of the
  specified inverse; 7.7e-13 is well under it."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BS = (-5.0, -1.5, -1.0, -0.5, 0.0, 0.5, 3.0, 15.0, "asinh")
DS = (0.1, 1.0, 3.0, 6.0, 10.0)
PIECES = ((0, 0, 1), (.02, .1, .8), (0, .3, .3), (.25, .25, 1), (.1, .5, .9), (0, 1, 1), (.5, .5, .5))
X = np.linspace(0.0, 1.0, 100001)
X.setflags(write=False)
INVERSE_MEASURED = 7.7e-13
INVERSE_BOUND = 16 * INVERSE_MEASURED


def _params(B, D, pieces, inverse=False):
    lp, sp, hp = pieces
    if B == "asinh":
        return R.Params(R.INVMODASINH if inverse else R.MODASINH, D=D, LP=lp, SP=sp, HP=hp)
    return R.Params(R.INVGHT if inverse else R.GHT, D=D, B=B, LP=lp, SP=sp, HP=hp)


@functools.lru_cache(maxsize=None)
def _T(B, D, pieces):
    c, regime = R.coeffs(_params(B, D, pieces))
    t = R.T(c, regime, X)
    t.setflags(write=False)
    return c, regime, t


# ---- the transcendentals ----
def test_exp_is_total_and_accurate():
    x = np.concatenate([np.linspace(-708.0, 708.0, 200001), [-22026.0, -1e300, 1e300, 0.0]])
    e = R.s_exp(x)
    assert np.isfinite(e).all() and (e > 0.0).all()
    assert e[-1] == 1.0 and e[-4] == e[0] and e[-3] == e[0] and e[-2] == R.s_exp(np.array(708.0))
    inner = np.abs(x) <= 700.0
    assert np.abs(e[inner] / np.exp(x[inner]) - 1.0).max() < 4e-16
    assert np.isnan(R.s_exp(np.array(np.nan))) and np.isnan(R.s_log(np.array(np.nan)))
    a = np.logspace(-300, 300, 100001)
    assert np.abs(R.s_log(a) - np.log(a)).max() <= 2e-16 * 700
    v = np.logspace(-3, 6, 10001)
    assert np.abs(R.s_asinh(v) / np.arcsinh(v) - 1.0).max() < 1e-12
    b = np.linspace(1.0, 4e5, 10001)
    for p in (0.8, -1.0 / 15.0, -2.0, -16.0 / 15.0):
        assert np.abs(R.s_pow(b, p) / np.power(b, p) - 1.0).max() < 1e-14


# ---- ranges ----
@pytest.mark.parametrize("B", BS)
def test_T_ranges(B):
    for D in DS:
        for pieces in PIECES:
            c, regime, t = _T(B, D, pieces)
            assert t[0] == 0.0, (B, D, pieces)
            assert abs(t[-1] - 1.0) <= 1e-14, (B, D, pieces, t[-1])
            assert np.isfinite(t).all() and t.min() >= 0.0 and t.max() <= 1.0, (B, D, pieces)
            assert (np.diff(t) >= 0.0).all(), (B, D, pieces)
            assert np.isfinite(c).all()


def test_q_at_zero_and_identity():
    for B in BS:
        c, regime = R.coeffs(_params(B, 3.0, (.02, .1, .8)))
        assert float(R.q(c, regime, 0.0)) == 0.0 and float(R.dq(c, regime, 0.0)) == c[R.G_D]
    p = R.Params(R.GHT, D=0.0, B=3.0, SP=0.2)
    assert R.coeffs(p)[1] == R.Q_IDENTITY
    x = np.array([-1.0, 0.0, 0.25, 1.0, 2.0], np.float32)
    assert np.array_equal(R.stretch(p, x[None, None]).ravel(), np.array([0, 0, .25, 1, 1], np.float32))
    assert np.array_equal(R.stretch(R.Params(R.INVGHT, D=0.0), x[None, None]).ravel(), np.array([0, 0, .25, 1, 1], np.float32))


# ---- agreement with libm ----
def _T_libm(B, D_user, pieces, x):
    lp, sp, hp = pieces
    D = np.exp(D_user) - 1.0
    b = abs(B) if B != "asinh" else 0.0

    def q(u):
        if B == "asinh":
            return np.arcsinh(D * u)
        if B == -1.0:
            return np.log(1.0 + D * u)
        if B < 0.0:
            return (1.0 - np.power(1.0 + b * D * u, (b - 1.0) / b)) / (1.0 - b)
        if B == 0.0:
            return 1.0 - np.exp(-D * u)
        return 1.0 - np.power(1.0 + B * D * u, -1.0 / B)

    def dq(u):
        if B == "asinh":
            return D / np.sqrt(1.0 + (D * u) ** 2)
        if B == -1.0:
            return D / (1.0 + D * u)
        if B < 0.0:
            return D * np.power(1.0 + b * D * u, -1.0 / b)
        if B == 0.0:
            return D * np.exp(-D * u)
        return D * np.power(1.0 + B * D * u, -(1.0 + B) / B)

    def S(x):
        x = np.asarray(x, np.float64)
        t = np.clip(x, lp, hp)
        s = np.where(t < sp, -q(np.abs(t - sp)), q(np.abs(t - sp)))
        return s + np.where(x < lp, dq(sp - lp), np.where(x > hp, dq(hp - sp), 0.0)) * (x - t)
    return np.clip((S(x) - S(0.0)) / (S(1.0) - S(0.0)), 0.0, 1.0)


def test_agreement_with_libm():
    worst, apart, total = 0.0, 0, 0
    for B in BS:
        for D in DS:
            for pieces in PIECES:
                t = _T(B, D, pieces)[2]
                lm = _T_libm(B, D, pieces, X)
                worst = max(worst, float(np.abs(t - lm).max()))
                a, b = t.astype(np.float32), lm.astype(np.float32)
                bound = np.spacing(np.maximum(a, b)).astype(np.float64) + 2.0 ** -40
                assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= bound).all(), (B, D, pieces)
                apart += int((a != b).sum())
                total += a.size
    print(f"libm: largest double difference {worst:.3g}, float32 results apart {100.0 * apart / total:.3g} %")
    assert worst < 1e-13


# ---- the inverse ----
def test_inverse_against_the_forward_function():
    worst, where = 0.0, None
    for B in BS:
        for D in DS:
            for pieces in PIECES:
                c, regime, t = _T(B, D, pieces)
                y = t.astype(np.float32).astype(np.float64)
                x = R.Tinv(c, regime, y)
                assert np.isfinite(x).all() and x.min() >= 0.0 and x.max() <= 1.0
                e = float(np.abs(R.T(c, regime, x) - y).max())
                if e > worst:
                    worst, where = e, (B, D, pieces)
    print(f"inverse: largest |T(Tinv(y)) - y| {worst:.3g} at {where}; bound {INVERSE_BOUND:.3g}")
    assert worst <= 1e-11, "the specified inverse is defective"
    assert worst <= INVERSE_BOUND, (worst, where)


def test_no_stretch_yields_nan_or_inf_from_finite_input():
    x = np.concatenate([X, [-5.0, 7.0, 1e-45, 1e-300, 1.0 - 2.0 ** -53]])
    for B in BS:
        for D in (0.1, 10.0):
            for pieces in PIECES:
                for inverse in (False, True):
                    p = _params(B, D, pieces, inverse)
                    r = R.sample(p, x)
                    assert np.isfinite(r).all() and r.min() >= 0.0 and r.max() <= 1.0, (B, D, pieces, inverse)
    for p in (R.Params(R.ASINH, beta=1000.0, offset=0.5), R.Params(R.ASINH, beta=1.0), R.Params(R.LINEAR, BP=0.999),
              R.Params(R.MTF, lo=0.2, m=1e-6, hi=0.2 + 1e-9), R.Params(R.MTF, m=1.0 - 1e-9)):
        r = R.sample(p, x)
        assert np.isfinite(r).all() and r.min() >= 0.0 and r.max() <= 1.0, p
    assert np.isnan(R.sample(R.Params(R.GHT, D=3.0, B=3.0), np.array([np.nan]))).all()


# ---- mtf and autostretch ----
def test_mtf():
    for m in (0.01, 0.25, 0.5, 0.9):
        # five roundings of 2^-53 each, the denominator's subtraction amplifying them at most 5 times at m = 0.9
        assert abs(float(R.mtf01(m, m)) - 0.5) <= 1e-14
        assert float(R.mtf01(0.0, m)) == 0.0 and float(R.mtf01(1.0, m)) == 1.0
    p = R.Params(R.MTF, lo=0.1, m=0.2, hi=0.9)
    x = np.array([0.0, 0.1, 0.1 + 0.8 * 0.2, 0.9, 1.0])
    assert np.allclose(R.sample(p, x), [0, 0, 0.5, 1, 1], atol=1e-15)
    t = R.sample(p, X)
    assert (np.diff(t) >= 0).all()


def _plane_stats(rng, level, spread, npix=6887):
    x = (level + spread * rng.randn(npix)).astype(np.float32)
    med = float(np.median(x))
    return med, float(np.median(np.abs(x - np.float32(med))))


def test_autostretch_sends_the_median_to_the_target():
    rng = np.random.RandomState(5)
    stats = [_plane_stats(rng, lv, sp) for lv, sp in ((0.1, 0.01), (0.3, 0.02), (0.7, 0.03), (0.9, 0.01))]
    med, mad = np.array([s[0] for s in stats]), np.array([s[1] for s in stats])
    for clip, target in ((-2.8, 0.25), (-1.5, 0.1), (-0.5, 0.5)):
        par = R.autostretch_params(med, mad, 4, 1, False, clip, target)
        for k, (lo, m, hi) in enumerate(par):
            inverted = med[k] > 0.5
            # the shadows clip does not saturate
            assert (lo == 0.0 and med[k] < hi < 1.0) if inverted else (0.0 < lo < med[k] and hi == 1.0)
            got = float(R.sample(R.Params(R.MTF, lo=lo, m=m, hi=hi), np.array(med[k])))
            # an inverted plane's background is bright: its median goes to 1 - target
            assert abs(got - ((1.0 - target) if inverted else target)) <= 1e-12, (k, clip, target, got)


def test_autostretch_linked():
    rng = np.random.RandomState(6)
    s = _plane_stats(rng, 0.12, 0.015)
    med, mad = np.array([s[0]] * 3), np.array([s[1]] * 3)
    un = R.autostretch_params(med, mad, 1, 3, False)
    li = R.autostretch_params(med, mad, 1, 3, True)
    assert np.array_equal(un.view(np.uint64), li.view(np.uint64)) and (un == un[0]).all()
    # two of three channels above 0.5: the linked image is inverted, one of three: it is not
    stats = [_plane_stats(rng, lv, 0.02) for lv in (0.7, 0.8, 0.3)]
    med, mad = np.array([t[0] for t in stats]), np.array([t[1] for t in stats])
    li = R.autostretch_params(med, mad, 1, 3, True)
    assert (li == li[0]).all() and li[0, 0] == 0.0 and li[0, 2] < 1.0
    un = R.autostretch_params(med, mad, 1, 3, False)
    assert un[2, 2] == 1.0 and un[0, 0] == 0.0
    li = R.autostretch_params(1.0 - med, mad, 1, 3, True)
    assert (li == li[0]).all() and li[0, 2] == 1.0 and li[0, 0] > 0.0
    got = float(R.sample(R.Params(R.MTF, lo=li[0, 0], m=li[0, 1], hi=1.0), np.array(np.mean(1.0 - med))))
    assert abs(got - 0.25) <= 1e-12
    for bad in (dict(clip=1.0), dict(clip=float("nan")), dict(target=0.0), dict(target=1.0)):
        with pytest.raises(ValueError):
            R.autostretch_params(med, mad, 1, 3, **bad)
    with pytest.raises(ValueError):
        R.autostretch_params(np.array([0.2]), np.array([0.0]), 1, 1)


# ---- colour models ----
def _pixels():
    rng = np.random.RandomState(7)
    x = (rng.rand(3, 4000) ** 2).astype(np.float32)
    x[:, 0] = 0.0
    x[:, 1] = (0.95, 0.02, 0.02)
    x[:, 2] = (0.9, 0.85, 0.01)
    return x


@pytest.mark.parametrize("model", (R.HUMAN, R.EVEN))
@pytest.mark.parametrize("fn", (R.GHT, R.MODASINH, R.INVGHT))
def test_colour_models(model, fn):
    x = _pixels()
    xd = x.astype(np.float64)
    base = dict(D=6.0 if fn != R.INVGHT else 2.0, B=3.0 if fn == R.GHT else -1.5 if fn == R.INVGHT else 0.0, SP=0.05,
                model=model)
    p = R.Params(fn, clipmode=R.CLIP, **base)
    c, regime = R.coeffs(p)
    L = R.lum(p, xd)
    with np.errstate(all="ignore"):
        s = xd * np.where(L == 0.0, 0.0, R.transfer(p, c, regime, L) / L)[None]
    clips = (s > 1.0).any(0)
    # the inverse darkens (Tinv(L) <= L), so only the forward functions push a channel past 1
    assert clips.any() == (fn != R.INVGHT) and (~clips).sum() > 100
    for mode in (R.CLIP, R.RESCALE, R.RGBBLEND):
        o = R.pixel3(R.Params(fn, clipmode=mode, **base), xd)
        assert o.max() <= 1.0 and o.min() >= 0.0, mode
        assert np.array_equal(o[:, ~clips].view(np.uint64), s[:, ~clips].view(np.uint64)), mode
        assert (o[:, 0] == 0.0).all()                                   # the black pixel
        if mode == R.RESCALE and clips.any():
            assert np.allclose(o[:, clips].max(0), 1.0, atol=1e-15)
        if mode == R.RGBBLEND and clips.any():
            assert np.allclose(o[:, clips].max(0), 1.0, atol=1e-12)
    # a NaN in one channel makes the whole pixel NaN
    y = xd.copy()
    y[1, 5] = np.nan
    o = R.pixel3(p, y)
    assert np.isnan(o[:, 5]).all() and int(np.isnan(o).sum()) == 3


def test_channel_mask_passes_bits_through():
    x = _pixels().reshape(1, 3, 40, 100).copy()
    x[0, 1, 0, 7] = -0.5
    x[0, 1, 0, 8] = 1.5
    full = R.stretch(R.Params(R.GHT, D=6.0, B=3.0, SP=0.05, model=R.HUMAN), x)
    for mask in (1, 2, 4, 3, 5, 6):
        o = R.stretch(R.Params(R.GHT, D=6.0, B=3.0, SP=0.05, model=R.HUMAN, mask=mask), x)
        for ch in range(3):
            want = full if mask >> ch & 1 else x
            assert np.array_equal(o[:, ch].view(np.uint32), want[:, ch].view(np.uint32)), (mask, ch)
    w = (x * 65535).clip(0, 65535).astype(np.uint16)
    o = R.stretch(R.Params(R.MTF, m=0.2, mask=5), w)
    assert np.array_equal(o[:, 1], (w[:, 1].astype(np.float64) / 65535.0).astype(np.float32))


def test_asinh():
    v = np.linspace(0.0, 1.0, 10001)
    for beta in (1.0, 30.0, 1000.0):
        r = R.sample(R.Params(R.ASINH, beta=beta), v)
        assert r[0] == 0.0 and abs(r[-1] - 1.0) < 1e-15 and (np.diff(r) >= 0).all() and r.max() <= 1.0
    p = R.Params(R.ASINH, beta=100.0, offset=0.1, model=R.HUMAN)
    grey = np.stack([v, v, v])
    assert np.allclose(R.pixel3(p, grey)[1], R.sample(p, v), atol=1e-15)
    assert (R.sample(p, np.array([0.0, 0.05, 0.1])) == 0.0).all()


# ---- refusals ----
def test_refusals():
    bad = [R.Params(9), R.Params(R.GHT, model=3), R.Params(R.GHT, clipmode=3), R.Params(R.GHT, mask=0),
           R.Params(R.GHT, mask=8), R.Params(R.MTF, lo=0.5, hi=0.5), R.Params(R.MTF, lo=0.6, hi=0.5),
           R.Params(R.MTF, m=0.0), R.Params(R.MTF, m=1.0), R.Params(R.MTF, m=float("nan")), R.Params(R.MTF, lo=-0.1),
           R.Params(R.MTF, hi=1.1), R.Params(R.LINEAR, BP=1.0), R.Params(R.LINEAR, BP=-0.1),
           R.Params(R.ASINH, beta=0.5), R.Params(R.ASINH, beta=1001.0), R.Params(R.ASINH, offset=1.0),
           R.Params(R.ASINH, offset=-0.1), R.Params(R.GHT, D=-1.0), R.Params(R.GHT, D=10.5),
           R.Params(R.INVGHT, D=1.0, B=-5.5), R.Params(R.GHT, D=1.0, B=15.5), R.Params(R.GHT, D=1.0, LP=0.3, SP=0.2),
           R.Params(R.MODASINH, D=1.0, SP=0.5, HP=0.4), R.Params(R.GHT, D=1.0, HP=1.5),
           R.Params(R.INVMODASINH, D=1.0, LP=-0.1)]
    for p in bad:
        with pytest.raises(ValueError):
            R.check(p)
    R.check(R.Params(R.MODASINH, D=1.0, B=99.0))         # modasinh has no B


def test_parsers():
    from siril_amd.stretch import parse_stretch_command as parse
    c = parse("ght img -D=3 -B=-1.5 -LP=0.01 -SP=0.1 -HP=0.9 -human -clipmode=clip RG -out=x.fit".split())
    assert (c.command, c.image, c.out) == ("ght", "img", "x.fit")
    assert c.kwargs == dict(D=3.0, B=-1.5, LP=0.01, SP=0.1, HP=0.9, model="human", clipmode="clip", channels="RG")
    assert parse("invmodasinh i -D=1 -even b".split()).kwargs == dict(D=1.0, model="even", channels="B")
    assert parse("autostretch i".split()).kwargs == {}
    assert parse("autostretch i -linked -1.5 0.3".split()).kwargs == dict(linked=True, shadows_clip=-1.5, target_bg=0.3)
    assert parse("asinh i -human 100 0.01".split()).kwargs == dict(human=True, stretch_factor=100.0, offset=0.01)
    assert parse("mtf i 0 .2 1 gb".split()).kwargs == dict(lo=0.0, m=0.2, hi=1.0, channels="GB")
    assert parse("linstretch i -BP=0.1".split()).kwargs == dict(BP=0.1)
    for line in ("ght", "ght i", "ght i -D=11", "ght i -D=x", "ght i -D=1 -B=16", "ght i -D=1 -LP=0.5 -SP=0.4",
                 "ght i -D=1 -HP=0.4 -SP=0.5", "ght i -D=1 -human -even", "ght i -D=1 -clipmode=soft", "ght i -D=1 X",
                 "ght i -D=1 R G", "ght i -D=1 -bogus", "ght i -D=1 -out=", "modasinh i -D=1 -B=2", "invmodasinh i -B=2 -D=1",
                 "invght i -B=1", "mtf i 0 .2", "mtf i 0 0 1", "mtf i 0 1 1", "mtf i .5 .5 .5", "mtf i 0 .5 2",
                 "mtf i 0 .5 1 X", "mtf i 0 .5 1 R G", "mtf i 0 nan 1", "mtf i a .5 1", "mtf 0 .5 1", "mtf i 0 .5 1 -linked",
                 "autostretch", "autostretch i 2.8", "autostretch i -2.8 0", "autostretch i -2.8 1", "autostretch i -2.8 .2 .3",
                 "autostretch i -human", "autostretch i -inf", "linstretch i", "linstretch i -BP=1", "linstretch i -BP=x",
                 "linstretch i 0.1", "linstretch i -BP=.1 -D=1", "asinh i", "asinh i 0.5", "asinh i 1001", "asinh i 10 1",
                 "asinh i 10 .1 .2", "asinh i 10 -even", "asinh i x", "stretchy i"):
        with pytest.raises(ValueError):
            parse(line.split())
    with pytest.raises(ValueError, match="Unexpected argument to ght `-bogus', aborting."):
        parse("ght i -D=1 -bogus".split())

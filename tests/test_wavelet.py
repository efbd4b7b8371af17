"""The a trous wavelets without a GPU: the refusals of sgpu_wavelet_check at
their exact boundary, the parsers of `wavelet` and `wrecons`, and the
restatement (tests/wavelet_ref.py) itself: an impulse gives the outer product
of the dilated taps, a constant plane gives details exactly 0, and all-ones
coefficients return the input within the rounding of the sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavelet_ref as WR  # noqa: E402

SHAPES = [(33, 33), (71, 97), (65, 129)]       # (H, W)


# ---- refusals ------------------------------------------------------------------
def test_check_refusals_and_exact_boundary():
    from siril_amd import SgpuError
    from siril_amd.wavelets import check_layers
    check_layers(33, 33, 6, 2)                  # m = 32 = min - 1
    for w, h in ((32, 40), (40, 32)):
        with pytest.raises(SgpuError) as e:
            check_layers(w, h, 6, 2)
        assert e.value.code != 0 and "too small" in str(e.value)
        check_layers(w, h, 5, 2)
        check_layers(w, h, 6, 1)                # the linear filter reaches half as far: one layer further
    check_layers(17, 17, 5, 2)
    check_layers(17, 17, 6, 1)
    for bad in ((17, 17, 6, 2), (16, 17, 6, 1), (100, 100, 0, 2), (100, 100, 7, 2), (100, 100, 3, 0), (100, 100, 3, 3),
                (1, 1, 2, 1)):
        with pytest.raises(SgpuError):
            check_layers(*bad)
    check_layers(1, 1, 1, 2)                    # n = 1 uses no tap
    for w in range(1, 40):
        for n in range(1, 7):
            for t in (1, 2):
                ok = WR.check(w, w + 3, n, t) is None
                try:
                    check_layers(w, w + 3, n, t)
                    assert ok, (w, n, t)
                except SgpuError:
                    assert not ok, (w, n, t)


# ---- parsers -------------------------------------------------------------------
def test_parse_wavelet():
    from siril_amd.wavelets import parse_wavelet_command as P
    c = P("wavelet moon 6 2".split())
    assert (c.image, c.nbr_layers, c.type, c.prefix) == ("moon", 6, 2, "")
    c = P(["moon.fit", "3", "1", "-prefix=w_"])
    assert (c.image, c.nbr_layers, c.type, c.prefix) == ("moon.fit", 3, 1, "w_")
    for bad in ("wavelet", "wavelet moon", "wavelet moon 6", "wavelet moon 0 2", "wavelet moon 7 2", "wavelet moon 3 3",
                "wavelet moon x 2", "wavelet moon 3 2 -layers=2", "wavelet moon 3 2 extra", "wavelet -prefix=a 3 2"):
        with pytest.raises(ValueError):
            P(bad.split())


def test_parse_wrecons():
    from siril_amd.wavelets import parse_wrecons_command as P
    c = P("wrecons moon 3 2 1.5 1 1 1".split())
    assert (c.image, c.coefs, c.type, c.out) == ("moon", [3.0, 2.0, 1.5, 1.0, 1.0, 1.0], 2, "")
    c = P(["moon", "-1.5", "0", "-type=1", "-out=sharp.fit"])
    assert (c.coefs, c.type, c.out) == ([-1.5, 0.0], 1, "sharp.fit")
    for bad in ("wrecons", "wrecons moon", "wrecons moon 1 1 1 1 1 1 1", "wrecons moon 1 -type=3", "wrecons moon 1 -out=",
                "wrecons moon 1 nan", "wrecons moon 1 inf", "wrecons moon 1 1e39", "wrecons moon 1 -clamp",
                "wrecons moon 1 -type=2 1", "wrecons -type=2 1"):
        with pytest.raises(ValueError):
            P(bad.split())


def test_cli_doc_names_the_commands():
    from siril_amd import cli
    assert "wavelet <image> <nbr_layers> <type>" in cli.__doc__ and "wrecons <image> c1" in cli.__doc__


# ---- the restatement -------------------------------------------------------------
@pytest.mark.parametrize("type_", [1, 2])
def test_impulse_gives_outer_product_of_dilated_taps(type_):
    h, w, n = 161, 151, 6
    x = np.zeros((h, w), np.float32)
    cy, cx = 80, 75
    x[cy, cx] = 1.0
    for j in range(n - 1):
        s = 1 << j
        t = WR.taps(type_, s)
        r = len(t) // 2
        want = np.zeros_like(x)
        want[cy - r:cy + r + 1, cx - r:cx + r + 1] = np.outer(t, t)      # products of powers of two: exact
        assert np.array_equal(WR.smooth(x, s, type_), want), j
    planes = WR.transform(x, n, type_)
    assert np.array_equal(planes[0], x - WR.smooth(x, 1, type_))
    assert abs(float(planes.astype(np.float64).sum()) - 1.0) < 1e-6     # the planes sum to the impulse
    # at the border the response folds back: whole-sample reflection
    x = np.zeros((h, w), np.float32)
    x[0, 0] = 1.0
    t = WR.taps(type_, 1)
    r = len(t) // 2
    fold = t[r:].copy()
    fold[1:] += t[:r][::-1]
    got = WR.smooth(x, 1, type_)
    assert np.array_equal(got[:r + 1, :r + 1], np.outer(t[r:], t[r:])) and fold.sum() == 1.0


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_plane(shape, type_):
    n = 6
    planes = WR.transform(np.full(shape, 0.25, np.float32), n, type_)
    assert np.array_equal(planes[:n - 1].view(np.uint32), np.zeros((n - 1,) + shape, np.uint32))
    assert np.array_equal(planes[n - 1], np.full(shape, 0.25, np.float32))


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_ones_returns_the_input(shape, type_):
    """One rounding per subtraction and per addition: 2(n-1) roundings of
    magnitudes at most 2 max|x| each, 4(n-1) 2^-24 max|x|."""
    x = WR.scene(*shape, seed=3)
    for n in range(1, 7):
        back = WR.reconstruct(WR.transform(x, n, type_), np.ones(n))
        err = float(np.max(np.abs(back.astype(np.float64) - x)))
        bound = 4 * (n - 1) * 2.0 ** -24 * float(np.max(np.abs(x)))
        print(shape, type_, n, err, bound)
        assert err <= bound, (n, err, bound)


def test_word_scaling_and_layout():
    x = WR.scene(40, 50, seed=1, word=True)
    pl = WR.transform(x, 3, 2)
    assert pl.shape == (3, 40, 50) and pl.dtype == np.float32
    assert np.array_equal(pl, WR.transform(x.astype(np.float32) * np.float32(1.0 / 65535.0), 3, 2))
    batch = np.stack([x, x[::-1].copy()])
    assert np.array_equal(WR.transform(batch, 3, 2)[1], WR.transform(batch[1], 3, 2))
    assert np.array_equal(WR.wrecons(x, (2, 1, 1)), WR.reconstruct(pl, (2, 1, 1)))

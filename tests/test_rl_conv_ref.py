"""The references of tests/rl_conv_ref.py against independent restatements
(no GPU): conv_exact against a float64 FFT circular convolution and the
oracle's zero-border correlation, conv_f32_fft against conv_exact on the
integer inputs the GPU tests use, the epilogue restatements on hand values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rl_conv_ref as RC  # noqa: E402

from oracle import rl_ref as R  # noqa: E402


def _fft64_circular(x, k):
    H, W = x.shape
    ks = k.shape[0]
    h = ks // 2
    kp = np.zeros((H, W), np.float64)
    for ky in range(ks):          # taps that alias (ks > n) add up
        for kx in range(ks):
            kp[(ky - h) % H, (kx - h) % W] += k[ky, kx]
    return np.fft.ifft2(np.fft.fft2(x.astype(np.float64)) * np.fft.fft2(kp)).real


@pytest.mark.parametrize("H,W,ks", [(9, 11, 3), (16, 16, 15), (5, 7, 9), (33, 20, 21), (2, 3, 7)])
def test_conv_exact_circular_matches_fft64(H, W, ks):
    """Five shapes, three of them with ks > n in a dimension (aliasing taps)."""
    x, k = RC.int_image(H, W), RC.int_taps(ks)
    got = RC.conv_exact(x, k, 1)
    assert got.dtype == np.int64
    assert np.abs(got - _fft64_circular(x, k)).max() <= 1e-9 * max(1.0, np.abs(got).max())
    xf = RC.float_image(H, W)
    kf = RC.moffat_taps(ks)
    gf = RC.conv_exact(xf, kf, 1)
    assert gf.dtype == np.float64
    assert np.abs(gf - _fft64_circular(xf, kf)).max() <= 1e-9


@pytest.mark.parametrize("H,W,ks", [(1, 1, 3), (5, 200, 15), (9, 11, 3), (20, 17, 7), (3, 4, 9)])
def test_conv_exact_zero_border_matches_oracle_correlation(H, W, ks):
    """conv2_zero is a correlation: with the fully flipped kernel it is the
    convolution ConvArgs::taps defines."""
    x, k = RC.int_image(H, W), RC.int_taps(ks)
    want = R.conv2_zero(x.astype(np.float64), k[::-1, ::-1].astype(np.float64))
    assert np.array_equal(RC.conv_exact(x, k, 0).astype(np.float64), want)


def test_conv_exact_places_one_tap():
    """c[y][x] = sum k[ky][kx] in[y + h - ky][x + h - kx]: a single tap at
    (ky, kx) = (0, 2) of a 3 x 3 kernel reads in[y + 1][x - 1]."""
    x = np.arange(20).reshape(4, 5)
    k = np.zeros((3, 3), np.int64)
    k[0, 2] = 1
    assert np.array_equal(RC.conv_exact(x, k, 1), np.roll(x, (-1, 1), axis=(0, 1)))
    z = RC.conv_exact(x, k, 0)
    assert np.array_equal(z[:-1, 1:], x[1:, :-1]) and not z[-1].any() and not z[:, 0].any()


def test_smooth_lengths():
    for need, want in ((16, 16), (17, 18), (128, 128), (251, 256), (487, 500), (8192, 8192), (8193, 0), (6155, 6250)):
        assert RC.fft_smooth_len(need) == want
    for H, W, ks in RC.FFT_CASES:
        assert RC.fft_smooth_len(W + 3 * (ks // 2)) and RC.fft_smooth_len(H + 3 * (ks // 2))
    assert sorted({RC.fft_smooth_len(W + 3) for _, W, ks in RC.FFT_CASES if ks == 3}) == \
        [16, 128, 162, 250, 360, 486, 512, 600, 1080, 8192]
    assert sorted({RC.fft_smooth_len(H + 3) for H, _, ks in RC.FFT_CASES if ks == 3}) == \
        [16, 128, 162, 250, 360, 486, 512, 600, 1080, 8192]


@pytest.mark.parametrize("H,W,ks", RC.FFT_CASES)
def test_conv_f32_fft_rounds_to_exact(H, W, ks):
    """On the integer inputs the single-precision FFT convolution rounds to
    the exact integers.  Its error is also held to 2e-6 of max|c|: a float32
    FFT convolution errs by about eps * log2(n1 n2) of the result's scale,
    6e-8 * 26 = 1.6e-6 at the largest plane here (a few 1e-7 are typical)."""
    x, k = RC.int_image(H, W), RC.int_taps(ks)
    want = RC.conv_exact(x, k, 1)
    got = RC.conv_f32_fft(x, k)
    assert got.dtype == np.float32 and got.shape == (H, W)
    assert np.array_equal(np.rint(got).astype(np.int64), want)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"conv_f32_fft {H}x{W} ks={ks}: max err {err:.3e}, max|c| {np.abs(want).max()}")
    assert err <= 2e-6 * np.abs(want).max()


def test_epilogues_on_hand_values():
    c = np.array([[0.0, 2.0, np.nan, -4.0]], np.float32)
    f = np.array([[3.0, 3.0, 3.0, 3.0]], np.float32)
    e = np.array([[1.0, 0.5, 2.0, 4.0]], np.float32)
    w = np.array([[0.5, 0.5, 0.5, 0.5]], np.float32)
    nine = np.float32(1e-9)
    assert np.array_equal(RC.epilogue(RC.EPI_RATIO, c, f=f), np.array([[3 / nine, 1.5, 3 / nine, -0.75]], np.float32))
    assert np.array_equal(RC.epilogue(RC.EPI_RATIO_NAIVE, c, f=f), np.array([[np.inf, 1.5, nine, nine]], np.float32))
    assert np.array_equal(RC.epilogue(RC.EPI_MULT, c[:, 1:2], est=e[:, 1:2]), [[1.0]])
    assert np.array_equal(RC.epilogue(RC.EPI_GRAD, c[:, 1:2], est=e[:, 1:2], dt=0.25), [[0.75]])
    assert np.array_equal(RC.epilogue(RC.EPI_MULT_REG, c[:, 1:2], est=e[:, 1:2], w=w[:, 1:2], rlam=1.0), [[2.0]])
    assert np.array_equal(RC.epilogue(RC.EPI_GRAD_REG, c[:, 1:2], est=e[:, 1:2], w=w[:, 1:2], rlam=1.0, dt=0.25),
                          [[0.875]])
    t = RC.epilogue(RC.EPI_TAPER, c[:, 1:2], x=f[:, 1:2], wy=[0.5], wx=[0.5])
    assert np.array_equal(t, [[0.25 * 3.0 + 0.75 * 2.0]])
    assert RC.stop_measure([[1.0, 3.0]], [[2.0, 2.0]]) == 1.0
    assert RC.ulp_diff(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])) == 1

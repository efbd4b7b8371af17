"""TEST INFRASTRUCTURE ONLY -- references of the Richardson-Lucy kernels taken
alone (sgpu_rl_conv_device / sgpu_rl_reg_device, include/sirilgpu.h):

  conv_exact     the convolution as ConvArgs::taps defines it (rl_conv.h),
                 summed tap by tap; exact for integer inputs
  conv_f32_fft   the same circular convolution the way rl_fft.hip documents
                 it, in single precision with scipy.fft: an independent
                 implementation of the same mathematics, the yardstick of the
                 FFT path's rounding error
  epilogue       float32 restatements of rl_epilogue's eight point-wise steps
  stop_measure   the stop sum from an output the GPU produced

and the inputs and case lists that tests/test_rl_conv_ref.py (CPU) and
tests/test_rl_conv_gpu.py (GPU) share.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
EPI_STORE, EPI_RATIO, EPI_RATIO_NAIVE, EPI_MULT, EPI_GRAD, EPI_TAPER, EPI_MULT_REG, EPI_GRAD_REG = range(8)
FFT_MAX_LEN = 8192


# ------------------------------------------------------------- convolutions
def conv_exact(x, k, wrap):
    """c[y][x] = sum_{ky,kx} k[ky][kx] * x[y + h - ky][x + h - kx], h = ks // 2:
    indices modulo the image (wrap) or zero outside.  int64 for integer
    inputs, float64 otherwise.  The circular form handles ks > n: np.roll
    reduces every shift modulo n, so aliasing taps add up."""
    x = np.asarray(x)
    k = np.asarray(k)
    integer = np.issubdtype(x.dtype, np.integer) and np.issubdtype(k.dtype, np.integer)
    dt = np.int64 if integer else np.float64
    x = x.astype(dt)
    k = k.astype(dt)
    ks = k.shape[0]
    assert k.shape == (ks, ks) and ks % 2 == 1
    h = ks // 2
    H, W = x.shape
    out = np.zeros((H, W), dt)
    if wrap:
        for ky in range(ks):
            for kx in range(ks):
                if k[ky, kx] != 0:
                    out += k[ky, kx] * np.roll(x, (ky - h, kx - h), axis=(0, 1))
        return out
    xp = np.zeros((H + 2 * h, W + 2 * h), dt)
    xp[h:h + H, h:h + W] = x
    for ky in range(ks):
        for kx in range(ks):
            if k[ky, kx] != 0:
                out += k[ky, kx] * xp[2 * h - ky:2 * h - ky + H, 2 * h - kx:2 * h - kx + W]
    return out


def fft_smooth_len(need):
    """Smallest even 2-3-5-smooth length >= need, 0 when none is <= 8192
    (fft_smooth_len of rl_fft.hip, restated)."""
    m = need + (need & 1)
    while m <= FFT_MAX_LEN:
        t = m
        for p in (2, 3, 5):
            while t % p == 0:
                t //= p
        if t == 1:
            return m
        m += 2
    return 0


def conv_f32_fft(x, k):
    """Circular convolution of x with k in single precision, as rl_fft.hip
    documents it: the periodic extension of x by h on every side, zero-padded
    to the smooth lengths n2 x n1 >= (H + 3h) x (W + 3h); the taps wrapped
    around (0, 0); rfft2, product, irfft2 (complex64 throughout); the window
    [h, h + H) x [h, h + W)."""
    import scipy.fft as sf
    x = np.asarray(x, F32)
    k = np.asarray(k, F32)
    H, W = x.shape
    ks = k.shape[0]
    h = ks // 2
    assert min(H, W) >= h + 1
    n1, n2 = fft_smooth_len(W + 3 * h), fft_smooth_len(H + 3 * h)
    assert n1 and n2
    ext = np.zeros((n2, n1), F32)
    ys = (np.arange(H + 2 * h) - h) % H
    xs = (np.arange(W + 2 * h) - h) % W
    ext[:H + 2 * h, :W + 2 * h] = x[np.ix_(ys, xs)]
    kp = np.zeros((n2, n1), F32)
    for ky in range(ks):
        for kx in range(ks):
            kp[(ky - h) % n2, (kx - h) % n1] = k[ky, kx]
    X = sf.rfft2(ext)
    K = sf.rfft2(kp)
    assert X.dtype == np.complex64 and K.dtype == np.complex64
    y = sf.irfft2(X * K, s=(n2, n1))
    assert y.dtype == np.float32
    return y[h:h + H, h:h + W].copy()


# ---------------------------------------------------------------- epilogues
def epilogue(epi, c, x=None, f=None, est=None, w=None, wy=None, wx=None, dt=0.0, rlam=0.0):
    """rl_epilogue (rl_conv.h) on the float32 convolution output c, op for op
    in float32 (EPI_TAPER's blend in double, as written there).  x is the
    convolved image (EPI_TAPER's `in`)."""
    c = np.asarray(c, F32)
    dt, rlam = F32(dt), F32(rlam)
    one = F32(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if epi == EPI_STORE:
            return c.copy()
        if epi == EPI_RATIO:
            d = np.where(np.isnan(c) | (c == 0), F32(1e-9), c).astype(F32)
            return (np.asarray(f, F32) / d).astype(F32)
        if epi == EPI_RATIO_NAIVE:
            q = (np.asarray(f, F32) / c).astype(F32)
            return np.where(F32(1e-9) < q, q, F32(1e-9)).astype(F32)
        if epi == EPI_TAPER:
            wt = (np.asarray(wy, F32)[:, None] * np.asarray(wx, F32)[None, :]).astype(F32)
            a = (wt * np.asarray(x, F32)).astype(F32)
            return (a.astype(np.float64) + (1.0 - wt.astype(np.float64)) * c.astype(np.float64)).astype(F32)
        e = np.asarray(est, F32)
        if epi == EPI_MULT:
            return (c * e).astype(F32)
        if epi == EPI_GRAD:
            return (e + dt * (-one + c)).astype(F32)
        rw = (rlam * np.asarray(w, F32)).astype(F32)
        if epi == EPI_MULT_REG:
            return ((c * e) * (one / (one - rw))).astype(F32)
        if epi == EPI_GRAD_REG:
            return (e + dt * ((-one + rw) + c)).astype(F32)
    raise ValueError(epi)


def stop_measure(out, ref):
    """sum |out - ref| / |ref|: each term formed in float32, summed in float64."""
    out, ref = np.asarray(out, F32), np.asarray(ref, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.abs(out - ref) / np.abs(ref)).astype(F32)
    return float(t.astype(np.float64).sum())


def ulp_diff(a, b):
    """Largest distance in units of the last place between two float32 arrays
    (finite values; +0 and -0 count as equal)."""
    a = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max()) if a.size else 0


# ------------------------------------------------------------------- inputs
def int_image(H, W, seed=0):
    """Integers uniform in [-8, 8]."""
    return np.random.default_rng([H, W, seed]).integers(-8, 9, (H, W)).astype(np.int64)


def int_taps(ks, seed=0):
    """Integers uniform in [-4, 4] with no symmetry: with the image in [-8, 8]
    every partial sum stays below 101^2 * 32 = 326 432 < 2^24, so the result
    is an integer float32 holds exactly in any summation order."""
    rng = np.random.default_rng([ks, seed, 77])
    while True:
        k = rng.integers(-4, 5, (ks, ks)).astype(np.int64)
        if ks == 1:
            k[0, 0] = 3
            return k
        if not (np.array_equal(k, k[::-1]) or np.array_equal(k, k[:, ::-1]) or np.array_equal(k, k[::-1, ::-1])
                or np.array_equal(k, k.T)):
            return k


def moffat_taps(ks):
    """An elliptical, off-centre Moffat profile (float32, sum 1)."""
    r = ks // 2
    y, x = np.mgrid[-r:ks - r, -r:ks - r].astype(np.float64)
    x, y = x - 0.7, y + 0.4
    ca, sa = np.cos(0.5), np.sin(0.5)
    xr, yr = ca * x + sa * y, (-sa * x + ca * y) * 1.4
    k = (1.0 + (xr * xr + yr * yr) / 9.0) ** (-4.5)
    return (k / k.sum()).astype(F32)


def float_image(H, W, seed=0):
    """Uniform [0, 1) float32."""
    return np.random.default_rng([H, W, seed, 5]).random((H, W), dtype=F32)


# -------------------------------------------------------------------- cases
# FFT path, (H, W, ks).  ks = 3 makes the FFT length n + 3: the lengths 16
# (8.2), 128 (8.8.2), 512 (8.8.8: one butterfly per thread), 250 (5.5.5.2),
# 162 (3^4.2), 486, 360, 600 and 1080 (more than one butterfly per thread) and
# 8192, each once as the row and once as the column length; every H here is
# odd (the last row pair holds one row).
_L3 = [(13, 125), (125, 13), (509, 247), (247, 509), (159, 483), (483, 159), (357, 597), (597, 357),
       (1077, 13), (13, 1077), (13, 8189), (8189, 13)]
FFT_CASES = [(H, W, 3) for H, W in _L3]
# larger PSFs at two plain shapes and at the thin slice (hk + 1, 3 hk), both orientations
for _ks in (15, 31, 63):
    _h = _ks // 2
    for _H, _W in ((65, 200), (97, 101), (_h + 1, 3 * _h)):
        FFT_CASES += [(_H, _W, _ks), (_W, _H, _ks)]

FLOAT_CASE = (65, 129, 31)   # the one float case of either path: (H, W, ks)

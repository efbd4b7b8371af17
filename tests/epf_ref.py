"""The guided filter of DESIGN.md 6n (E0, E1, E3, E4) restated in numpy float64
with the operation order of siril_amd/csrc/epf_host.h: the contract the kernels
(siril_amd/csrc/epf.hip) and the shared header are held to, bit for bit.  The
widening is tests/stretch_ref.py's `widen`, the modulation
tests/median_ref.py's.  The bilateral filter (E2, mode 0) is not built and is
refused.  numpy does not contract and every elementwise
operation below is rounded once.  Parity with Siril (OpenCV) is unpinned."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_ref as MR  # noqa: E402
from stretch_ref import widen  # noqa: E402

F = np.float32
BILATERAL, GUIDED = 0, 1
MIN_D, MAX_D = 3, 25


def window(d, ss):
    """E1: d itself, or for d = 0 OpenCV's 2 round(1.5 ss) + 1, clamped to 3 .. 25."""
    if d != 0:
        return d
    rd = np.floor(1.5 * float(ss) + 0.5)
    return 2 * int(min(max(rd, 1.0), 12.0)) + 1


def check(w, h, mode, d, si, ss, modulation=1.0):
    """None, or why the filter is refused (E6)."""
    if w < 1 or h < 1:
        return "empty"
    if w > 65535 or h > 65535:
        return "too large"
    if mode != GUIDED:
        return "mode"
    if not (np.isfinite(si) and si > 0.0):
        return "si"
    if d == 0 and not (np.isfinite(ss) and ss > 0.0):
        return "ss"
    if d != 0 and (d % 2 == 0 or not MIN_D <= d <= MAX_D):
        return "d"
    if (window(d, ss) - 1) // 2 > min(w, h) - 1:
        return "too small"
    if not (np.isfinite(modulation) and 0.0 <= modulation <= 1.0):
        return "modulation"
    return None


def centre(x):
    """E4's x: the sample rounded to float32 once (a float sample is itself, bits kept)."""
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return widen(x).astype(F)
    return x.astype(F, copy=False)


def _pad(v, r):
    return np.pad(v, [(0, 0)] * (v.ndim - 2) + [(r, r), (r, r)], mode="reflect")


def box(f, r):
    """E3's box of float64 planes: row sums left to right, the rows top to bottom, times 1 / (d d)."""
    d = 2 * r + 1
    h, w = f.shape[-2:]
    pad = _pad(f, r)
    with np.errstate(all="ignore"):
        rows = pad[..., :, 0:w].copy()
        for dx in range(1, d):
            rows = rows + pad[..., :, dx:dx + w]
        col = rows[..., 0:h, :].copy()
        for dy in range(1, d):
            col = col + rows[..., dy:dy + h, :]
        return col * (1.0 / float(d * d))


def guided(x, guide, d, si):
    """E3 of planes [..., H, W]; guide None: the input guides itself.  float32 m."""
    r = (d - 1) // 2
    p = widen(x)
    I = p if guide is None else widen(guide)
    eps = si * si
    with np.errstate(all="ignore"):
        mI, mp, cII, cIp = box(I, r), box(p, r), box(I * I, r), box(I * p, r)
        var = cII - mI * mI
        cov = cIp - mI * mp
        a = cov / (var + eps)
        b = mp - a * mI
        a, b = a.astype(F), b.astype(F)
        return (box(a.astype(np.float64), r) * I + box(b.astype(np.float64), r)).astype(F)


def epf(x, d=0, si=0.02, ss=3.0, modulation=1.0, mode=GUIDED, guide=None):
    """E0, E1, E3, E4: [..., H, W] float32 or uint16 -> float32."""
    x = np.asarray(x)
    assert check(x.shape[-1], x.shape[-2], mode, d, si, ss, modulation) is None
    assert guide is None or guide.shape == x.shape
    d = window(d, ss)
    m = guided(x, guide, d, si)
    return MR.modulate(modulation, m, centre(x))


def same(got, want):
    """NaN at the same places, every other sample equal as uint32."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])

"""TEST INFRASTRUCTURE: numpy restatement of the calibration specification
(DESIGN.md "Calibration", S1-S7), the reference the GPU kernels are compared
with bit for bit.  Float operations are float32 numpy operations (one rounding
each); the sequential double sums use np.add.accumulate, never np.sum (whose
pairwise order differs).  Parity with a Siril binary is unpinned."""
import math

import numpy as np

INV = np.float32(1.0) / np.float32(65535.0)
GR = (math.sqrt(5.0) - 1.0) / 2.0
COLD, HOT = 0, 1


# ---- S1 -----------------------------------------------------------------------
def to_float(a):
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return a.astype(np.float32) * INV
    assert a.dtype == np.float32
    return a


# ---- S2 -----------------------------------------------------------------------
def apply_bias(x, bias=None, level=None):
    if bias is not None:
        return x - bias
    if level is not None:
        return x - np.float32(level)
    return x


def s2(frame, bias=None, level=None, dark=None, k=1.0, flat=None, norm=1.0):
    """One frame ([H, W] uint16 or float32) -> float32."""
    with np.errstate(all="ignore"):
        x = apply_bias(to_float(frame), bias, level)
        if dark is not None:
            t = np.float32(k) * dark
            x = x - t
        if flat is not None:
            q = x / flat
            x = np.where(flat == 0, np.float32(0), np.float32(norm) * q).astype(np.float32)
    assert x.dtype == np.float32
    return x


# ---- S4 -----------------------------------------------------------------------
def _seq_sum(a, axis):
    if a.shape[axis] == 0:
        return np.zeros(a.shape[:axis] + a.shape[axis + 1:], np.float64)
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def region_stats(plane, x0=0, y0=0, x1=None, y1=None, step=1):
    """(n, mean, sigma): rows left to right, then rows top to bottom."""
    reg = np.asarray(plane, np.float32)[y0:y1:step, x0:x1:step].astype(np.float64)
    ok = (reg != 0) & ~np.isnan(reg)
    v = np.where(ok, reg, 0.0)
    n = int(ok.sum())
    s = float(_seq_sum(_seq_sum(v, 1), 0))
    q = float(_seq_sum(_seq_sum(v * v, 1), 0))
    if n == 0:
        return 0, 0.0, 0.0
    mean = s / n
    var = q / n - mean * mean
    return n, mean, (math.sqrt(var) if n > 1 and var > 0 else 0.0)


# ---- S3 -----------------------------------------------------------------------
def optim_area(w, h):
    if w > 512 and h > 512:
        return (w - 512) // 2, (h - 512) // 2, 512, 512
    return 0, 0, w, h


def dark_optimize(frame, dark, bias=None, level=None, count=None):
    """k_f (np.float32) of one frame; count: a list that receives the number
    of noise evaluations."""
    h, w = dark.shape
    ax, ay, aw, ah = optim_area(w, h)
    sl = (slice(ay, ay + ah), slice(ax, ax + aw))
    xb = apply_bias(to_float(frame), bias, level)[sl]
    dk = dark[sl]
    evals = [0]

    def noise(k):
        evals[0] += 1
        return region_stats(xb - np.float32(k) * dk)[2]

    a, b = np.float32(0), np.float32(2)
    c = np.float32(float(b) - GR * (float(b) - float(a)))
    d = np.float32(float(a) + GR * (float(b) - float(a)))
    fc, fd = noise(c), noise(d)
    while abs(float(c) - float(d)) > 1e-3:
        if fc < fd:
            b, d, fd = d, c, fc
            c = np.float32(float(b) - GR * (float(b) - float(a)))
            fc = noise(c)
        else:
            a, c, fc = c, d, fd
            d = np.float32(float(a) + GR * (float(b) - float(a)))
            fd = noise(d)
    if count is not None:
        count.append(evals[0])
    return (a + b) * np.float32(0.5)


# ---- S5 -----------------------------------------------------------------------
def equalize_cfa(flat):
    """(new plane, green diagonal 0 | 1, c1, c2) of a Bayer flat."""
    flat = np.asarray(flat, np.float32)
    h, w = flat.shape
    x0, x1, y0, y1 = (w // 3) & ~1, (2 * w // 3) & ~1, (h // 3) & ~1, (2 * h // 3) & ~1
    with np.errstate(all="ignore"):
        m = [np.float64(region_stats(flat, min(x0 + (s & 1), x1), min(y0 + (s >> 1), y1), x1, y1, 2)[1])
             for s in range(4)]
        if abs(1 - m[0] / m[3]) < abs(1 - m[1] / m[2]):
            diag, s1, c1, s2_, c2 = 0, 1, np.float32(m[0] / m[1]), 2, np.float32(m[0] / m[2])
        else:
            diag, s1, c1, s2_, c2 = 1, 0, np.float32(m[1] / m[0]), 3, np.float32(m[1] / m[3])
        out = flat.copy()
        for s, c in ((s1, c1), (s2_, c2)):
            out[s >> 1::2, s & 1::2] = flat[s >> 1::2, s & 1::2] * c
    return out, diag, c1, c2


def flat_norm(flat):
    return np.float32(region_stats(flat)[1])


# ---- S6 -----------------------------------------------------------------------
def find_deviant(dark, cold, hot):
    """(list int32 [n, 2] of (y*W + x, type), (median, sigma, thresHot, thresCold))."""
    from oracle import oracle as O
    dark = np.asarray(dark, np.float32)
    median = O.norm_stats(dark, lite=True)[1]
    sigma = region_stats(dark)[2]
    th, tc = np.float32(median + hot * sigma), np.float32(median - cold * sigma)
    with np.errstate(invalid="ignore"):
        hotm = (dark >= th) if hot != -1 else np.zeros(dark.shape, bool)
        coldm = (~hotm & (dark < tc)) if cold != -1 else np.zeros(dark.shape, bool)
    pos = np.flatnonzero(hotm | coldm)
    lst = np.stack([pos, np.where(hotm.ravel()[pos], HOT, COLD)], 1).astype(np.int32).reshape(-1, 2)
    return lst, (float(median), float(sigma), float(th), float(tc))


# ---- S7 -----------------------------------------------------------------------
def cosmetic(frame, lst, cfa=False):
    """Sequential in place on a copy: entry i sees what entries 0..i-1 left."""
    from oracle import oracle as O
    img = np.array(frame, np.float32)
    h, w = img.shape
    step = 2 if cfa else 1
    for pos, typ in np.asarray(lst).reshape(-1, 2):
        y, x = divmod(int(pos), w)
        r = 1 if typ == HOT else 2
        vals = [img[y + dy * step, x + dx * step]
                for dy in range(-r, r + 1) for dx in range(-r, r + 1)
                if (dx or dy) and 0 <= y + dy * step < h and 0 <= x + dx * step < w]
        if not vals:
            continue
        if typ == HOT:
            s = 0.0
            for v in vals:
                s += float(v)
            img[y, x] = np.float32(s / len(vals))
        else:
            img[y, x] = np.float32(O.quickmedian(vals))
    return img


# ---- everything ---------------------------------------------------------------
def calibrate(frames, bias=None, level=None, dark=None, flat=None, norm=1.0, dark_optim=False, deviant=None,
              cfa=False, k=None):
    """[N, H, W] -> (float32 [N, H, W], k float32 [N])."""
    out, ks = [], []
    for f, fr in enumerate(frames):
        kf = np.float32(1) if k is None else np.float32(k[f])
        if dark_optim:
            kf = dark_optimize(fr, dark, bias, level)
        x = s2(fr, bias, level, dark, kf, flat, norm)
        if deviant is not None and len(deviant):
            x = cosmetic(x, deviant, cfa)
        out.append(x)
        ks.append(kf)
    return np.stack(out), np.array(ks, np.float32)


# ---- synthetic case of the dark optimisation -----------------------------------
def synth_optim_case(w=97, h=53, k_true=(0.6, 1.0, 1.45), seed=3, dtype=np.uint16):
    """Frames 2000 + k_true * dark + N(0, 30) ADU over a gamma(2, 200) ADU dark
    with 1 % of its pixels at 30000 (shared with the GPU tests)."""
    rng = np.random.default_rng(seed)
    dark = rng.gamma(2.0, 200.0, (h, w))
    dark[rng.random((h, w)) < 0.01] = 30000.0
    frames = np.stack([2000.0 + k * dark + rng.normal(0.0, 30.0, (h, w)) for k in k_true])
    frames = np.clip(np.rint(frames), 0, 65535).astype(np.uint16)
    dark16 = np.clip(np.rint(dark), 0, 65535).astype(np.uint16)
    if dtype == np.float32:
        frames = to_float(frames)
    return frames, to_float(dark16)

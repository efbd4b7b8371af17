"""The median filter of DESIGN.md 6l (M0-M5) restated in numpy.  A median is a
selection: the output is one of the window's samples with its own bits, so
everything built on this file compares bit for bit.  This restatement is the
contract the kernels (siril_amd/csrc/median.hip) and the shared header
(median_host.h) are held to."""
import numpy as np

F = np.float32
INV_USHRT = F(1.0) / F(65535.0)


def to_float(a):
    """M0: WORD samples scale by 1/65535, float samples pass."""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return a.astype(F) * INV_USHRT
    return a.astype(F, copy=False)


def check(w, h, ksize, modulation=1.0, iterations=1):
    """None, or why the filter is refused (M5)."""
    if ksize % 2 == 0 or not 3 <= ksize <= 15:
        return "ksize"
    if (ksize - 1) // 2 > min(w, h) - 1:
        return "too small"
    if not (np.isfinite(modulation) and 0.0 <= modulation <= 1.0):
        return "modulation"
    if not 1 <= iterations <= 8:
        return "iterations"
    if w > 65535 or h > 65535:
        return "too large"
    return None


def key(a):
    """M2: uint32 keys whose unsigned order is -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN."""
    b = np.ascontiguousarray(a, F).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F)


def median(y, ksize):
    """M1, M2 of float32 planes [..., H, W]: the sample of rank (ksize^2 - 1)/2 of every window, its bits kept."""
    r = (ksize - 1) // 2
    h, w = y.shape[-2:]
    k = np.pad(key(y), [(0, 0)] * (y.ndim - 2) + [(r, r), (r, r)], mode="reflect")
    views = np.stack([k[..., dy:dy + h, dx:dx + w] for dy in range(ksize) for dx in range(ksize)], axis=-1)
    views.sort(axis=-1)
    return unkey(views[..., (ksize * ksize - 1) // 2])


def modulate(modulation, m, x):
    """M3, float32 step by step."""
    mod = F(modulation)
    if mod == F(1.0):
        return m
    with np.errstate(invalid="ignore", over="ignore"):
        keep = F(1.0) - mod
        a = mod * m
        b = keep * x
        return (a + b).astype(F, copy=False)


def fmedian(x, ksize, modulation=1.0, iterations=1):
    """M0-M4: [..., H, W] float32 or uint16 -> float32."""
    y = to_float(x)
    assert check(y.shape[-1], y.shape[-2], ksize, modulation, iterations) is None
    for _ in range(iterations):
        y = modulate(modulation, median(y, ksize), y)
    return y


def same(a, b, payload=True):
    """Bit for bit.  payload=False: NaN at the same places, every other sample equal as uint32 (an arithmetic
    result's NaN payload is not specified)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    if payload:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def scene(h, w, seed=0, word=False):
    """A deterministic test plane: a gradient, a texture, and salt and pepper."""
    rng = np.random.RandomState(2000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.2 + 0.3 * x / max(w - 1, 1) + 0.1 * y / max(h - 1, 1) + 0.05 * rng.rand(h, w)
    n = max(4, h * w // 50)
    v[rng.randint(h, size=n), rng.randint(w, size=n)] = rng.choice([0.0, 0.95], size=n)
    if word:
        return np.round(v * 65535.0 * 0.9).astype(np.uint16)
    return v.astype(F)

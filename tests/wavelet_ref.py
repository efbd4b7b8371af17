"""The a trous wavelet arithmetic of DESIGN.md 6j (W0-W5) restated in numpy:
float32 throughout, one rounding per operation (numpy never contracts a
multiply and an add).  This restatement is the contract the kernels
(siril_amd/csrc/wavelet.hip) and the shared header (wavelet_host.h) are held
to, bit for bit."""
import numpy as np

F = np.float32
INV_USHRT = F(1.0) / F(65535.0)


def to_float(a):
    """W0: WORD samples scale by 1/65535, float samples pass."""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return a.astype(F) * INV_USHRT
    return a.astype(F, copy=False)


def reach(n, type=2):
    """W1: the largest offset a tap of an n-layer transform uses."""
    return 0 if n <= 1 else (2 if type == 2 else 1) << (n - 2)


def check(w, h, n, type=2):
    """None, or why the transform is refused."""
    if not 1 <= n <= 6:
        return "nbr_layers"
    if type not in (1, 2):
        return "type"
    if reach(n, type) > min(w, h) - 1:
        return "too small"
    return None


def refl(i, n):
    """W1, on an index array, applied once."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def _smooth_axis(a, s, type, axis):
    n = a.shape[axis]
    i = np.arange(n)

    def tap(d):
        return np.take(a, refl(i + d, n), axis=axis)

    if type == 2:
        outer = (tap(-2 * s) + tap(2 * s)) * F(1.0 / 16.0)
        inner = (tap(-s) + tap(s)) * F(1.0 / 4.0)
        return (outer + inner) + a * F(3.0 / 8.0)
    return (tap(-s) + tap(s)) * F(1.0 / 4.0) + a * F(1.0 / 2.0)


def smooth(c, s, type=2):
    """W2: rows first, then columns of the row result; the last two axes are (H, W)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _smooth_axis(_smooth_axis(c, s, type, -1), s, type, -2)


def transform(x, n, type=2):
    """W3: [..., H, W] -> [..., n, H, W], the details w_0 .. w_{n-2} and the residual."""
    c = to_float(x)
    assert check(c.shape[-1], c.shape[-2], n, type) is None
    planes = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n - 1):
            nxt = smooth(c, 1 << j, type)
            planes.append(c - nxt)
            c = nxt
    planes.append(c)
    return np.stack(planes, axis=-3).astype(F, copy=False)


def reconstruct(planes, coefs):
    """W4: [..., n, H, W] and n coefficients -> [..., H, W]."""
    k = np.asarray(coefs, F).reshape(-1)
    n = planes.shape[-3]
    assert len(k) == n
    with np.errstate(invalid="ignore", over="ignore"):
        acc = k[0] * planes[..., 0, :, :]
        for j in range(1, n):
            acc = acc + k[j] * planes[..., j, :, :]
    return acc.astype(F, copy=False)


def wrecons(x, coefs, type=2):
    """W5: the fused form is W4 of W3, bit for bit."""
    return reconstruct(transform(x, len(np.asarray(coefs).reshape(-1)), type), coefs)


def taps(type, s):
    """The dilated 1-D filter as a dense vector of length 2*R*s + 1."""
    t = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16] if type == 2 else [1 / 4, 1 / 2, 1 / 4]
    v = np.zeros((len(t) - 1) * s + 1, F)
    v[::s] = t
    return v


def scene(h, w, seed=0, word=False):
    """A deterministic test plane: a gradient, a texture and a few bright points."""
    rng = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.2 + 0.3 * x / max(w - 1, 1) + 0.1 * y / max(h - 1, 1) + 0.05 * rng.rand(h, w)
    for _ in range(6):
        v[rng.randint(h), rng.randint(w)] += 0.4
    if word:
        return np.round(v * 65535.0 * 0.9).astype(np.uint16)
    return v.astype(F)

"""Restatement of the thin-plate-spline background extraction (DESIGN.md 6k,
R0-R7) in numpy / Python float64 with the operation order of
siril_amd/csrc/bkg_rbf_host.h: the contract the kernels of
siril_amd/csrc/background_rbf.hip and the host functions are compared with.
B0-B3 and B7 are tests/bkg_ref.py's.  numpy does not contract, every
elementwise operation below is rounded once, and the sequential sums are
np.add.accumulate (strictly left to right).  Parity with a Siril binary is
unpinned."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402

MAX_SAMPLES = 1024
SQRT2 = 1.4142135623730951
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
_C = [1.0 / float(2 * k + 1) for k in range(10)]


def check(w, h, samples, tolerance, smooth):
    """R0 -> the grid; ValueError for the refusals."""
    g = BR.grid(w, h, samples)
    if g["K"] > MAX_SAMPLES:
        raise ValueError("more than 1024 sample boxes")
    if not (tolerance >= 0 and math.isfinite(tolerance)):
        raise ValueError("tolerance must be finite and >= 0")
    if not (smooth >= 0.0 and smooth <= 1.0):
        raise ValueError("smooth must be in [0, 1]")
    return g


def axes(w, h):
    """R1 -> (x0, y0, a)."""
    x0, y0 = float(w - 1) * 0.5, float(h - 1) * 0.5
    return x0, y0, 1.0 / max(x0, y0)


def rbf_log(s):
    """R2's logarithm of positive normal doubles (any shape)."""
    s = np.ascontiguousarray(s, np.float64)
    b = s.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    z = (m - 1.0) / (m + 1.0)
    z2 = z * z
    p = np.full(s.shape, _C[9])
    for k in range(8, -1, -1):
        p = p * z2
        p = p + _C[k]
    r = (2.0 * z) * p
    ed = e.astype(np.float64)
    return (ed * LN2_LO + r) + ed * LN2_HI


def phi(s):
    s = np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        return np.where(s == 0.0, 0.0, (0.5 * s) * rbf_log(s))


def lam_rel(smooth):
    return 1e-4 * math.pow(10.0, 3.0 * (smooth - 0.5))


def samples(med, keep, g, w, h):
    """R0 + R1 -> (u, v, z) of the kept boxes in ascending k, and their pixel centres."""
    x0, y0, a = axes(w, h)
    cx, cy = BR.centres(g)
    ks = [k for k in range(g["K"]) if keep[k]]
    px = np.array([cx[k % g["nx"]] for k in ks], np.int64)
    py = np.array([cy[k // g["nx"]] for k in ks], np.int64)
    u = (px.astype(np.float64) - x0) * a
    v = (py.astype(np.float64) - y0) * a
    z = np.array([float(med[k]) for k in ks], np.float64)
    return u, v, z, px, py


def system(u, v, z, lam_rel_value):
    """R3 -> (aug float64[n+1, n+2], mean_abs, lambda)."""
    n = len(z)
    du = u[:, None] - u[None, :]
    dv = v[:, None] - v[None, :]
    P = phi(du * du + dv * dv)
    total = np.add.accumulate(np.abs(P).ravel())[-1]
    mean_abs = total / (float(n) * float(n))
    lam = lam_rel_value * mean_abs
    aug = np.zeros((n + 1, n + 2), np.float64)
    aug[:n, :n] = P
    idx = np.arange(n)
    aug[idx, idx] = aug[idx, idx] + lam
    aug[:n, n] = 1.0
    aug[n, :n] = 1.0
    aug[:n, n + 1] = z
    return aug, float(mean_abs), float(lam)


def pivot_key(col):
    return np.ascontiguousarray(col, np.float64).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


def lu_solve(aug, tie_last=False):
    """R4 on [A | rhs] (order N, N + 1 columns; a copy is worked on) -> (status 0 | 2, x float64[N]);
    x is +0 when the status is 2.  tie_last: the wrong tie rule (the highest row among equal pivots), for
    the tests that show a system tells the two apart."""
    a = np.array(aug, np.float64)
    N = a.shape[0]
    assert a.shape == (N, N + 1)
    with np.errstate(all="ignore"):
        for k in range(N):
            key = pivot_key(a[k:, k])
            p = k + int(np.argmax(key))         # the first of the largest
            if tie_last:
                p = k + len(key) - 1 - int(np.argmax(key[::-1]))
            kp = int(key[p - k])
            if kp == 0 or kp >= 0x7FF0000000000000:
                return 2, np.zeros(N, np.float64)
            if p != k:
                a[[k, p], k:] = a[[p, k], k:]
            if k + 1 < N:
                l = a[k + 1:, k] / a[k, k]
                t = l[:, None] * a[k, k + 1:][None, :]
                a[k + 1:, k + 1:] = a[k + 1:, k + 1:] - t
        x = np.zeros(N, np.float64)
        b = a[:, N].copy()
        for i in range(N - 1, -1, -1):
            x[i] = b[i] / a[i, i]
            b[:i] = b[:i] - a[:i, i] * x[i]
    return 0, x


def fit(med, keep, g, w, h, lam_rel_value, descending=False):
    """R0-R5 of one plane -> dict(n, status, x float64[n+1], mean, mean_abs, lam, u, v, px, py).
    descending: the same system with the samples in the opposite order (the rounding floor of the solve)."""
    u, v, z, px, py = samples(med, keep, g, w, h)
    n = len(z)
    if n == 0:
        return dict(n=0, status=1, x=np.zeros(1), mean=0.0, mean_abs=0.0, lam=0.0, u=u, v=v, px=px, py=py)
    if descending:
        aug, mean_abs, lam = system(u[::-1], v[::-1], z[::-1], lam_rel_value)
    else:
        aug, mean_abs, lam = system(u, v, z, lam_rel_value)
    st, x = lu_solve(aug)
    if descending:
        x = np.concatenate([x[:n][::-1], x[n:]])
    mean = 0.0 if st else float(np.add.accumulate(z)[-1] / float(n))
    return dict(n=n, status=st, x=x, mean=mean, mean_abs=mean_abs, lam=lam, u=u, v=v, px=px, py=py, aug=aug)


def weights_row(f):
    """The d_weights row of a plane: the weights, the constant, then +0 up to MAX_SAMPLES + 1."""
    row = np.zeros(MAX_SAMPLES + 1, np.float64)
    if f["status"] == 0:
        row[:f["n"] + 1] = f["x"]
    return row


def background(x, u, v, w, h):
    """R6: float64[h, w] from the weights followed by the constant."""
    x0, y0, a = axes(w, h)
    pu = ((np.arange(w, dtype=np.float64) - x0) * a)[None, :]
    pv = ((np.arange(h, dtype=np.float64) - y0) * a)[:, None]
    acc = np.zeros((h, w), np.float64)
    n = len(u)
    for i in range(n):
        du = pu - u[i]
        dv = pv - v[i]
        acc = acc + x[i] * phi(du * du + dv * dv)
    return acc + x[n]


def correct(plane, b, mean, status=0, divide=False):
    """R7 (B7) of one plane -> float32[h, w]."""
    xf = BR.to_float(plane)
    if status:
        return xf.copy()
    xd = xf.astype(np.float64)
    with np.errstate(all="ignore"):
        if divide:
            return np.where(b == 0.0, np.float32(0.0), ((xd / b) * np.float64(mean)).astype(np.float32)).astype(np.float32)
        return ((xd - b) + np.float64(mean)).astype(np.float32)


def subsky_rbf_plane(plane, samples_per_line=20, tolerance=1.0, smooth=0.5, divide=False, lam_rel_value=None):
    """R0-R7 of one plane -> (out float32, info dict).  lam_rel_value: the double the library returned
    (its own pow), else this module's."""
    h, w = plane.shape
    g = check(w, h, samples_per_line, tolerance, smooth)
    med = BR.box_medians(plane, g)
    keep, kept, T, m, mad = BR.select(med, tolerance)
    lr = lam_rel(smooth) if lam_rel_value is None else float(lam_rel_value)
    f = fit(med, keep, g, w, h, lr)
    b = None if f["status"] else background(f["x"], f["u"], f["v"], w, h)
    out = correct(plane, b, f["mean"], f["status"], divide)
    return out, dict(med=med, keep=keep, kept=kept, fit=f, bkg=b, weights=weights_row(f), mean=f["mean"],
                     status=f["status"], grid=g, lam_rel=lr)

"""Restatement of the polynomial background extraction
in numpy / Python float64: the contract the kernels of
siril_amd/csrc/background.hip and the host functions of bkg_host.h are compared
with.  Python floats are IEEE doubles and every sum below is an explicit
sequential loop; B6 is numpy float64 in the stated Horner order (numpy does not
contract).  Parity with a Siril binary is unpinned."""
import math

import numpy as np

BOX, R, NS, RANK = 25, 12, 625, 312
MAX_K = 8192
INV = np.float32(1.0) / np.float32(65535.0)
TERMS = [(n - j, j) for n in range(5) for j in range(n + 1)]       # (i, j) of u^i v^j


def ncoef(d):
    return (d + 1) * (d + 2) // 2


def to_float(plane):
    """B0: WORD -> (float)v * INV; float32 as it is."""
    a = np.asarray(plane)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    if a.dtype == np.uint16:
        return a.astype(np.float32) * INV
    assert a.dtype == np.float32
    return a


def grid(w, h, samples):
    """B1 -> dict(nx, ny, dist, startx, starty, K); ValueError for its refusals."""
    if w < BOX or h < BOX:
        raise ValueError("the frame is smaller than one sample box")
    if samples < 1:
        raise ValueError("samples < 1")
    dist = w // samples
    if dist < 1:
        raise ValueError("more samples per line than pixels")
    nx, ny = (w - BOX) // dist + 1, (h - BOX) // dist + 1
    if nx * ny > MAX_K:
        raise ValueError("more than 8192 sample boxes")
    return dict(nx=nx, ny=ny, dist=dist, startx=((w - BOX) % dist) // 2, starty=((h - BOX) % dist) // 2, K=nx * ny)


def check_params(degree, tolerance):
    if degree not in (1, 2, 3, 4):
        raise ValueError("degree must be 1 .. 4")
    if not (tolerance >= 0 and math.isfinite(tolerance)):
        raise ValueError("tolerance must be finite and >= 0")


def centres(g):
    cx = [R + g["startx"] + i * g["dist"] for i in range(g["nx"])]
    cy = [R + g["starty"] + j * g["dist"] for j in range(g["ny"])]
    return cx, cy


def box_medians(plane, g):
    """B2: float32[K]."""
    f = to_float(plane)
    cx, cy = centres(g)
    med = np.zeros(g["K"], np.float32)
    for j, y in enumerate(cy):
        for i, x in enumerate(cx):
            bits = np.ascontiguousarray(f[y - R:y + R + 1, x - R:x + R + 1]).view(np.uint32).ravel()
            key = bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
            k = np.sort(key)[RANK]
            b = (k ^ np.uint32(0x80000000)) if (k >> 31) else (~k & np.uint32(0xFFFFFFFF))
            m = np.array([b], np.uint32).view(np.float32)[0]
            med[j * g["nx"] + i] = m if np.isfinite(m) else np.float32(0.0)
    return med


def _median(a):
    a = sorted(a)
    K = len(a)
    return a[K // 2] if K % 2 else (a[K // 2 - 1] + a[K // 2]) * 0.5


def select(med, tol):
    """B3 -> (keep uint8[K], kept, T, m, MAD)."""
    v = [float(x) for x in med]
    m = _median(v)
    mad = _median([abs(x - m) for x in v])
    T = m + float(tol) * mad
    keep = np.array([1 if (x > 0.0 and x <= T) else 0 for x in v], np.uint8)
    return keep, int(keep.sum()), T, m, mad


def _coord(c, n):
    x0 = float(n - 1) * 0.5
    ax = 1.0 / x0
    return (float(c) - x0) * ax


def _powers(u):
    u2 = u * u
    u3 = u2 * u
    u4 = u3 * u
    return [1.0, u, u2, u3, u4]


def axis_moments(n):
    """B5: [1, mean of u, mean of u^2, ...] over x = 0 .. n-1."""
    s = [0.0] * 5
    for x in range(n):
        p = _powers(_coord(x, n))
        for i in range(1, 5):
            s[i] = s[i] + p[i]
    return [1.0] + [s[i] / float(n) for i in range(1, 5)]


def normal_equations(med, keep, g, w, h, degree, descending=False):
    """A (n x n lists) and rhs of B4 over the kept boxes in ascending k
    (descending: the same sums in the opposite order, for the rounding floor)."""
    n = ncoef(degree)
    cx, cy = centres(g)
    A = [[0.0] * n for _ in range(n)]
    rhs = [0.0] * n
    order = range(g["K"] - 1, -1, -1) if descending else range(g["K"])
    for k in order:
        if not keep[k]:
            continue
        up = _powers(_coord(cx[k % g["nx"]], w))
        vp = _powers(_coord(cy[k // g["nx"]], h))
        phi = [up[i] * vp[j] for (i, j) in TERMS[:n]]
        z = float(med[k])
        for p in range(n):
            for q in range(n):
                A[p][q] = A[p][q] + phi[p] * phi[q]
            rhs[p] = rhs[p] + phi[p] * z
    return A, rhs


def cholesky_solve(A, rhs):
    """-> (status 0 | 2, c list of len(rhs))."""
    n = len(rhs)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0):
            return 2, [0.0] * n
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, n):
            a = A[i][j]
            for k in range(j):
                a = a - L[i][k] * L[j][k]
            L[i][j] = a / L[j][j]
    y = [0.0] * n
    for i in range(n):
        a = rhs[i]
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a / L[i][i]
    c = [0.0] * n
    for i in range(n - 1, -1, -1):
        a = y[i]
        for k in range(i + 1, n):
            a = a - L[k][i] * c[k]
        c[i] = a / L[i][i]
    return 0, c


def model_mean(c, w, h):
    Mx, My = axis_moments(w), axis_moments(h)
    s = 0.0
    for p, (i, j) in enumerate(TERMS):
        s = s + float(c[p]) * (Mx[i] * My[j])
    return s


def fit(med, keep, g, w, h, degree, descending=False):
    """B4 + B5 -> (status, c float64[15], mean)."""
    n = ncoef(degree)
    c = np.zeros(15, np.float64)
    if int(np.sum(keep)) < n:
        return 1, c, 0.0
    A, rhs = normal_equations(med, keep, g, w, h, degree, descending)
    st, sol = cholesky_solve(A, rhs)
    if st:
        return st, c, 0.0
    c[:n] = sol
    return 0, c, model_mean(c, w, h)


def background(c, w, h):
    """B6: float64[h, w], always the full degree-4 form."""
    c = np.asarray(c, np.float64)
    C = np.zeros((5, 5), np.float64)
    for p, (i, j) in enumerate(TERMS):
        C[i, j] = c[p]
    x0, y0 = float(w - 1) * 0.5, float(h - 1) * 0.5
    u = ((np.arange(w, dtype=np.float64) - x0) * (1.0 / x0))[None, :]
    v = ((np.arange(h, dtype=np.float64) - y0) * (1.0 / y0))[:, None]
    r = [(((C[k, 4] * v + C[k, 3]) * v + C[k, 2]) * v + C[k, 1]) * v + C[k, 0] for k in range(5)]
    return (((r[4] * u + r[3]) * u + r[2]) * u + r[1]) * u + r[0]


def correct(plane, c, mean, status=0, divide=False):
    """B7 of one plane -> float32[h, w]."""
    x = to_float(plane)
    if status:
        return x.copy()
    h, w = x.shape
    b = background(c, w, h)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        if divide:
            out = np.where(b == 0.0, np.float32(0.0), ((xd / b) * np.float64(mean)).astype(np.float32))
            return out.astype(np.float32)
        return ((xd - b) + np.float64(mean)).astype(np.float32)


def subsky_plane(plane, degree=1, samples=20, tolerance=1.0, divide=False):
    """B1-B7 of one plane -> (out float32, info dict)."""
    check_params(degree, tolerance)
    h, w = plane.shape
    g = grid(w, h, samples)
    med = box_medians(plane, g)
    keep, kept, T, m, mad = select(med, tolerance)
    st, c, mean = fit(med, keep, g, w, h, degree)
    out = correct(plane, c, mean, st, divide)
    return out, dict(med=med, keep=keep, kept=kept, T=T, coef=c, mean=mean, status=st, grid=g)

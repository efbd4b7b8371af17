"""Restatement of the stretches in numpy float64 with the
operation order of siril_amd/csrc/stretch_host.h: the contract the kernel of
siril_amd/csrc/stretch.hip and the host functions are compared with.  The
logarithm is tests/bkg_rbf_ref.py's (6k); exp is built here from + - * / and
bit operations in the same way; sqrt is IEEE.  numpy does not contract and every
elementwise operation below is rounded once.  Parity with a Siril binary is
unpinned."""
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bkg_rbf_ref import LN2_HI, LN2_LO, rbf_log  # noqa: E402

MTF, LINEAR, ASINH, GHT, INVGHT, MODASINH, INVMODASINH = range(7)
INDEPENDENT, HUMAN, EVEN = range(3)
CLIP, RESCALE, RGBBLEND = range(3)
Q_LOG, Q_NEG, Q_EXP, Q_POS, Q_ASINH, Q_IDENTITY = range(6)
NCOEF = 16
TINY = 2.2250738585072014e-308
INV_LN2 = 1.4426950408889634
MAD_SIGMA = 1.4826
HUMAN_W = (0.2126, 0.7152, 0.0722)
THIRD = 1.0 / 3.0
_FACT = [1.0 / float(math.factorial(k)) for k in range(14)]
# the ght family's coefficient block
G_D, G_B, G_AB, G_LP, G_SP, G_HP, G_A1, G_S1, G_A2, G_S2, G_S0, G_SPAN, G_INV, G_P1, G_P2, G_BD = range(16)


@dataclass
class Params:
    function: int
    model: int = INDEPENDENT
    clipmode: int = RGBBLEND
    mask: int = 7
    lo: float = 0.0
    m: float = 0.5
    hi: float = 1.0
    D: float = 0.0
    B: float = 0.0
    LP: float = 0.0
    SP: float = 0.0
    HP: float = 1.0
    beta: float = 1.0
    offset: float = 0.0
    BP: float = 0.0


# ---- T0 ----
def widen(a):
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return a.astype(np.float64) / 65535.0
    assert a.dtype == np.float32
    return a.astype(np.float64)


def clip01(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(v < 0.0, 0.0, v)
        return np.where(v > 1.0, 1.0, v)


# ---- T1 ----
def s_log(s):
    s = np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        return np.where(s != s, s, rbf_log(s).reshape(s.shape))


def floor_arg(s):
    s = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(s < TINY, TINY, s)


def s_exp(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        xc = np.where(x < -708.0, -708.0, x)
        xc = np.where(xc > 708.0, 708.0, xc)
        xc = np.where(x != x, 0.0, xc)
    nd = np.floor(xc * INV_LN2 + 0.5)
    r = (xc - nd * LN2_HI) - nd * LN2_LO
    p = np.full(x.shape, _FACT[13])
    for k in range(12, -1, -1):
        p = p * r
        p = p + _FACT[k]
    n = nd.astype(np.int64)
    scale = ((n + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return np.where(x != x, x, p * scale)


def s_pow(a, p):
    return s_exp(p * s_log(a))


def s_asinh(v):
    v = np.asarray(v, np.float64)
    return s_log(v + np.sqrt(v * v + 1.0))


# ---- T2 ----
def mtf01(xp, m, m1=None, m2=None):
    xp = np.asarray(xp, np.float64)
    if m1 is None:
        m1, m2 = m - 1.0, 2.0 * m - 1.0
    with np.errstate(all="ignore"):
        r = (m1 * xp) / (m2 * xp - m)
    return np.where(xp == 0.0, 0.0, np.where(xp == 1.0, 1.0, r))


# ---- T3 ----
def autostretch_params(median, mad, nimages, nch, linked=False, clip=-2.8, target=0.25):
    """lo, m, hi of every plane, float64[nimages * nch, 3]; median and mad in [0, 1] units."""
    if not (clip <= 0.0 and math.isfinite(clip)):
        raise ValueError("the shadows clip must be finite and <= 0")
    if not 0.0 < target < 1.0:
        raise ValueError("the target background must be inside (0, 1)")
    out = np.zeros((nimages * nch, 3))

    def finish(med, edge, inv):
        lo, hi = (0.0, edge) if inv else (edge, 1.0)
        if not hi > lo:
            raise ValueError("the plane has no spread")
        xm = float(clip01(((hi - med) if inv else (med - lo)) / (hi - lo)))
        t = float(mtf01(xm, target))
        m = 1.0 - t if inv else t
        if not 0.0 < m < 1.0:
            raise ValueError("the plane has no spread")
        return lo, m, hi

    for i in range(nimages):
        ps = range(i * nch, (i + 1) * nch)
        inv_all = 2 * sum(float(median[p]) > 0.5 for p in ps) > nch
        sum_med = sum_edge = 0.0
        for p in ps:
            med, sig = float(median[p]), MAD_SIGMA * float(mad[p])
            cs = clip * sig
            inv = inv_all if linked else med > 0.5
            edge = float(clip01(med - cs if inv else med + cs))
            if not linked:
                out[p] = finish(med, edge, inv)
            sum_med = sum_med + med
            sum_edge = sum_edge + edge
        if linked:
            out[i * nch:(i + 1) * nch] = finish(sum_med / float(nch), sum_edge / float(nch), inv_all)
    return out


# ---- T5 ----
def q(c, regime, u):
    u = np.asarray(u, np.float64)
    if regime == Q_LOG:
        return s_log(1.0 + c[G_D] * u)
    if regime == Q_NEG:
        return (1.0 - s_pow(1.0 + c[G_BD] * u, c[G_P1])) / (1.0 - c[G_AB])
    if regime == Q_EXP:
        return 1.0 - s_exp(-(c[G_D] * u))
    if regime == Q_POS:
        return 1.0 - s_pow(1.0 + c[G_BD] * u, c[G_P1])
    return s_asinh(c[G_D] * u)


def dq(c, regime, u):
    u = np.asarray(u, np.float64)
    du = c[G_D] * u
    w = 1.0 + c[G_BD] * u
    if regime == Q_LOG:
        return c[G_D] / (1.0 + du)
    if regime == Q_NEG:
        return c[G_D] * s_pow(w, -1.0 / c[G_AB])
    if regime == Q_EXP:
        return c[G_D] * s_exp(-du)
    if regime == Q_POS:
        return c[G_D] * s_pow(w, -(1.0 + c[G_B]) / c[G_B])
    return c[G_D] / np.sqrt(1.0 + du * du)


def qinv(c, regime, v):
    v = np.asarray(v, np.float64)
    if regime == Q_LOG:
        return (s_exp(v) - 1.0) / c[G_D]
    if regime == Q_NEG:
        base = 1.0 - v * (1.0 - c[G_AB])
        return (s_pow(floor_arg(base), c[G_P2]) - 1.0) / c[G_BD]
    if regime == Q_EXP:
        return -s_log(floor_arg(1.0 - v)) / c[G_D]
    if regime == Q_POS:
        return (s_pow(floor_arg(1.0 - v), c[G_P2]) - 1.0) / c[G_BD]
    return ((s_exp(v) - s_exp(-v)) * 0.5) / c[G_D]


# ---- T7 ----
def S(c, regime, x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(x < c[G_LP], c[G_LP], x)
        t = np.where(t > c[G_HP], c[G_HP], t)
        d = t - c[G_SP]
        u = np.where(d < 0.0, -d, d)
        qv = q(c, regime, u)
        sq = np.where(d < 0.0, -qv, qv)
        slope = np.where(x < c[G_LP], c[G_S1], np.where(x > c[G_HP], c[G_S2], 0.0))
        return sq + slope * (x - t)


def T(c, regime, x):
    x = np.asarray(x, np.float64)
    if regime == Q_IDENTITY:
        return x
    return clip01((S(c, regime, x) - c[G_S0]) * c[G_INV])


def Tinv(c, regime, y):
    y = np.asarray(y, np.float64)
    if regime == Q_IDENTITY:
        return y
    with np.errstate(all="ignore"):
        s = c[G_S0] + y * c[G_SPAN]
        lo = -c[G_A1]
        sc = np.where(s < lo, lo, s)
        sc = np.where(sc > c[G_A2], c[G_A2], sc)
        v = np.where(sc < 0.0, -sc, sc)
        u = qinv(c, regime, v)
        xq = np.where(sc < 0.0, c[G_SP] - u, c[G_SP] + u)
        slope = np.where(s < lo, c[G_S1], np.where(s > c[G_A2], c[G_S2], 1.0))
        lin = (s - sc) / floor_arg(slope)
        return clip01(xq + lin)


# ---- T9 and T6 ----
def check(p):
    def in01(v):
        return 0.0 <= v <= 1.0
    if p.function not in range(7):
        raise ValueError("unknown function")
    if p.model not in range(3):
        raise ValueError("unknown colour model")
    if p.clipmode not in range(3):
        raise ValueError("unknown clip mode")
    if not 1 <= p.mask <= 7:
        raise ValueError("the channel mask must be 1 .. 7")
    if p.function == MTF:
        if not (in01(p.lo) and in01(p.hi)):
            raise ValueError("low and high must be in [0, 1]")
        if not p.hi > p.lo:
            raise ValueError("high must be above low")
        if not 0.0 < p.m < 1.0:
            raise ValueError("the midtones balance must be inside (0, 1)")
    elif p.function == LINEAR:
        if not 0.0 <= p.BP < 1.0:
            raise ValueError("BP must be in [0, 1)")
    elif p.function == ASINH:
        if not 1.0 <= p.beta <= 1000.0:
            raise ValueError("the stretch must be in [1, 1000]")
        if not 0.0 <= p.offset < 1.0:
            raise ValueError("the offset must be in [0, 1)")
    else:
        if not 0.0 <= p.D <= 10.0:
            raise ValueError("D must be in [0, 10]")
        if p.function in (GHT, INVGHT) and not -5.0 <= p.B <= 15.0:
            raise ValueError("B must be in [-5, 15]")
        if not (in01(p.LP) and in01(p.SP) and in01(p.HP) and p.LP <= p.SP <= p.HP):
            raise ValueError("0 <= LP <= SP <= HP <= 1 must hold")


def coeffs(p):
    """T6 -> (float64[16], regime)."""
    check(p)
    c = np.zeros(NCOEF)
    if p.function == MTF:
        c[:6] = p.lo, p.m, p.hi, p.hi - p.lo, p.m - 1.0, 2.0 * p.m - 1.0
        return c, 0
    if p.function == LINEAR:
        c[:2] = p.BP, 1.0 - p.BP
        return c, 0
    if p.function == ASINH:
        c[:4] = p.beta, p.offset, 1.0 - p.offset, float(s_asinh(p.beta))
        return c, 0
    modasinh = p.function in (MODASINH, INVMODASINH)
    B = 0.0 if modasinh else float(p.B)
    b = -B if B < 0.0 else B
    D = float(s_exp(p.D)) - 1.0
    c[[G_D, G_B, G_AB, G_LP, G_SP, G_HP]] = D, B, b, p.LP, p.SP, p.HP
    if p.D == 0.0:
        return c, Q_IDENTITY
    c[G_BD] = b * D
    if modasinh:
        regime = Q_ASINH
    elif B == -1.0:
        regime = Q_LOG
    elif B < 0.0:
        regime = Q_NEG
        c[G_P1], c[G_P2] = (b - 1.0) / b, b / (b - 1.0)
    elif B == 0.0:
        regime = Q_EXP
    else:
        regime = Q_POS
        c[G_P1], c[G_P2] = -1.0 / B, -B
    ul, uh = p.SP - p.LP, p.HP - p.SP
    c[G_A1], c[G_S1] = float(q(c, regime, ul)), float(dq(c, regime, ul))
    c[G_A2], c[G_S2] = float(q(c, regime, uh)), float(dq(c, regime, uh))
    c[G_S0] = float(S(c, regime, 0.0))
    c[G_SPAN] = float(S(c, regime, 1.0)) - c[G_S0]
    c[G_INV] = 1.0 / c[G_SPAN]
    return c, regime


# ---- T8 ----
def joint(p, nch):
    return nch == 3 and (p.function == ASINH or (p.function >= GHT and p.model != INDEPENDENT))


def transfer(p, c, regime, x):
    """The ght family's transfer, forward or inverse, of x in [0, 1] (float64)."""
    return Tinv(c, regime, x) if p.function in (INVGHT, INVMODASINH) else T(c, regime, x)


def asinh_pre(c, x):
    with np.errstate(invalid="ignore"):
        v = x - c[1]
        v = np.where(v < 0.0, 0.0, v)
        return v / c[2]


def asinh_k(c, v):
    with np.errstate(all="ignore"):
        k = s_asinh(c[0] * v) / (v * c[3])
        return np.where(v == 0.0, 1.0, k)


def min1(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 1.0, 1.0, v)


def sample(p, x):
    """One parameter block on widened samples (float64, any shape) -> float64 before the rounding to float."""
    c, regime = coeffs(p)
    x = clip01(x)
    with np.errstate(all="ignore"):
        if p.function == MTF:
            return mtf01(clip01((x - c[0]) / c[3]), c[1], c[4], c[5])
        if p.function == LINEAR:
            v = (x - c[0]) / c[1]
            return np.where(v < 0.0, 0.0, v)
        if p.function == ASINH:
            v = asinh_pre(c, x)
            return min1(v * asinh_k(c, v))
        return transfer(p, c, regime, x)


def lum(p, x):
    w = HUMAN_W if p.model == HUMAN else (THIRD, THIRD, THIRD)
    return (w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]


def pixel3(p, xw):
    """xw float64[3, ...] widened samples of pixels -> float64[3, ...]."""
    c, regime = coeffs(p)
    with np.errstate(all="ignore"):
        if p.function == ASINH:
            x = asinh_pre(c, clip01(xw))
            return min1(x * asinh_k(c, lum(p, x))[None])
        x = clip01(xw)
        L = lum(p, x)
        tl = transfer(p, c, regime, L)
        kk = np.where(L == 0.0, 0.0, tl / L)
        s = x * kk[None]
        if p.clipmode == CLIP:
            return min1(s)
        if p.clipmode == RESCALE:
            mx = s[0]
            mx = np.where(s[1] > mx, s[1], mx)
            mx = np.where(s[2] > mx, s[2], mx)
            return np.where(mx[None] > 1.0, s / mx[None], s)
        clips = (s[0] > 1.0) | (s[1] > 1.0) | (s[2] > 1.0)
        t = transfer(p, c, regime, x)
        kb = np.ones(L.shape)
        for ch in range(3):
            r = (1.0 - t[ch]) / (s[ch] - t[ch])
            kb = np.where((s[ch] > 1.0) & (r < kb), r, kb)
        kt = 1.0 - kb
        return np.where(clips[None], min1(kb[None] * s + kt[None] * t), s)


def stretch(p, frames):
    """A parameter block on frames [N, H, W] or [N, C, H, W] (float32 or uint16) -> float32, T8 with the mask."""
    frames = np.asarray(frames)
    xw = widen(frames)
    nch = frames.shape[1] if frames.ndim == 4 else 1
    if joint(p, nch):
        o = np.moveaxis(pixel3(p, np.moveaxis(xw, 1, 0)), 0, 1)
    else:
        o = sample(p, xw)
    out = o.astype(np.float32)
    if nch == 3:
        for ch in range(3):
            if not p.mask >> ch & 1:
                out[:, ch] = xw[:, ch].astype(np.float32)
    return out


def float32_bits_equal(a, b):
    """NaN at the same places and every other sample equal as uint32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])

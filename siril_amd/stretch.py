"""The non-linear stretches on the GPU (Siril's `mtf`, `autostretch`,
`linstretch`, `asinh`, `ght`, `invght`, `modasinh`, `invmodasinh`): what turns a
linear stack into an image one can look at.

    shown, used = autostretch(frames)                  # [N, H, W] or [N, C, H, W]
    shown = ght(frames, D=6, B=3, SP=0.05, model="human")
    back = invght(shown, D=6, B=3, SP=0.05, model="human")

The kernel is siril_amd/csrc/stretch.hip behind the C-ABI
(`sgpu_stretch_planes_device`); the stretches are the specification in
DESIGN.md 6m (T0-T9), restated in tests/stretch_ref.py: samples widened to
double and clipped to [0, 1], double arithmetic rounded once per operation with
log / exp / pow built from + - * /, one rounding to float32.  Parity with a
Siril binary is unpinned.

Headless: `python -m siril_amd.cli <command> <image> ...` for each of the eight
commands (`run_stretch`).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from ._lib import StretchParams, check, lib

MTF, LINEAR, ASINH, GHT, INVGHT, MODASINH, INVMODASINH = range(7)
FUNCTIONS = ("mtf", "linstretch", "asinh", "ght", "invght", "modasinh", "invmodasinh")
MODELS = ("independent", "human", "even")
CLIPMODES = ("clip", "rescale", "rgbblend")
NCOEF = 16
MASKS = {"R": 1, "G": 2, "B": 4, "RG": 3, "RB": 5, "GB": 6, "RGB": 7}
COMMANDS = FUNCTIONS + ("autostretch",)


def channel_mask(channels) -> int:
    """`R`, `G`, `B`, `RG`, `RB`, `GB` (or None / `RGB`: every channel) -> the mask of sgpu_stretch_params."""
    if channels is None:
        return 7
    if isinstance(channels, int):
        return channels
    try:
        return MASKS[str(channels).upper()]
    except KeyError:
        raise ValueError(f"channels must be one of R, G, B, RG, RB, GB, not `{channels}'") from None


def _enum(value, names, what):
    if isinstance(value, int):
        return value
    try:
        return names.index(str(value).lower())
    except ValueError:
        raise ValueError(f"{what} must be one of {', '.join(names)}, not `{value}'") from None


def params(function, model="independent", clipmode="rgbblend", channels=None, lo=0.0, m=0.5, hi=1.0, D=0.0, B=0.0,
           LP=0.0, SP=0.0, HP=1.0, beta=1.0, offset=0.0, BP=0.0) -> StretchParams:
    """One parameter block (sgpu_stretch_params); D is D_user, 0 .. 10."""
    return StretchParams(_enum(function, FUNCTIONS, "function"), _enum(model, MODELS, "the colour model"),
                         _enum(clipmode, CLIPMODES, "the clip mode"), channel_mask(channels), lo, m, hi, D, B, LP, SP, HP,
                         beta, offset, BP)


def check_params(p: StretchParams) -> None:
    """T9's refusals (SgpuError)."""
    check(lib().sgpu_stretch_check(C.byref(p)), "sgpu_stretch_check")


def coeffs(p: StretchParams) -> np.ndarray:
    """The coefficient block the kernel is handed (T6): float64[16]."""
    c = np.zeros(NCOEF, np.float64)
    check(lib().sgpu_stretch_coeffs(C.byref(p), c.ctypes.data_as(C.POINTER(C.c_double))), "sgpu_stretch_coeffs")
    return c


def autostretch_params(stats, nimages: int, nchannels: int, unit: float = 1.0, linked: bool = False,
                       shadows_clip: float = -2.8, target_bg: float = 0.25) -> np.ndarray:
    """T3: lo, m, hi of every plane, float64[nimages*nchannels, 3], from the
    NormStats of normalization.norm_stats_device on the planes."""
    tab = np.ascontiguousarray(stats.as_table(), np.float64)
    st = np.ascontiguousarray(stats.status, np.int32)
    out = np.zeros((nimages * nchannels, 3), np.float64)
    check(lib().sgpu_autostretch_params(C.c_void_p(tab.ctypes.data), C.c_void_p(st.ctypes.data), nimages, nchannels,
                                        float(unit), int(bool(linked)), float(shadows_clip), float(target_bg),
                                        C.c_void_p(out.ctypes.data)), "sgpu_autostretch_params")
    return out


def _vp(p):
    return C.c_void_p(p) if p else None


def stretch_device(ctx, d_in: int, elem_size: int, nimages: int, nchannels: int, w: int, h: int, plane_stride: int,
                   blocks: Sequence[StretchParams], d_out: int, out_stride: int):
    """sgpu_stretch_planes_device on raw device pointers; asynchronous."""
    arr = (StretchParams * len(blocks))(*blocks)
    check(lib().sgpu_stretch_planes_device(ctx.h, _vp(d_in), elem_size, nimages, nchannels, w, h, plane_stride, arr,
                                           len(blocks), _vp(d_out), out_stride), "sgpu_stretch_planes_device")


def last_kernel_ms(ctx):
    """(ms, launches) of the context's last stretch call."""
    ms, n = C.c_float(0), C.c_int(0)
    check(lib().sgpu_stretch_last_kernel_ms(ctx.h, C.byref(ms), C.byref(n)), "sgpu_stretch_last_kernel_ms")
    return float(ms.value), n.value


def _shape(frames):
    from .wavelets import _frames
    _frames(frames)
    n = int(frames.shape[0])
    nch = int(frames.shape[1]) if frames.dim() == 4 else 1
    return n, nch, int(frames.shape[-2]), int(frames.shape[-1])


def stretch(frames, blocks, out=None, ctx=None):
    """T0-T8 of CUDA frames [N, H, W] or [N, C, H, W] (float32, or 16-bit WORD
    storage as int16): float32, shaped like frames.  `blocks` is one
    StretchParams or a sequence of 1, N or N*C of them (per call, per image, per
    plane).  `out` is allocated unless given and may not be `frames`."""
    import torch
    from .wavelets import _ctx
    n, nch, h, w = _shape(frames)
    if isinstance(blocks, StretchParams):
        blocks = [blocks]
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_cuda or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    stretch_device(_ctx(ctx, frames), frames.data_ptr(), frames.element_size(), n, nch, w, h, h * w, list(blocks),
                   out.data_ptr(), h * w)
    return out


def mtf(frames, lo: float, m: float, hi: float, channels=None, out=None, ctx=None):
    """The midtones transfer function (T2) with shadows lo, midtones balance m and highlights hi."""
    return stretch(frames, params(MTF, lo=lo, m=m, hi=hi, channels=channels), out, ctx)


def autostretch(frames, linked: bool = False, shadows_clip: float = -2.8, target_bg: float = 0.25, out=None, ctx=None):
    """`mtf` with the parameters of T3 from every plane's median and MAD
    (normalization.norm_stats_device; its rule for which samples count is kept:
    samples that are 0 do not).  Returns the image and the parameters used,
    float64[N*C, 3] = lo, m, hi per plane.  The statistics cost one
    synchronisation for a handful of doubles: this is not the hot path."""
    from .normalization import norm_stats_device
    from .wavelets import _ctx
    n, nch, h, w = _shape(frames)
    ctx = _ctx(ctx, frames)
    st = norm_stats_device(ctx, frames.reshape(n * nch, h, w), lite=True)
    used = autostretch_params(st, n, nch, 65535.0 if frames.element_size() == 2 else 1.0, linked, shadows_clip,
                              target_bg)
    blocks = [params(MTF, lo=lo, m=m, hi=hi) for lo, m, hi in used]
    return stretch(frames, blocks, out, ctx), used


def linstretch(frames, BP: float, out=None, ctx=None):
    """max(0, (x - BP)/(1 - BP)) (T4)."""
    return stretch(frames, params(LINEAR, BP=BP), out, ctx)


def asinh(frames, stretch_factor: float, offset: float = 0.0, human: bool = False, out=None, ctx=None):
    """The asinh stretch (T4); on three channels the factor comes from the luminance (human weights or thirds)."""
    return stretch(frames, params(ASINH, beta=stretch_factor, offset=offset, model="human" if human else "even"), out, ctx)


def _ght(fn, frames, D, B, LP, SP, HP, model, clipmode, channels, out, ctx):
    return stretch(frames, params(fn, model, clipmode, channels, D=D, B=B, LP=LP, SP=SP, HP=HP), out, ctx)


def ght(frames, D, B=0.0, LP=0.0, SP=0.0, HP=1.0, model="independent", clipmode="rgbblend", channels=None, out=None,
        ctx=None):
    """The generalised hyperbolic stretch (T5-T8); D is D_user in [0, 10]."""
    return _ght(GHT, frames, D, B, LP, SP, HP, model, clipmode, channels, out, ctx)


def invght(frames, D, B=0.0, LP=0.0, SP=0.0, HP=1.0, model="independent", clipmode="rgbblend", channels=None, out=None,
           ctx=None):
    """The inverse of `ght`'s transfer, in closed form."""
    return _ght(INVGHT, frames, D, B, LP, SP, HP, model, clipmode, channels, out, ctx)


def modasinh(frames, D, LP=0.0, SP=0.0, HP=1.0, model="independent", clipmode="rgbblend", channels=None, out=None,
             ctx=None):
    """`ght` with q(u) = asinh(D u)."""
    return _ght(MODASINH, frames, D, 0.0, LP, SP, HP, model, clipmode, channels, out, ctx)


def invmodasinh(frames, D, LP=0.0, SP=0.0, HP=1.0, model="independent", clipmode="rgbblend", channels=None, out=None,
                ctx=None):
    """The inverse of `modasinh`'s transfer."""
    return _ght(INVMODASINH, frames, D, 0.0, LP, SP, HP, model, clipmode, channels, out, ctx)


# ------------------------------------------------------------------ commands
@dataclass
class StretchCommand:
    command: str
    image: str
    kwargs: dict = field(default_factory=dict)
    out: str = ""


def _number(name, what, word):
    try:
        v = float(word)
    except ValueError:
        raise ValueError(f"{name}: {what} must be a number, not `{word}'") from None
    if math.isnan(v):
        raise ValueError(f"{name}: {what} must be a number, not `{word}'")
    return v


def _is_number(word):
    try:
        float(word)
        return True
    except ValueError:
        return False


def _range(name, what, v, lo, hi, text, open_lo=False, open_hi=False):
    if not ((v > lo if open_lo else v >= lo) and (v < hi if open_hi else v <= hi)):
        raise ValueError(f"{name}: {what} must be in {text}")
    return v


def parse_stretch_command(words: Sequence[str]) -> StretchCommand:
    """One of
    `mtf <image> <low> <mid> <high> [channels]`,
    `autostretch <image> [-linked] [shadowsclip [targetbg]]`,
    `linstretch <image> -BP=`,
    `asinh <image> [-human] <stretch> [offset]`,
    `ght <image> -D= [-B=] [-LP=] [-SP=] [-HP=] [-human|-even|-independent] [-clipmode=clip|rescale|rgbblend] [channels]`,
    `invght`, `modasinh`, `invmodasinh` with ght's options (the modasinh pair has no -B=);
    every one takes [-out=FILE]."""
    words = list(words)
    if not words or words[0] not in COMMANDS:
        raise ValueError(f"not a stretch command: `{words[0] if words else ''}'")
    name = words[0]
    pos = [w for w in words[1:] if not w.startswith("-") or _is_number(w)]
    opts = [w for w in words[1:] if w.startswith("-") and not _is_number(w)]
    if not pos or _is_number(pos[0]):
        raise ValueError(f"{name} needs an image")
    cmd = StretchCommand(command=name, image=pos[0])
    pos, kw = pos[1:], cmd.kwargs
    family = name in ("ght", "invght", "modasinh", "invmodasinh")
    for o in opts:
        if o.startswith("-out="):
            if not o[5:]:
                raise ValueError(f"{name}: -out= needs a file name")
            cmd.out = o[5:]
        elif name == "autostretch" and o == "-linked":
            kw["linked"] = True
        elif name == "linstretch" and o.startswith("-BP="):
            kw["BP"] = _range(name, "-BP=", _number(name, "-BP=", o[4:]), 0.0, 1.0, "[0, 1)", open_hi=True)
        elif name == "asinh" and o == "-human":
            kw["human"] = True
        elif family and o.startswith("-D="):
            kw["D"] = _range(name, "-D=", _number(name, "-D=", o[3:]), 0.0, 10.0, "[0, 10]")
        elif family and name in ("ght", "invght") and o.startswith("-B="):
            kw["B"] = _range(name, "-B=", _number(name, "-B=", o[3:]), -5.0, 15.0, "[-5, 15]")
        elif family and o[:4] in ("-LP=", "-SP=", "-HP="):
            kw[o[1:3]] = _range(name, o[:4], _number(name, o[:4], o[4:]), 0.0, 1.0, "[0, 1]")
        elif family and o in ("-human", "-even", "-independent"):
            if "model" in kw:
                raise ValueError(f"{name}: only one of -human, -even, -independent")
            kw["model"] = o[1:]
        elif family and o.startswith("-clipmode="):
            if o[10:] not in CLIPMODES:
                raise ValueError(f"{name}: -clipmode= must be clip, rescale or rgbblend, not `{o[10:]}'")
            kw["clipmode"] = o[10:]
        else:
            raise ValueError(f"Unexpected argument to {name} `{o}', aborting.")
    if name == "mtf":
        if len(pos) not in (3, 4) or not all(_is_number(w) for w in pos[:3]):
            raise ValueError("mtf needs an image, low, mid and high, and at most the channels (R, G, B, RG, RB, GB)")
        lo, m, hi = (_number(name, what, w) for what, w in zip(("low", "mid", "high"), pos))
        _range(name, "low", lo, 0.0, 1.0, "[0, 1]")
        _range(name, "high", hi, 0.0, 1.0, "[0, 1]")
        _range(name, "mid", m, 0.0, 1.0, "(0, 1)", open_lo=True, open_hi=True)
        if not hi > lo:
            raise ValueError("mtf: high must be above low")
        kw.update(lo=lo, m=m, hi=hi)
        if len(pos) == 4:
            try:
                kw["channels"] = pos[3].upper() if channel_mask(pos[3]) else None
            except ValueError as e:
                raise ValueError(f"mtf: {e}") from None
    elif name == "autostretch":
        if len(pos) > 2:
            raise ValueError("autostretch takes at most the shadows clip and the target background")
        if pos:
            kw["shadows_clip"] = _number(name, "the shadows clip", pos[0])
            if not (kw["shadows_clip"] <= 0.0 and math.isfinite(kw["shadows_clip"])):
                raise ValueError("autostretch: the shadows clip must be finite and <= 0")
        if len(pos) == 2:
            kw["target_bg"] = _range(name, "the target background", _number(name, "the target background", pos[1]),
                                     0.0, 1.0, "(0, 1)", open_lo=True, open_hi=True)
    elif name == "linstretch":
        if pos:
            raise ValueError(f"Unexpected argument to linstretch `{pos[0]}', aborting.")
        if "BP" not in kw:
            raise ValueError("linstretch needs -BP=")
    elif name == "asinh":
        if len(pos) not in (1, 2):
            raise ValueError("asinh needs an image and the stretch (1 .. 1000), and at most the offset")
        kw["stretch_factor"] = _range(name, "the stretch", _number(name, "the stretch", pos[0]), 1.0, 1000.0, "[1, 1000]")
        if len(pos) == 2:
            kw["offset"] = _range(name, "the offset", _number(name, "the offset", pos[1]), 0.0, 1.0, "[0, 1)", open_hi=True)
    else:
        if "D" not in kw:
            raise ValueError(f"{name} needs -D=")
        if len(pos) > 1:
            raise ValueError(f"Unexpected argument to {name} `{pos[1]}', aborting.")
        if pos:
            try:
                channel_mask(pos[0])
            except ValueError as e:
                raise ValueError(f"{name}: {e}") from None
            kw["channels"] = pos[0].upper()
        if not kw.get("LP", 0.0) <= kw.get("SP", 0.0) <= kw.get("HP", 1.0):
            raise ValueError(f"{name}: 0 <= LP <= SP <= HP <= 1 must hold")
    return cmd


def apply_command(cmd: StretchCommand, frames, ctx=None):
    """The parsed command on frames: what `run_stretch` writes."""
    fn = {"mtf": mtf, "linstretch": linstretch, "asinh": asinh, "ght": ght, "invght": invght, "modasinh": modasinh,
          "invmodasinh": invmodasinh}
    if cmd.command == "autostretch":
        return autostretch(frames, ctx=ctx, **cmd.kwargs)[0]
    return fn[cmd.command](frames, ctx=ctx, **cmd.kwargs)


def run_stretch(line, ctx=None):
    """Run one stretch command line (a string or its words): reads the FITS
    image (16- or 32-bit, one or three layers), stretches it and writes one
    32-bit image, <stem>_<command>.fit next to the input unless -out= names it.
    Returns its path."""
    from .sequence import write_fits
    from .stacking import Context
    from .wavelets import _image_path, _load
    cmd = parse_stretch_command(line.split() if isinstance(line, str) else line)
    path = _image_path(cmd.image)
    ctx = ctx or Context(0)
    t = _load(path, ctx)
    try:
        res = apply_command(cmd, t, ctx)
    except RuntimeError as e:
        raise ValueError(f"{cmd.command}: {e}") from None
    d, stem = os.path.dirname(os.path.abspath(path)), os.path.splitext(os.path.basename(path))[0]
    out = cmd.out or os.path.join(d, f"{stem}_{cmd.command}.fit")
    write_fits(out, res[0].cpu().numpy())
    return out

"""Frame calibration on the GPU: bias, dark, flat, dark optimisation and
cosmetic correction (Siril's `calibrate` command, core/preprocess.c).

    masters = prepare_masters(dark=dark, flat=flat, cfa=True, equalize_cfa=True, cc_sigma=(3, 3))
    out, k = calibrate(frames, masters, dark_optim=True)

The kernels are siril_amd/csrc/calibrate.hip behind the C-ABI
(`sgpu_calibrate_frames_device` and friends); the arithmetic is the
specification in DESIGN.md "Calibration", restated in tests/calib_ref.py.
Parity with a Siril binary is unpinned.

Headless: `python -m siril_amd.cli calibrate <seq> [-bias=F | -bias="=LEVEL"]
[-dark=F] [-flat=F] [-cc=dark [cold hot]] [-cfa] [-equalize_cfa] [-opt]
[-prefix=pp_]` (`run_calibrate`).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from ._lib import check, lib

INV_USHRT_MAX = np.float32(1.0) / np.float32(65535.0)      # S1
COLD_PIXEL, HOT_PIXEL = 0, 1


def to_float_plane(a) -> np.ndarray:
    """S1 on a master: uint16 -> float32 * (1.0f / 65535.0f); float32 as it is."""
    a = np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    if a.dtype == np.uint16:
        return np.ascontiguousarray(a.astype(np.float32) * INV_USHRT_MAX)
    return np.ascontiguousarray(a, np.float32)


@dataclass
class Masters:
    """Device-resident masters of one calibration (prepare_masters)."""
    bias: object = None                     # float32 CUDA plane, or None
    bias_level: Optional[float] = None      # [0, 1] units, used when there is no plane
    dark: object = None
    flat: object = None                     # after -equalize_cfa when that is on
    norm: float = 1.0                       # multiplies the flat quotient
    cfa: bool = False
    deviant: object = None                  # int32 CUDA [n, 2]: (y*W + x, COLD_PIXEL | HOT_PIXEL)
    equalize: Optional[tuple] = None        # (green diagonal, c1, c2) of -equalize_cfa
    cc_stats: Optional[tuple] = None        # (median, sigma, thresHot, thresCold) of the dark
    ctx: object = field(default=None, repr=False)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _use_stream(ctx, t):
    import torch
    ctx.set_stream(torch.cuda.current_stream(t.device).cuda_stream)


def region_stats(plane, x0=0, y0=0, x1=None, y1=None, step=1, ctx=None):
    """S4 of a float32 CUDA plane [H, W] -> (n, mean, sigma)."""
    from .stacking import Context
    ctx = ctx or Context(plane.device.index or 0)
    h, w = plane.shape
    n, m, s = C.c_long(0), C.c_double(0), C.c_double(0)
    _use_stream(ctx, plane)
    check(lib().sgpu_region_stats_device(ctx.h, _ptr(plane), w, h, x0, y0, w if x1 is None else x1,
                                         h if y1 is None else y1, step, C.byref(n), C.byref(m), C.byref(s)),
          "sgpu_region_stats_device")
    return int(n.value), float(m.value), float(s.value)


def equalize_cfa_flat(flat, pattern_size: int = 2, ctx=None):
    """S5: a new equalised plane and (green diagonal, c1, c2)."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(flat.device.index or 0)
    h, w = flat.shape
    out = torch.empty_like(flat)
    coef = (C.c_float * 2)()
    diag = C.c_int(0)
    _use_stream(ctx, flat)
    check(lib().sgpu_equalize_cfa_flat_device(ctx.h, _ptr(flat), _ptr(out), w, h, pattern_size, coef, C.byref(diag)),
          "sgpu_equalize_cfa_flat_device")
    return out, (int(diag.value), float(coef[0]), float(coef[1]))


def find_deviant_pixels(dark, cold: float, hot: float, ctx=None):
    """S6: (int32 CUDA list [n, 2], (median, sigma, thresHot, thresCold))."""
    import torch
    from .stacking import Context
    if dark is None:
        h = w = 1
        dev = 0
    else:
        h, w = dark.shape
        dev = dark.device.index or 0
    ctx = ctx or Context(dev)
    if dark is not None:
        _use_stream(ctx, dark)
    cnt = C.c_long(0)
    st = (C.c_double * 4)()
    check(lib().sgpu_find_deviant_pixels_device(ctx.h, _ptr(dark), w, h, float(cold), float(hot), None, 0,
                                                C.byref(cnt), st), "sgpu_find_deviant_pixels_device")
    lst = torch.empty((cnt.value, 2), dtype=torch.int32, device=dark.device)
    if cnt.value:
        check(lib().sgpu_find_deviant_pixels_device(ctx.h, _ptr(dark), w, h, float(cold), float(hot), _ptr(lst),
                                                    cnt.value, C.byref(cnt), st), "sgpu_find_deviant_pixels_device")
    return lst, tuple(float(v) for v in st)


def cosmetic_correction(frames, deviant, cfa: bool = False, ctx=None):
    """S7 in place on float32 CUDA frames [N, H, W]; returns `frames`."""
    from .stacking import Context
    ctx = ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous() or frames.element_size() != 4:
        raise ValueError("frames must be a contiguous float32 CUDA tensor [N, H, W]")
    n, h, w = frames.shape
    cnt = 0 if deviant is None else int(deviant.shape[0])
    _use_stream(ctx, frames)
    check(lib().sgpu_cosmetic_correction_device(ctx.h, _ptr(frames), n, w, h, h * w, _ptr(deviant) if cnt else None,
                                                cnt, int(bool(cfa))), "sgpu_cosmetic_correction_device")
    return frames


def prepare_masters(bias=None, dark=None, flat=None, cfa: bool = False, equalize_cfa: bool = False,
                    cc_sigma: Optional[Sequence[float]] = None, norm: Optional[float] = None, ctx=None,
                    device: int = 0, cfa_pattern_size: int = 2) -> Masters:
    """Bring the masters to the device once: bias a plane or a level in [0, 1]
    units, dark and flat planes (numpy or torch; uint16 planes go through S1).
    equalize_cfa: S5 on a copy of the flat.  norm: the flat's S4 mean (after
    the equalisation) unless given.  cc_sigma = (cold, hot): S6 deviant list
    of the dark (-1 disables one kind)."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(device)
    dev = torch.device("cuda", ctx.device)

    def up(a):
        return None if a is None else torch.from_numpy(to_float_plane(a)).to(dev)

    m = Masters(cfa=bool(cfa), ctx=ctx)
    if bias is not None and np.isscalar(bias):
        m.bias_level = float(np.float32(bias))
    else:
        m.bias = up(bias)
    m.dark = up(dark)
    m.flat = up(flat)
    if equalize_cfa and m.flat is not None:
        m.flat, m.equalize = equalize_cfa_flat(m.flat, cfa_pattern_size, ctx)
    if norm is not None:
        m.norm = float(np.float32(norm))
    elif m.flat is not None:
        m.norm = float(np.float32(region_stats(m.flat, ctx=ctx)[1]))
    if cc_sigma is not None:
        m.deviant, m.cc_stats = find_deviant_pixels(m.dark, cc_sigma[0], cc_sigma[1], ctx)
    return m


def calibrate_device(ctx, d_in, d_out, elem_size: int, n: int, w: int, h: int, frame_stride: int, masters: Masters,
                     d_k=None, dark_optim: bool = False):
    """sgpu_calibrate_frames_device on raw device pointers (frame f at
    base + f*frame_stride samples, in and out)."""
    cnt = 0 if masters.deviant is None else int(masters.deviant.shape[0])
    lvl = masters.bias_level
    check(lib().sgpu_calibrate_frames_device(
        ctx.h, C.c_void_p(d_in), C.c_void_p(d_out), elem_size, n, w, h, frame_stride, _ptr(masters.bias),
        int(lvl is not None), float(lvl or 0.0), _ptr(masters.dark), _ptr(masters.flat), float(masters.norm),
        C.c_void_p(d_k) if d_k else None, _ptr(masters.deviant) if masters.deviant is not None else None, cnt,
        int(bool(masters.cfa)), int(bool(dark_optim))), "sgpu_calibrate_frames_device")


def dark_optimize(frames, masters: Masters, ctx=None) -> np.ndarray:
    """S3 alone: k[N] (float32) of CUDA frames [N, H, W]."""
    from .stacking import Context
    ctx = ctx or masters.ctx or Context(frames.device.index or 0)
    n, h, w = frames.shape
    k = np.zeros(n, np.float32)
    lvl = masters.bias_level
    _use_stream(ctx, frames)
    check(lib().sgpu_dark_optimize_device(ctx.h, _ptr(frames), frames.element_size(), n, w, h, h * w,
                                          _ptr(masters.bias), int(lvl is not None), float(lvl or 0.0),
                                          _ptr(masters.dark), None, k.ctypes.data_as(C.c_void_p)),
          "sgpu_dark_optimize_device")
    return k


def calibrate(frames, masters: Masters, dark_optim: bool = False, out=None, ctx=None):
    """Calibrate CUDA frames [N, H, W] (float32, or 16-bit WORD storage) into
    float32 `out` (allocated unless given; `frames` itself is allowed for
    float32 input): S1, S2, S3 with dark_optim, S7 when the masters carry a
    deviant list.  Returns out, or (out, k) with dark_optim (k: float32
    numpy, the factor each frame's dark was scaled with)."""
    import torch
    from .stacking import Context
    ctx = ctx or masters.ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W]")
    n, h, w = frames.shape
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != (n, h, w) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    for pl in (masters.bias, masters.dark, masters.flat):
        if pl is not None and tuple(pl.shape) != (h, w):
            raise ValueError("a master does not have the frames' size")
    dk = torch.empty(n, dtype=torch.float32, device=frames.device) if dark_optim else None
    _use_stream(ctx, frames)
    calibrate_device(ctx, frames.data_ptr(), out.data_ptr(), frames.element_size(), n, w, h, h * w, masters,
                     dk.data_ptr() if dk is not None else None, dark_optim)
    if dark_optim:
        return out, dk.cpu().numpy()
    return out


# ------------------------------------------------------------------ command
@dataclass
class CalibrateCommand:
    seq: str
    bias: Optional[str] = None              # file
    bias_level: Optional[float] = None      # [0, 1] units (-bias="=LEVEL", LEVEL in ADU)
    dark: Optional[str] = None
    flat: Optional[str] = None
    cc: bool = False
    cc_sigma: tuple = (3.0, 3.0)            # (cold, hot), Siril's defaults
    cfa: bool = False
    equalize_cfa: bool = False
    opt: bool = False
    prefix: str = "pp_"


def parse_calibrate_command(words: Sequence[str]) -> CalibrateCommand:
    """`calibrate <seq> [-bias=F | -bias="=LEVEL"] [-dark=F] [-flat=F]
    [-cc=dark [cold hot]] [-cfa] [-equalize_cfa] [-opt] [-prefix=pp_]`."""
    words = list(words)
    if words and words[0] == "calibrate":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("calibrate needs a sequence name")
    cmd = CalibrateCommand(seq=words[0])
    i = 1
    while i < len(words):
        o = words[i]
        i += 1
        if o.startswith("-bias="):
            v = o[6:].strip('"')
            if v.startswith("="):
                cmd.bias_level = float(np.float32(float(v[1:])) * INV_USHRT_MAX)
            elif v:
                cmd.bias = v
            else:
                raise ValueError("Missing filename after -bias=")
        elif o.startswith("-dark="):
            cmd.dark = o[6:]
        elif o.startswith("-flat="):
            cmd.flat = o[6:]
        elif o.startswith("-cc="):
            if o[4:] != "dark":
                raise ValueError("only -cc=dark is supported (bad-pixel maps are not)")
            cmd.cc = True
            nums = []
            while i < len(words) and len(nums) < 2:      # the two sigmas, -1 included
                try:
                    nums.append(float(words[i]))
                except ValueError:
                    break
                i += 1
            if len(nums) == 2:
                cmd.cc_sigma = (nums[0], nums[1])
            elif nums:
                raise ValueError("-cc=dark takes both sigmas (cold hot) or neither")
        elif o == "-cfa":
            cmd.cfa = True
        elif o == "-equalize_cfa":
            cmd.equalize_cfa = True
        elif o == "-opt":
            cmd.opt = True
        elif o.startswith("-prefix="):
            cmd.prefix = o[8:]
        elif o in ("-debayer", "-fix_xtrans"):
            raise ValueError(f"{o} is not supported by this calibrate")
        else:
            raise ValueError(f"Unexpected argument to calibrate `{o}', aborting.")
    if (cmd.cc or cmd.opt) and not cmd.dark:
        raise ValueError("-cc=dark and -opt need -dark=")
    return cmd


def _read_seq(path: str):
    """(name, fixed, image numbers) of a regular-FITS .seq file."""
    name, fixed, nums = None, 5, []
    with open(path) as f:
        for line in f:
            if line.startswith("T"):
                raise ValueError("calibrate reads regular FITS sequences only (not SER / FITSEQ)")
            if line.startswith("S "):
                parts = line[2:].strip()
                if parts.startswith("'"):
                    name, rest = parts[1:].split("'", 1)
                    rest = rest.split()
                else:
                    name, *rest = parts.split()
                fixed = int(rest[3])
            elif line.startswith("I "):
                nums.append(int(line.split()[1]))
    if name is None:
        raise ValueError(f"{path}: no S line")
    return name, fixed, nums


def _master_file(path: str, d: str) -> np.ndarray:
    from .sequence import read_fits
    for cand in (path, path + ".fit", os.path.join(d, path), os.path.join(d, path + ".fit")):
        if os.path.isfile(cand):
            a = read_fits(cand)
            if a.ndim != 2:
                raise ValueError(f"{cand}: RGB masters are not supported")
            return a
    raise FileNotFoundError(path)


def run_calibrate(line, ctx=None, max_batch_bytes: int = 1 << 30):
    """Run one `calibrate` command line (a string or its words): reads the
    regular FITS sequence, calibrates in batches of at most max_batch_bytes
    of output, writes 32-bit <prefix><name>NNNNN.fit and <prefix><name>.seq.
    Returns (path of the new .seq, k per frame or None)."""
    import torch
    from .sequence import frame_name, read_fits, write_fits, write_seq
    from .stacking import Context
    cmd = parse_calibrate_command(line.split() if isinstance(line, str) else line)
    seq = cmd.seq if cmd.seq.endswith(".seq") else cmd.seq + ".seq"
    d = os.path.dirname(os.path.abspath(seq))
    name, fixed, nums = _read_seq(seq)
    if nums != list(range(nums[0], nums[0] + len(nums))):
        raise ValueError("calibrate needs consecutively numbered images")
    ctx = ctx or Context(0)
    masters = prepare_masters(
        bias=cmd.bias_level if cmd.bias_level is not None else (_master_file(cmd.bias, d) if cmd.bias else None),
        dark=_master_file(cmd.dark, d) if cmd.dark else None, flat=_master_file(cmd.flat, d) if cmd.flat else None,
        cfa=cmd.cfa, equalize_cfa=cmd.equalize_cfa, cc_sigma=cmd.cc_sigma if cmd.cc else None, ctx=ctx)
    ks = []
    first = read_fits(os.path.join(d, frame_name(name, nums[0], fixed)))
    if first.ndim != 2:
        raise ValueError("calibrate takes one-plane (mono / CFA) frames")
    h, w = first.shape
    batch = max(1, int(max_batch_bytes // (h * w * 4)))
    dev = torch.device("cuda", ctx.device)
    for b0 in range(0, len(nums), batch):
        part = nums[b0:b0 + batch]
        host = np.stack([first if (b0 == 0 and j == 0) else read_fits(os.path.join(d, frame_name(name, num, fixed)))
                         for j, num in enumerate(part)])
        if host.shape[1:] != (h, w):
            raise ValueError("frames of different sizes")
        t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
        res = calibrate(t, masters, dark_optim=cmd.opt, ctx=ctx)
        if cmd.opt:
            res, k = res
            ks.extend(float(v) for v in k)
        res = res.cpu().numpy()
        for j, num in enumerate(part):
            write_fits(os.path.join(d, frame_name(cmd.prefix + name, num, fixed)), res[j])
    out_seq = os.path.join(d, cmd.prefix + name + ".seq")
    write_seq(out_seq, cmd.prefix + name, len(nums), beg=nums[0], fixed=fixed)
    return out_seq, (np.array(ks, np.float32) if cmd.opt else None)

"""A trous ("with holes") wavelets on the GPU (Siril's `wavelet`, `wrecons`
and `extract`, filters/wavelets): the decomposition of every plane into
n - 1 detail planes and a residual, and the weighted reconstruction that
sharpens with them.

    planes = atrous(frames, 6)                          # [..., 6, H, W]
    sharp = reconstruct(planes, (3, 2, 1.5, 1, 1, 1))
    sharp = wrecons(frames, (3, 2, 1.5, 1, 1, 1))       # the same bits, no plane is written

The kernels are siril_amd/csrc/wavelet.hip behind the C-ABI
(`sgpu_wavelet_planes_device`, `sgpu_wavelet_reconstruct_device`,
`sgpu_wrecons_planes_device`); the arithmetic is the specification in
DESIGN.md 6j (W0-W5), restated in tests/wavelet_ref.py.  Parity with a Siril
binary is unpinned.

Headless: `python -m siril_amd.cli wavelet <image> <nbr_layers> <type>
[-prefix=]` (`run_wavelet`) and `python -m siril_amd.cli wrecons <image> c1 ...
cn [-type=1|2] [-out=FILE]` (`run_wrecons`).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

from ._lib import check, lib

MAX_LAYERS = 6
MAX_LAUNCHES = 16
FORMS = ("tile", "row", "col", "recon")


def check_layers(w: int, h: int, nbr_layers: int, type: int = 2) -> None:
    """W1's refusals (SgpuError): nbr_layers outside 1 .. 6, type outside 1 .. 2,
    a w x h plane too small for the largest tap offset."""
    check(lib().sgpu_wavelet_check(int(w), int(h), int(nbr_layers), int(type)), "sgpu_wavelet_check")


def _coef(coefs):
    k = np.asarray(coefs, dtype=np.float32).reshape(-1)
    if not 1 <= len(k) <= MAX_LAYERS:
        raise ValueError("1 .. 6 coefficients, one per plane")
    return (C.c_float * len(k))(*[float(v) for v in k])


def _vp(p):
    return C.c_void_p(p) if p else None


def atrous_device(ctx, d_in: int, elem_size: int, nplanes: int, w: int, h: int, plane_stride: int, nbr_layers: int,
                  type: int, d_planes: int, out_plane_stride: int, out_image_stride: int):
    """sgpu_wavelet_planes_device on raw device pointers; asynchronous."""
    check(lib().sgpu_wavelet_planes_device(ctx.h, _vp(d_in), elem_size, nplanes, w, h, plane_stride, nbr_layers, type,
                                           _vp(d_planes), out_plane_stride, out_image_stride),
          "sgpu_wavelet_planes_device")


def reconstruct_device(ctx, d_planes: int, nplanes: int, w: int, h: int, plane_stride: int, image_stride: int,
                       coefs, d_out: int, out_stride: int):
    """sgpu_wavelet_reconstruct_device on raw device pointers; asynchronous."""
    k = _coef(coefs)
    check(lib().sgpu_wavelet_reconstruct_device(ctx.h, _vp(d_planes), nplanes, w, h, plane_stride, image_stride, len(k),
                                                k, _vp(d_out), out_stride), "sgpu_wavelet_reconstruct_device")


def wrecons_device(ctx, d_in: int, elem_size: int, nplanes: int, w: int, h: int, plane_stride: int, coefs, type: int,
                   d_out: int, out_stride: int):
    """sgpu_wrecons_planes_device on raw device pointers; asynchronous."""
    k = _coef(coefs)
    check(lib().sgpu_wrecons_planes_device(ctx.h, _vp(d_in), elem_size, nplanes, w, h, plane_stride, len(k), type, k,
                                           _vp(d_out), out_stride), "sgpu_wrecons_planes_device")


def last_kernel_ms(ctx) -> list:
    """[(form, first scale, scales, ms)] of the launches of the context's last
    wavelet call; form is one of FORMS."""
    ms, what, n = (C.c_float * MAX_LAUNCHES)(), (C.c_int * MAX_LAUNCHES)(), C.c_int(0)
    check(lib().sgpu_wavelet_last_kernel_ms(ctx.h, ms, what, C.byref(n)), "sgpu_wavelet_last_kernel_ms")
    return [(FORMS[what[k] // 100], what[k] // 10 % 10, what[k] % 10, float(ms[k])) for k in range(n.value)]


def _frames(frames, lead_dims=(3, 4)):
    import torch
    if frames.dim() not in lead_dims or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W] or [N, C, H, W]")
    if frames.dtype not in (torch.float32, torch.int16):
        raise ValueError("frames must be float32, or int16 holding WORD samples")


def _ctx(ctx, t):
    import torch
    from .stacking import Context
    ctx = ctx or Context(t.device.index or 0)
    ctx.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    return ctx


def atrous(frames, nbr_layers: int, type: int = 2, ctx=None):
    """W3 of CUDA frames [N, H, W] or [N, C, H, W] (float32, or 16-bit WORD
    storage as int16), every plane on its own: float32 [..., n, H, W] holding
    w_0 .. w_{n-2} and the residual c_{n-1}."""
    import torch
    _frames(frames)
    lead, (h, w) = tuple(frames.shape[:-2]), frames.shape[-2:]
    n = int(nbr_layers)
    check_layers(w, h, n, type)
    out = torch.empty(lead + (n, h, w), dtype=torch.float32, device=frames.device)
    atrous_device(_ctx(ctx, frames), frames.data_ptr(), frames.element_size(), int(np.prod(lead)), w, h, h * w, n,
                  int(type), out.data_ptr(), h * w, n * h * w)
    return out


def reconstruct(planes, coefs, out=None, ctx=None):
    """W4 of float32 CUDA planes [..., n, H, W] with n coefficients: float32 [..., H, W]."""
    import torch
    if planes.dim() not in (4, 5) or not planes.is_cuda or not planes.is_contiguous() or planes.dtype != torch.float32:
        raise ValueError("planes must be a contiguous float32 CUDA tensor [N, n, H, W] or [N, C, n, H, W]")
    lead, (n, h, w) = tuple(planes.shape[:-3]), planes.shape[-3:]
    if len(np.asarray(coefs).reshape(-1)) != n:
        raise ValueError(f"{n} planes need {n} coefficients")
    if out is None:
        out = torch.empty(lead + (h, w), dtype=torch.float32, device=planes.device)
    if tuple(out.shape) != lead + (h, w) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor [..., H, W]")
    reconstruct_device(_ctx(ctx, planes), planes.data_ptr(), int(np.prod(lead)), w, h, h * w, n * h * w, coefs,
                       out.data_ptr(), h * w)
    return out


def wrecons(frames, coefs, type: int = 2, out=None, ctx=None):
    """W5: reconstruct(atrous(frames, len(coefs), type), coefs) bit for bit in
    one pass over the scales, without writing a detail plane.  `out` (float32,
    shaped like frames) is allocated unless given and may not be `frames`."""
    import torch
    _frames(frames)
    lead, (h, w) = tuple(frames.shape[:-2]), frames.shape[-2:]
    n = len(np.asarray(coefs).reshape(-1))
    check_layers(w, h, n, type)
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_cuda or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    wrecons_device(_ctx(ctx, frames), frames.data_ptr(), frames.element_size(), int(np.prod(lead)), w, h, h * w, coefs,
                   int(type), out.data_ptr(), h * w)
    return out


# ------------------------------------------------------------------ commands
@dataclass
class WaveletCommand:
    image: str
    nbr_layers: int
    type: int
    prefix: str = ""


@dataclass
class WreconsCommand:
    image: str
    coefs: List[float] = field(default_factory=list)
    type: int = 2
    out: str = ""


def parse_wavelet_command(words: Sequence[str]) -> WaveletCommand:
    """`wavelet <image> <nbr_layers> <type> [-prefix=]`: nbr_layers 1 .. 6,
    type 1 (linear) or 2 (B3 spline)."""
    words = list(words)
    if words and words[0] == "wavelet":
        words = words[1:]
    if len(words) < 3 or any(w.startswith("-") for w in words[:3]):
        raise ValueError("wavelet needs an image, the number of layers (1 .. 6) and the type (1 or 2)")
    try:
        n, t = int(words[1]), int(words[2])
    except ValueError:
        raise ValueError(f"wavelet: the number of layers and the type must be integers, not `{words[1]} {words[2]}'") \
            from None
    if not 1 <= n <= MAX_LAYERS:
        raise ValueError("wavelet: the number of layers must be 1 .. 6")
    if t not in (1, 2):
        raise ValueError("wavelet: the type must be 1 (linear) or 2 (B3 spline)")
    cmd = WaveletCommand(image=words[0], nbr_layers=n, type=t)
    for o in words[3:]:
        if o.startswith("-prefix="):
            cmd.prefix = o[8:]
        else:
            raise ValueError(f"Unexpected argument to wavelet `{o}', aborting.")
    return cmd


def parse_wrecons_command(words: Sequence[str]) -> WreconsCommand:
    """`wrecons <image> c1 ... cn [-type=1|2] [-out=FILE]`: n = 1 .. 6 finite
    coefficients, finest scale first, the residual's last."""
    words = list(words)
    if words and words[0] == "wrecons":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("wrecons needs an image")
    cmd = WreconsCommand(image=words[0])
    options = False
    for o in words[1:]:
        if o.startswith("-type="):
            if o[6:] not in ("1", "2"):
                raise ValueError("wrecons: -type= must be 1 (linear) or 2 (B3 spline)")
            cmd.type = int(o[6:])
            options = True
        elif o.startswith("-out="):
            if not o[5:]:
                raise ValueError("wrecons: -out= needs a file name")
            cmd.out = o[5:]
            options = True
        else:
            try:
                v = float(o)
            except ValueError:
                raise ValueError(f"Unexpected argument to wrecons `{o}', aborting.") from None
            if options:
                raise ValueError("wrecons: the coefficients come before the options")
            if not (abs(v) <= float(np.finfo(np.float32).max)):      # finite as a float32 (NaN fails too)
                raise ValueError("wrecons: the coefficients must be finite")
            cmd.coefs.append(v)
    if not 1 <= len(cmd.coefs) <= MAX_LAYERS:
        raise ValueError("wrecons needs 1 .. 6 coefficients, one per layer")
    return cmd


def _image_path(image: str) -> str:
    if os.path.exists(image):
        return image
    for ext in (".fit", ".fits", ".fts"):
        if os.path.exists(image + ext):
            return image + ext
    raise ValueError(f"no such image: {image}")


def _load(path: str, ctx):
    import torch
    from .sequence import read_fits
    host = read_fits(path)
    t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host)
    return t.reshape((1,) + tuple(host.shape)).to(torch.device("cuda", ctx.device)).contiguous()


def run_wavelet(line, ctx=None):
    """Run one `wavelet` command line (a string or its words): reads the FITS
    image (16- or 32-bit, one or three layers) and writes its n planes as
    32-bit <prefix><stem>_wavelet<k>.fit, k = 1 .. n, each with the image's
    layers, next to the image.  Returns the list of paths."""
    from .sequence import write_fits
    from .stacking import Context
    cmd = parse_wavelet_command(line.split() if isinstance(line, str) else line)
    path = _image_path(cmd.image)
    ctx = ctx or Context(0)
    t = _load(path, ctx)
    try:
        planes = atrous(t, cmd.nbr_layers, cmd.type, ctx=ctx)
    except RuntimeError as e:
        raise ValueError(f"wavelet: {e}") from None
    planes = planes[0].cpu().numpy()        # [n, H, W] or [3, n, H, W]
    d, stem = os.path.dirname(os.path.abspath(path)), os.path.splitext(os.path.basename(path))[0]
    out = []
    for k in range(cmd.nbr_layers):
        out.append(os.path.join(d, f"{cmd.prefix}{stem}_wavelet{k + 1}.fit"))
        write_fits(out[-1], np.ascontiguousarray(planes[k] if planes.ndim == 3 else planes[:, k]))
    return out


def run_wrecons(line, ctx=None):
    """Run one `wrecons` command line: reads the FITS image, runs the fused
    transform and reconstruction with the given coefficients and writes one
    32-bit image, <stem>_wrecons.fit next to the input unless -out= names it.
    Returns its path."""
    from .sequence import write_fits
    from .stacking import Context
    cmd = parse_wrecons_command(line.split() if isinstance(line, str) else line)
    path = _image_path(cmd.image)
    ctx = ctx or Context(0)
    t = _load(path, ctx)
    try:
        res = wrecons(t, cmd.coefs, cmd.type, ctx=ctx)
    except RuntimeError as e:
        raise ValueError(f"wrecons: {e}") from None
    d, stem = os.path.dirname(os.path.abspath(path)), os.path.splitext(os.path.basename(path))[0]
    out = cmd.out or os.path.join(d, stem + "_wrecons.fit")
    write_fits(out, res[0].cpu().numpy())
    return out

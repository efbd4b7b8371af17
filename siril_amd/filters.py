"""The median filter on the GPU (Siril's `fmedian ksize modulation`,
filters/median): every sample becomes the median of the ksize x ksize window
around it, blended with the sample itself by `modulation`, `iterations` times.

    clean = fmedian(frames, 3)                    # [N, H, W] or [N, C, H, W]
    soft = fmedian(frames, 5, modulation=0.6, iterations=2)

The kernels are siril_amd/csrc/median.hip behind the C-ABI
(`sgpu_fmedian_planes_device`); the filter is the specification in DESIGN.md
6l (M0-M5), restated in tests/median_ref.py: windows reflected at the edges,
samples ordered by their keys (NaN and the sign of zero included), the median
returned with its own bits.  Parity with a Siril binary is unpinned.

Headless: `python -m siril_amd.cli fmedian <image> <ksize> <modulation>
[-iter=N] [-out=FILE]` (`run_fmedian`).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from ._lib import check, lib

MIN_KSIZE, MAX_KSIZE, MAX_ITERATIONS = 3, 15, 8
MAX_LAUNCHES = 8
# `route`: 0 is what an application passes.  The others exist so that the two
# routes can be compared bit for bit and timed against each other.
ROUTE_AUTO, ROUTE_NETWORK, ROUTE_SELECT, ROUTE_SELECT_WIDE = 0, 1, 2, 3
ROUTES = ("auto", "network", "select", "select-wide")
MAX_NETWORK_KSIZE = 7


def check_fmedian(w: int, h: int, ksize: int, modulation: float = 1.0, iterations: int = 1) -> None:
    """M5's refusals (SgpuError): ksize even or outside 3 .. 15, a w x h plane
    smaller than the window's radius + 1, modulation not finite or outside
    [0, 1], iterations outside 1 .. 8, a side above 65535."""
    check(lib().sgpu_fmedian_check(int(w), int(h), int(ksize), float(modulation), int(iterations)),
          "sgpu_fmedian_check")


def _vp(p):
    return C.c_void_p(p) if p else None


def fmedian_device(ctx, d_in: int, elem_size: int, nplanes: int, w: int, h: int, plane_stride: int, ksize: int,
                   modulation: float, iterations: int, d_out: int, out_stride: int, route: int = ROUTE_AUTO):
    """sgpu_fmedian_planes_device on raw device pointers; asynchronous."""
    check(lib().sgpu_fmedian_planes_device(ctx.h, _vp(d_in), elem_size, nplanes, w, h, plane_stride, int(ksize),
                                           float(modulation), int(iterations), int(route), _vp(d_out), out_stride),
          "sgpu_fmedian_planes_device")


def last_kernel_ms(ctx) -> list:
    """[(route, ksize, ms)] of the launches (one per iteration) of the
    context's last fmedian call; route is one of ROUTES."""
    ms, what, n = (C.c_float * MAX_LAUNCHES)(), (C.c_int * MAX_LAUNCHES)(), C.c_int(0)
    check(lib().sgpu_fmedian_last_kernel_ms(ctx.h, ms, what, C.byref(n)), "sgpu_fmedian_last_kernel_ms")
    return [(ROUTES[what[k] // 100], what[k] % 100, float(ms[k])) for k in range(n.value)]


def fmedian(frames, ksize: int, modulation: float = 1.0, iterations: int = 1, out=None, ctx=None,
            route: int = ROUTE_AUTO):
    """M0-M4 of CUDA frames [N, H, W] or [N, C, H, W] (float32, or 16-bit WORD
    storage as int16), every plane on its own: float32, shaped like frames.
    `out` is allocated unless given and may not be `frames`."""
    import torch
    from .wavelets import _ctx, _frames
    _frames(frames)
    lead, (h, w) = tuple(frames.shape[:-2]), frames.shape[-2:]
    check_fmedian(w, h, ksize, modulation, iterations)
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_cuda or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    fmedian_device(_ctx(ctx, frames), frames.data_ptr(), frames.element_size(), int(np.prod(lead)), w, h, h * w, ksize,
                   modulation, iterations, out.data_ptr(), h * w, route)
    return out


# ------------------------------------------------------------------ command
@dataclass
class FmedianCommand:
    image: str
    ksize: int
    modulation: float
    iterations: int = 1
    out: str = ""


def parse_fmedian_command(words: Sequence[str]) -> FmedianCommand:
    """`fmedian <image> <ksize> <modulation> [-iter=N] [-out=FILE]`: ksize odd
    in 3 .. 15, modulation in [0, 1], N in 1 .. 8."""
    words = list(words)
    if words and words[0] == "fmedian":
        words = words[1:]
    if len(words) < 3 or any(w.startswith("-") for w in words[:3]):
        raise ValueError("fmedian needs an image, the window size (odd, 3 .. 15) and the modulation (0 .. 1)")
    try:
        ksize = int(words[1])
    except ValueError:
        raise ValueError(f"fmedian: the window size must be an integer, not `{words[1]}'") from None
    try:
        modulation = float(words[2])
    except ValueError:
        raise ValueError(f"fmedian: the modulation must be a number, not `{words[2]}'") from None
    if not MIN_KSIZE <= ksize <= MAX_KSIZE or ksize % 2 == 0:
        raise ValueError("fmedian: the window size must be odd, 3 .. 15")
    if math.isnan(modulation) or not 0.0 <= modulation <= 1.0:
        raise ValueError("fmedian: the modulation must be in [0, 1]")
    cmd = FmedianCommand(image=words[0], ksize=ksize, modulation=modulation)
    for o in words[3:]:
        if o.startswith("-iter="):
            try:
                cmd.iterations = int(o[6:])
            except ValueError:
                raise ValueError(f"fmedian: -iter= needs an integer, not `{o[6:]}'") from None
            if not 1 <= cmd.iterations <= MAX_ITERATIONS:
                raise ValueError("fmedian: -iter= must be 1 .. 8")
        elif o.startswith("-out="):
            if not o[5:]:
                raise ValueError("fmedian: -out= needs a file name")
            cmd.out = o[5:]
        else:
            raise ValueError(f"Unexpected argument to fmedian `{o}', aborting.")
    return cmd


def run_fmedian(line, ctx=None):
    """Run one `fmedian` command line (a string or its words): reads the FITS
    image (16- or 32-bit, one or three layers), filters every layer and writes
    one 32-bit image, <stem>_fmedian.fit next to the input unless -out= names
    it.  Returns its path."""
    from .sequence import write_fits
    from .stacking import Context
    from .wavelets import _image_path, _load
    cmd = parse_fmedian_command(line.split() if isinstance(line, str) else line)
    path = _image_path(cmd.image)
    ctx = ctx or Context(0)
    t = _load(path, ctx)
    try:
        res = fmedian(t, cmd.ksize, cmd.modulation, cmd.iterations, ctx=ctx)
    except RuntimeError as e:
        raise ValueError(f"fmedian: {e}") from None
    d, stem = os.path.dirname(os.path.abspath(path)), os.path.splitext(os.path.basename(path))[0]
    out = cmd.out or os.path.join(d, stem + "_fmedian.fit")
    write_fits(out, res[0].cpu().numpy())
    return out

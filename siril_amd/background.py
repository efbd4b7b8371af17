"""Polynomial background extraction on the GPU (Siril's `seqsubsky <seq>
<degree>`, filters/background_extraction.c): per plane, the medians of a grid
of 25 x 25 sample boxes, the selection of the boxes that hold sky, a
least-squares polynomial of degree 1 .. 4 through them, and its subtraction
(or division) with the model's mean put back.

    out, info = subsky(frames, degree=1, samples=20, tolerance=1.0)

The kernels are siril_amd/csrc/background.hip behind the C-ABI
(`sgpu_subsky_planes_device`); the arithmetic is the specification in DESIGN.md
6i (B0-B7), restated in tests/bkg_ref.py.  Parity with a Siril binary is
unpinned.

Thin-plate-spline model (Siril's `subsky -rbf`): the same boxes and selection,
a spline phi = r^2 log r with a constant term through the kept boxes, smoothed
on the diagonal, evaluated at every pixel in double.

    out, info = subsky_rbf(frames, samples=20, tolerance=1.0, smooth=0.5)

Its kernels are siril_amd/csrc/background_rbf.hip
(`sgpu_subsky_rbf_planes_device`); the arithmetic is DESIGN.md 6k (R0-R7),
restated in tests/bkg_rbf_ref.py, parity with a Siril binary unpinned.

Headless: `python -m siril_amd.cli seqsubsky <seq> <degree> [-samples=20]
[-tolerance=1.0] [-nodither] [-prefix=bkg_]` (`run_seqsubsky`, polynomial
only) and `python -m siril_amd.cli subsky <image> {-rbf | <degree>}
[-samples=20] [-tolerance=1.0] [-smooth=0.5] [-nodither] [-divide]
[-out=FILE]` (`run_subsky`).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from ._lib import BkgParams, check, lib

NCOEF = 15
STATUS_TEXT = {1: "fewer sample boxes kept than coefficients", 2: "the normal matrix is not positive definite"}
RBF_MAX_SAMPLES = 1024
RBF_STATUS_TEXT = {1: "no sample box kept", 2: "the spline system is singular"}


def sample_grid(w: int, h: int, samples: int = 20) -> dict:
    """B1: nx, ny, dist, startx, starty and K = nx * ny of a w x h plane
    (SgpuError for a plane smaller than a box, samples < 1 or > w, K > 8192)."""
    v = [C.c_int(0) for _ in range(5)]
    check(lib().sgpu_bkg_grid(int(w), int(h), int(samples), *[C.byref(x) for x in v]), "sgpu_bkg_grid")
    nx, ny, dist, sx, sy = (int(x.value) for x in v)
    return dict(nx=nx, ny=ny, dist=dist, startx=sx, starty=sy, K=nx * ny)


def _params(degree, samples, tolerance, divide) -> BkgParams:
    p = BkgParams()
    lib().sgpu_bkg_default_params(C.byref(p))
    p.degree, p.samples, p.tolerance, p.divide = int(degree), int(samples), float(tolerance), int(bool(divide))
    return p


def subsky_device(ctx, d_in: int, elem_size: int, nplanes: int, w: int, h: int, plane_stride: int, params: BkgParams,
                  d_out: int, d_med=None, d_keep=None, d_coef=None, d_mean=None, d_kept=None, d_status=None):
    """sgpu_subsky_planes_device on raw device pointers (plane p at base +
    p*plane_stride samples, in and out); asynchronous."""
    vp = [C.c_void_p(x) if x else None for x in (d_med, d_keep, d_coef, d_mean, d_kept, d_status)]
    check(lib().sgpu_subsky_planes_device(ctx.h, C.c_void_p(d_in) if d_in else None, elem_size, nplanes, w, h,
                                          plane_stride, C.byref(params), C.c_void_p(d_out) if d_out else None, *vp),
          "sgpu_subsky_planes_device")


def last_kernel_ms(ctx) -> tuple:
    """(box medians, fit, streaming pass) kernel times of the context's last call, in ms."""
    ms = (C.c_float * 3)()
    check(lib().sgpu_bkg_last_kernel_ms(ctx.h, ms), "sgpu_bkg_last_kernel_ms")
    return float(ms[0]), float(ms[1]), float(ms[2])


def subsky(frames, degree: int = 1, samples: int = 20, tolerance: float = 1.0, divide: bool = False, out=None,
           ctx=None, strict: bool = True):
    """Remove the polynomial background of CUDA frames [N, H, W] or
    [N, C, H, W] (float32, or 16-bit WORD storage as int16), every plane on its
    own, into float32 `out` (allocated unless given; `frames` itself is allowed
    for float32 input).  Returns (out, info): info holds numpy arrays shaped
    like the leading dimensions -- med [.., K] float32, keep [.., K] uint8,
    coef [.., 15] float64, mean, kept, status -- and grid (sample_grid).
    strict: raise ValueError for the first plane whose status is not 0."""
    import torch
    from .stacking import Context
    if frames.dim() not in (3, 4) or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W] or [N, C, H, W]")
    if frames.dtype not in (torch.float32, torch.int16):
        raise ValueError("frames must be float32, or int16 holding WORD samples")
    ctx = ctx or Context(frames.device.index or 0)
    lead, (h, w) = tuple(frames.shape[:-2]), frames.shape[-2:]
    P = int(np.prod(lead))
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_cuda or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    grid = sample_grid(w, h, samples)
    K = grid["K"]
    dev = frames.device
    med = torch.empty((P, K), dtype=torch.float32, device=dev)
    keep = torch.empty((P, K), dtype=torch.uint8, device=dev)
    coef = torch.empty((P, NCOEF), dtype=torch.float64, device=dev)
    mean = torch.empty(P, dtype=torch.float64, device=dev)
    kept = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    subsky_device(ctx, frames.data_ptr(), frames.element_size(), P, w, h, h * w,
                  _params(degree, samples, tolerance, divide), out.data_ptr(), med.data_ptr(), keep.data_ptr(),
                  coef.data_ptr(), mean.data_ptr(), kept.data_ptr(), status.data_ptr())
    info = dict(med=med.cpu().numpy().reshape(lead + (K,)), keep=keep.cpu().numpy().reshape(lead + (K,)),
                coef=coef.cpu().numpy().reshape(lead + (NCOEF,)), mean=mean.cpu().numpy().reshape(lead),
                kept=kept.cpu().numpy().reshape(lead), status=status.cpu().numpy().reshape(lead), grid=grid)
    if strict and P and info["status"].any():
        idx = tuple(int(v) for v in np.argwhere(info["status"] != 0)[0])
        st = int(info["status"][idx])
        raise ValueError(f"subsky: plane {idx}: status {st} ({STATUS_TEXT.get(st, '?')}), "
                         f"{int(info['kept'][idx])} of {K} boxes kept")
    return out, info


# ------------------------------------------------------------------ thin-plate spline
def rbf_check(w: int, h: int, samples: int = 20, tolerance: float = 1.0, smooth: float = 0.5) -> None:
    """R0's refusals (SgpuError): the grid's, more than 1024 boxes, a bad tolerance, smooth outside [0, 1]."""
    check(lib().sgpu_bkg_rbf_check(int(w), int(h), int(samples), float(tolerance), float(smooth)), "sgpu_bkg_rbf_check")


def subsky_rbf_device(ctx, d_in: int, elem_size: int, nplanes: int, w: int, h: int, plane_stride: int, samples: int,
                      tolerance: float, smooth: float, divide: bool, d_out: int, d_med=None, d_keep=None,
                      d_weights=None, d_mean=None, d_kept=None, d_status=None) -> float:
    """sgpu_subsky_rbf_planes_device on raw device pointers (plane p at base +
    p*plane_stride samples, in and out); asynchronous.  Returns lam_rel."""
    vp = [C.c_void_p(x) if x else None for x in (d_med, d_keep, d_weights, d_mean, d_kept, d_status)]
    lam = C.c_double(0.0)
    check(lib().sgpu_subsky_rbf_planes_device(ctx.h, C.c_void_p(d_in) if d_in else None, elem_size, nplanes, w, h,
                                              plane_stride, int(samples), float(tolerance), float(smooth),
                                              int(bool(divide)), C.c_void_p(d_out) if d_out else None, *vp,
                                              C.byref(lam)), "sgpu_subsky_rbf_planes_device")
    return float(lam.value)


def rbf_last_kernel_ms(ctx) -> tuple:
    """(box medians, selection + system + solve, evaluation pass, whole call) of the context's last
    subsky_rbf call, in ms."""
    ms = (C.c_float * 4)()
    check(lib().sgpu_bkg_rbf_last_kernel_ms(ctx.h, ms), "sgpu_bkg_rbf_last_kernel_ms")
    return tuple(float(v) for v in ms)


def subsky_rbf(frames, samples: int = 20, tolerance: float = 1.0, smooth: float = 0.5, divide: bool = False,
               out=None, ctx=None, strict: bool = True):
    """Remove the thin-plate-spline background of CUDA frames, with subsky's
    tensor rules.  Returns (out, info): med [.., K] float32, keep [.., K] uint8,
    weights [.., 1025] float64 (the weights in the order of the kept boxes,
    the constant, then +0), mean (of the kept medians), kept, status, grid and
    lam_rel (the double the kernels were given).  strict: raise ValueError for
    the first plane whose status is not 0."""
    import torch
    from .stacking import Context
    if frames.dim() not in (3, 4) or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W] or [N, C, H, W]")
    if frames.dtype not in (torch.float32, torch.int16):
        raise ValueError("frames must be float32, or int16 holding WORD samples")
    ctx = ctx or Context(frames.device.index or 0)
    lead, (h, w) = tuple(frames.shape[:-2]), frames.shape[-2:]
    P = int(np.prod(lead))
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    if tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_cuda or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor shaped like frames")
    rbf_check(w, h, samples, tolerance, smooth)
    grid = sample_grid(w, h, samples)
    K, NW = grid["K"], RBF_MAX_SAMPLES + 1
    dev = frames.device
    med = torch.empty((P, K), dtype=torch.float32, device=dev)
    keep = torch.empty((P, K), dtype=torch.uint8, device=dev)
    weights = torch.empty((P, NW), dtype=torch.float64, device=dev)
    mean = torch.empty(P, dtype=torch.float64, device=dev)
    kept = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    lam_rel = subsky_rbf_device(ctx, frames.data_ptr(), frames.element_size(), P, w, h, h * w, samples, tolerance,
                                smooth, divide, out.data_ptr(), med.data_ptr(), keep.data_ptr(), weights.data_ptr(),
                                mean.data_ptr(), kept.data_ptr(), status.data_ptr())
    info = dict(med=med.cpu().numpy().reshape(lead + (K,)), keep=keep.cpu().numpy().reshape(lead + (K,)),
                weights=weights.cpu().numpy().reshape(lead + (NW,)), mean=mean.cpu().numpy().reshape(lead),
                kept=kept.cpu().numpy().reshape(lead), status=status.cpu().numpy().reshape(lead), grid=grid,
                lam_rel=lam_rel)
    if strict and P and info["status"].any():
        idx = tuple(int(v) for v in np.argwhere(info["status"] != 0)[0])
        st = int(info["status"][idx])
        raise ValueError(f"subsky -rbf: plane {idx}: status {st} ({RBF_STATUS_TEXT.get(st, '?')}), "
                         f"{int(info['kept'][idx])} of {K} boxes kept")
    return out, info


def rbf_solve(aug, ctx=None):
    """R4 alone: `aug` is a CUDA float64 tensor [nsys, order, order + 1] (or
    [order, order + 1]) of systems [A | rhs]; a copy is worked on.  Returns
    (x float64 [nsys, order], status int32 [nsys]) as numpy arrays: status 2
    and x = +0 for a pivot that is 0 or not finite."""
    import torch
    from .stacking import Context
    if aug.dim() == 2:
        aug = aug.unsqueeze(0)
    if aug.dim() != 3 or not aug.is_cuda or aug.dtype != torch.float64 or aug.shape[2] != aug.shape[1] + 1:
        raise ValueError("aug must be a CUDA float64 tensor [nsys, order, order + 1]")
    ctx = ctx or Context(aug.device.index or 0)
    nsys, order = int(aug.shape[0]), int(aug.shape[1])
    work = aug.contiguous().clone()
    x = torch.empty((nsys, order), dtype=torch.float64, device=aug.device)
    status = torch.empty(nsys, dtype=torch.int32, device=aug.device)
    ctx.set_stream(torch.cuda.current_stream(aug.device).cuda_stream)
    check(lib().sgpu_bkg_rbf_solve_device(ctx.h, nsys, order, C.c_void_p(work.data_ptr()), C.c_void_p(x.data_ptr()),
                                          C.c_void_p(status.data_ptr())), "sgpu_bkg_rbf_solve_device")
    return x.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------ command
@dataclass
class SeqSubskyCommand:
    seq: str
    degree: int = 1
    samples: int = 20
    tolerance: float = 1.0
    prefix: str = "bkg_"


def parse_seqsubsky_command(words: Sequence[str]) -> SeqSubskyCommand:
    """`seqsubsky <seq> <degree> [-samples=20] [-tolerance=1.0] [-nodither]
    [-prefix=bkg_]`.  -nodither is accepted and changes nothing (the output is
    always 32-bit); -rbf and -smooth= are refused."""
    words = list(words)
    if words and words[0] == "seqsubsky":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("seqsubsky needs a sequence name")
    if len(words) < 2 or words[1].startswith("-"):
        if len(words) > 1 and words[1] == "-rbf":
            raise ValueError("-rbf is not supported by this seqsubsky (polynomial models only)")
        raise ValueError("seqsubsky needs the polynomial degree (1 .. 4) after the sequence name")
    try:
        degree = int(words[1])
    except ValueError:
        raise ValueError(f"seqsubsky: the degree must be an integer 1 .. 4, not `{words[1]}'") from None
    if not 1 <= degree <= 4:
        raise ValueError("seqsubsky: the degree must be 1 .. 4")
    cmd = SeqSubskyCommand(seq=words[0], degree=degree)
    for o in words[2:]:
        if o.startswith("-samples="):
            cmd.samples = int(o[9:])
            if cmd.samples < 1:
                raise ValueError("seqsubsky: -samples= must be at least 1")
        elif o.startswith("-tolerance="):
            cmd.tolerance = float(o[11:])
            if not (cmd.tolerance >= 0.0 and np.isfinite(cmd.tolerance)):
                raise ValueError("seqsubsky: -tolerance= must be finite and >= 0")
        elif o == "-nodither":
            pass
        elif o.startswith("-prefix="):
            cmd.prefix = o[8:]
        elif o == "-rbf" or o.startswith("-smooth="):
            raise ValueError(f"{o.split('=')[0]} is not supported by this seqsubsky (polynomial models only)")
        else:
            raise ValueError(f"Unexpected argument to seqsubsky `{o}', aborting.")
    return cmd


def run_seqsubsky(line, ctx=None, max_batch_bytes: int = 1 << 30):
    """Run one `seqsubsky` command line (a string or its words): reads the
    regular FITS sequence (16- or 32-bit, one or three layers), works in
    batches of at most max_batch_bytes of output, writes 32-bit
    <prefix><name>NNNNN.fit and <prefix><name>.seq.  A plane whose fit fails
    raises, naming the frame, before the .seq is written.  Returns (path of
    the new .seq, info) with info["kept"] and info["status"] per frame (and
    layer)."""
    import torch
    from .calibration import _read_seq
    from .sequence import frame_name, read_fits, write_fits, write_seq
    from .stacking import Context
    cmd = parse_seqsubsky_command(line.split() if isinstance(line, str) else line)
    seq = cmd.seq if cmd.seq.endswith(".seq") else cmd.seq + ".seq"
    d = os.path.dirname(os.path.abspath(seq))
    try:
        name, fixed, nums = _read_seq(seq)
    except ValueError as e:
        raise ValueError(str(e).replace("calibrate", "seqsubsky")) from None
    if not nums or nums != list(range(nums[0], nums[0] + len(nums))):
        raise ValueError("seqsubsky needs consecutively numbered images")
    ctx = ctx or Context(0)
    first = read_fits(os.path.join(d, frame_name(name, nums[0], fixed)))
    shape = first.shape
    nl = 1 if first.ndim == 2 else shape[0]
    batch = max(1, int(max_batch_bytes // (int(np.prod(shape)) * 4)))
    dev = torch.device("cuda", ctx.device)
    kept, status = [], []
    for b0 in range(0, len(nums), batch):
        part = nums[b0:b0 + batch]
        host = np.stack([first if (b0 == 0 and j == 0) else read_fits(os.path.join(d, frame_name(name, num, fixed)))
                         for j, num in enumerate(part)])
        if host.shape[1:] != shape:
            raise ValueError("frames of different sizes")
        t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
        res, info = subsky(t, cmd.degree, cmd.samples, cmd.tolerance, ctx=ctx, strict=False)
        if info["status"].any():
            idx = np.argwhere(info["status"] != 0)[0]
            st = int(info["status"][tuple(idx)])
            raise ValueError(f"seqsubsky: {frame_name(name, part[int(idx[0])], fixed)}"
                             + (f" layer {int(idx[1])}" if nl > 1 else "")
                             + f": background fit failed, status {st} ({STATUS_TEXT.get(st, '?')})")
        res = res.cpu().numpy()
        for j, num in enumerate(part):
            write_fits(os.path.join(d, frame_name(cmd.prefix + name, num, fixed)), res[j])
        kept.append(info["kept"])
        status.append(info["status"])
    out_seq = os.path.join(d, cmd.prefix + name + ".seq")
    write_seq(out_seq, cmd.prefix + name, len(nums), beg=nums[0], fixed=fixed, nb_layers=nl)
    return out_seq, dict(kept=np.concatenate(kept), status=np.concatenate(status))


@dataclass
class SubskyCommand:
    image: str
    rbf: bool = False
    degree: int = 0
    samples: int = 20
    tolerance: float = 1.0
    smooth: float = 0.5
    divide: bool = False
    out: str = ""


def parse_subsky_command(words: Sequence[str]) -> SubskyCommand:
    """`subsky <image> {-rbf | <degree>} [-samples=20] [-tolerance=1.0]
    [-smooth=0.5] [-nodither] [-divide] [-out=FILE]`.  -nodither is accepted
    and changes nothing (the output is always 32-bit); -smooth= without -rbf,
    -dither and unknown words are refused."""
    words = list(words)
    if words and words[0] == "subsky":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("subsky needs an image")
    if len(words) < 2:
        raise ValueError("subsky needs -rbf or the polynomial degree (1 .. 4) after the image")
    cmd = SubskyCommand(image=words[0])
    if words[1] == "-rbf":
        cmd.rbf = True
    else:
        try:
            cmd.degree = int(words[1])
        except ValueError:
            raise ValueError(f"subsky: -rbf or an integer degree 1 .. 4 comes after the image, not `{words[1]}'") from None
        if not 1 <= cmd.degree <= 4:
            raise ValueError("subsky: the degree must be 1 .. 4")
    smooth_given = False
    for o in words[2:]:
        try:
            if o.startswith("-samples="):
                cmd.samples = int(o[9:])
                if cmd.samples < 1:
                    raise ValueError("subsky: -samples= must be at least 1")
            elif o.startswith("-tolerance="):
                cmd.tolerance = float(o[11:])
                if not (cmd.tolerance >= 0.0 and np.isfinite(cmd.tolerance)):
                    raise ValueError("subsky: -tolerance= must be finite and >= 0")
            elif o.startswith("-smooth="):
                cmd.smooth = float(o[8:])
                smooth_given = True
                if not 0.0 <= cmd.smooth <= 1.0:
                    raise ValueError("subsky: -smooth= must be in [0, 1]")
            elif o == "-nodither":
                pass
            elif o == "-divide":
                cmd.divide = True
            elif o.startswith("-out="):
                if not o[5:]:
                    raise ValueError("subsky: -out= needs a file name")
                cmd.out = o[5:]
            else:
                raise ValueError(f"Unexpected argument to subsky `{o}', aborting.")
        except ValueError as e:
            if "subsky" in str(e):
                raise
            raise ValueError(f"subsky: bad number in `{o}'") from None
    if smooth_given and not cmd.rbf:
        raise ValueError("subsky: -smooth= belongs to -rbf")
    return cmd


def run_subsky(line, ctx=None):
    """Run one `subsky` command line (a string or its words): reads the FITS
    image (16- or 32-bit, one or three layers), removes the background of every
    layer on its own -- the polynomial of the given degree, or the thin-plate
    spline with -rbf -- and writes one 32-bit image, <stem>_subsky.fit next to
    the input unless -out= names it.  A layer whose fit fails raises.  Returns
    (path, info) with the call's info."""
    from .sequence import write_fits
    from .stacking import Context
    from .wavelets import _image_path, _load
    cmd = parse_subsky_command(line.split() if isinstance(line, str) else line)
    path = _image_path(cmd.image)
    ctx = ctx or Context(0)
    t = _load(path, ctx)
    try:
        if cmd.rbf:
            res, info = subsky_rbf(t, cmd.samples, cmd.tolerance, cmd.smooth, cmd.divide, ctx=ctx)
        else:
            res, info = subsky(t, cmd.degree, cmd.samples, cmd.tolerance, cmd.divide, ctx=ctx)
    except RuntimeError as e:
        raise ValueError(f"subsky: {e}") from None
    d, stem = os.path.dirname(os.path.abspath(path)), os.path.splitext(os.path.basename(path))[0]
    out = cmd.out or os.path.join(d, stem + "_subsky.fit")
    write_fits(out, res[0].cpu().numpy())
    return out, info

"""Host-side mirror of Siril's DFT registration entry (REG_DFT) over the
C-ABI.

  * `register_shift_dft`  -- registration/shift_methods.c:60-321: shifts of
                              every frame against the reference frame on a
                              square selection, as Siril computes them
  * `set_shifts` / `translation_from_H` / `H_from_translation`
                            -- io/sequence.c:1863-1868, registration.c:301-313
  * `find_stars` / `match_stars` / `register_stars` / `run_register`
                            -- star detection and star-based global
                              registration (modelled on Siril's
                              star finder and matcher, parity unpinned)
  * `fit_stars`             -- Gaussian / Moffat PSF fit of the found stars
                              (parity unpinned)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._lib import check, lib


def H_from_translation(dx: float, dy: float) -> np.ndarray:
    """registration.c:306-313: identity with h02 = dx, h12 = -dy."""
    H = np.eye(3)
    H[0, 2] = dx
    H[1, 2] = -dy
    return H


def translation_from_H(H) -> tuple:
    """registration.c:301-304: dx = h02, dy = -h12."""
    return float(H[0][2]), float(-H[1][2])


def set_shifts(shiftx: float, shifty: float, top_down: bool = False) -> np.ndarray:
    """io/sequence.c:1863-1868: H of a (shiftx, shifty) registration."""
    return H_from_translation(shiftx, -shifty if top_down else shifty)


# filter_pattern strings (algos/demosaicing.c:54-73) for the 2x2 Bayer cases
BAYER_PATTERNS = {"RGGB": 0, "BGGR": 1, "GBRG": 2, "GRBG": 3}


def compiled_pattern(pattern: str) -> np.ndarray:
    """get_compiled_pattern (algos/demosaicing.c:327-341) of a 2x2 Bayer
    string (or a 36-letter X-Trans string): R 0, G 1, B 2."""
    m = {"R": 0, "G": 1, "B": 2}
    if len(pattern) not in (4, 36):
        raise ValueError("CFA pattern must have 4 (Bayer) or 36 (X-Trans) letters")
    return np.array([m.get(ch, 3) for ch in pattern.upper()], np.uint8)


def _cfa_args(cfa):
    if cfa is None:
        return None, 0
    pat = compiled_pattern(cfa) if isinstance(cfa, str) else np.ascontiguousarray(cfa, np.uint8).ravel()
    dim = {4: 2, 36: 6}.get(pat.size)
    if dim is None:
        raise ValueError("CFA pattern must have 4 or 36 entries")
    return pat, dim


def _is16(t):
    import torch
    return t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))


def interpolate_nongreen(img, cfa, ctx=None):
    """interpolate_nongreen (io/image_format_fits.c:4389-4401) in place on a
    torch.cuda 2-D tensor: float32 -> interpolate_nongreen_float (:4319-4349),
    16-bit WORD storage -> interpolate_nongreen_ushort (:4351-4381)."""
    import torch
    from .stacking import default_context
    ctx = ctx or default_context()
    pat, dim = _cfa_args(cfa)
    u16 = _is16(img)
    if (img.dtype != torch.float32 and not u16) or img.dim() != 2 or img.stride(1) != 1:
        raise TypeError("img must be a 2-D float32 or 16-bit tensor with unit column stride")
    ctx.set_stream(torch.cuda.current_stream(img.device).cuda_stream)
    name = "sgpu_interpolate_nongreen_u16_device" if u16 else "sgpu_interpolate_nongreen_device"
    check(getattr(lib(), name)(ctx.h, C.c_void_p(img.data_ptr()), img.shape[1], img.shape[0], img.stride(0),
                               pat.ctypes.data_as(C.c_void_p), dim), name)
    return img


def dft_shifts(ref: np.ndarray, frames: Sequence[np.ndarray], ctx=None, cfa=None) -> np.ndarray:
    """(nframes, 2) int array of (shiftx, shifty), host selections (S x S).
    `cfa`: Bayer string / compiled pattern of a CFA (one-layer) sequence."""
    from .stacking import default_context
    ctx = ctx or default_context()
    u16 = np.asarray(ref).dtype == np.uint16          # DATA_USHORT selections
    dt = np.uint16 if u16 else np.float32
    ref = np.ascontiguousarray(ref, dt)
    S = ref.shape[0]
    if ref.shape != (S, S):
        raise ValueError("DFT registration needs a square selection (shift_methods.c:75)")
    fr = [np.ascontiguousarray(f, dt) for f in frames]
    for f in fr:
        if f.shape != (S, S):
            raise ValueError("all selections must be S x S")
    ptrs = (C.c_void_p * len(fr))(*[f.ctypes.data for f in fr])
    sx = np.zeros(len(fr), np.int32)
    sy = np.zeros(len(fr), np.int32)
    pat, dim = _cfa_args(cfa)
    name = "sgpu_dft_shifts_u16" if u16 else "sgpu_dft_shifts_cfa"
    check(getattr(lib(), name)(ctx.h, ref.ctypes.data_as(C.c_void_p), ptrs, len(fr), S,
                               pat.ctypes.data_as(C.c_void_p) if pat is not None else None, dim,
                               sx.ctypes.data_as(C.c_void_p), sy.ctypes.data_as(C.c_void_p)), name)
    return np.stack([sx, sy], 1)


def register_shift_dft(frames, ref_index: int, selection, ctx=None, peaks: bool = False, cfa=None):
    """Device path: frames is a torch.cuda tensor [N, H, W] (one layer; float32,
    or int16 / uint16 storage of DATA_USHORT WORD samples),
    selection = (x, y, w, h) with w == h.  Returns a (N, 2) int tensor of
    (shiftx, shifty); the reference frame gets (0, 0) like set_shifts(ref, 0, 0)
    (shift_methods.c:182)."""
    import torch
    from .stacking import default_context
    ctx = ctx or default_context()
    x, y, w, h = selection
    if w != h:
        raise ValueError("DFT registration needs a square selection (shift_methods.c:75)")
    n, H, W = frames.shape
    if x < 0 or y < 0 or x + w > W or y + h > H:
        raise ValueError("selection outside the frames")
    base = frames[:, y:y + h, x:x + w]
    shifts = torch.zeros((n, 2), dtype=torch.int32, device=frames.device)
    pk = torch.zeros(n, dtype=torch.float32, device=frames.device) if peaks else None
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    ref = base[ref_index]
    pat, dim = _cfa_args(cfa)
    # float32 frames, or 16-bit WORD storage (DATA_USHORT sequences)
    name = "sgpu_dft_register_u16_device" if _is16(frames) else "sgpu_dft_register_cfa_device"
    check(getattr(lib(), name)(ctx.h, C.c_void_p(ref.data_ptr()), W, C.c_void_p(base.data_ptr()), W,
                               frames.stride(0), n, w,
                               pat.ctypes.data_as(C.c_void_p) if pat is not None else None, dim,
                               C.c_void_p(shifts.data_ptr()), C.c_void_p(pk.data_ptr()) if peaks else None), name)
    shifts[ref_index] = 0
    return (shifts, pk) if peaks else shifts


def quality_estimate(frames, ctx=None) -> np.ndarray:
    """QualityEstimate (algos/quality.c:39-45) of every image of `frames`
    [N, h, w]: float32 -> QualityEstimate_float (algos/quality_float.c:41-147),
    uint16 (DATA_USHORT) -> QualityEstimate_ushort (algos/quality.c:49-276).
    numpy, or a torch.cuda tensor (float32, or int16 / uint16 storage of WORD
    samples) whose rows may be a window of larger frames.  Unnormalised
    qualities, f64."""
    from .stacking import default_context
    ctx = ctx or default_context()
    if isinstance(frames, np.ndarray):
        u16 = frames.dtype == np.uint16
        fr = np.ascontiguousarray(frames, np.uint16 if u16 else np.float32)
        n, h, w = fr.shape
        q = np.zeros(n, np.float64)
        name = "sgpu_quality_estimate_u16" if u16 else "sgpu_quality_estimate"
        check(getattr(lib(), name)(ctx.h, fr.ctypes.data_as(C.c_void_p), n, w, h,
                                   q.ctypes.data_as(C.c_void_p)), name)
        return q
    import torch
    n, h, w = frames.shape
    u16 = frames.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))
    assert (frames.dtype == torch.float32 or u16) and frames.stride(2) == 1
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    q = np.zeros(n, np.float64)
    name = "sgpu_quality_estimate_u16_device" if u16 else "sgpu_quality_estimate_device"
    check(getattr(lib(), name)(ctx.h, C.c_void_p(frames.data_ptr()), n, w, h, frames.stride(1),
                               frames.stride(0), q.ctypes.data_as(C.c_void_p)), name)
    return q


def normalize_quality(quality, ref_index: int):
    """register_shift_dft's q_min / q_max / best-frame tracking (seeded with
    the reference frame, shift_methods.c:184,241-246) and normalizeQualityData
    (:36-54).  Returns (normalised qualities, best frame index)."""
    q = np.array(quality, np.float64)
    q_min = q_max = q[ref_index]
    q_index = ref_index
    for i, v in enumerate(q):
        if i == ref_index:
            continue
        if v > q_max:
            q_max, q_index = v, i
        q_min = q_min if q_min < v else v      # the C min() macro (NaN propagates like it)
    lib().sgpu_normalize_quality(q.ctypes.data_as(C.c_void_p), len(q), q_min, q_max)
    return q, q_index


def register_shift_dft_full(frames, ref_index: int, selection, ctx=None, cfa=None):
    """register_shift_dft (registration/shift_methods.c:60-321) with its
    per-frame outputs: integer shifts (as register_shift_dft above), the
    normalised quality of every frame (QualityEstimate on the selection --
    after interpolate_nongreen for CFA frames, as the reference reads them --
    then normalizeQualityData) and the best frame index.
    Returns (shifts [N, 2] int32 tensor, quality [N] f64, best index)."""
    import torch
    from .stacking import default_context
    ctx = ctx or default_context()
    shifts = register_shift_dft(frames, ref_index, selection, ctx=ctx, cfa=cfa)
    x, y, w, h = selection
    win = frames[:, y:y + h, x:x + w]
    if cfa is not None:
        # a private copy (seq_read_frame_part reads one): contiguous() would
        # alias the caller's frames when the window is the whole block
        win = win.clone(memory_format=torch.contiguous_format)
        for i in range(win.shape[0]):
            interpolate_nongreen(win[i], cfa, ctx)
    q, best = normalize_quality(quality_estimate(win, ctx), ref_index)
    return shifts, q, best


# ---- applying the registration (apply_reg, interpolation "none") ----------
def apply_reg_shifts(Hs, ref_index: int):
    """Integer shifts of apply_reg with interpolation none: H = Href^-1 * Himg
    (cvTransfH) then shift_fit_from_reg's round_to_int(dx), round_to_int(dy)
    (registration.c:322-370).  Hs: per-frame 3x3 homographies (translations).
    Returns (shiftx, shifty) int32 arrays."""
    Hs = np.asarray(Hs, np.float64)
    n = Hs.shape[0]
    h02 = np.ascontiguousarray(Hs[:, 0, 2])
    h12 = np.ascontiguousarray(Hs[:, 1, 2])
    sx = np.zeros(n, np.int32)
    sy = np.zeros(n, np.int32)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().sgpu_apply_reg_shifts(n, dp(h02), dp(h12), ref_index, dp(sx), dp(sy)), "sgpu_apply_reg_shifts")
    return sx, sy


def shift_frames(frames, shiftx, shifty, out=None, ctx=None):
    """shift_fit_from_reg on every frame of a CUDA tensor [N, H, W] (float32,
    or 16-bit WORD samples): out[f, y + sy, x + sx] = frames[f, y, x], zero
    elsewhere (rows in FITS / Siril memory order).  Returns `out`."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W]")
    es = frames.element_size()
    n, h, w = frames.shape
    if out is None:
        out = torch.empty_like(frames)
    sx = np.ascontiguousarray(shiftx, np.int32)
    sy = np.ascontiguousarray(shifty, np.int32)
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    check(lib().sgpu_shift_frames_device(ctx.h, C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()), es, n, w, h,
                                         h * w, sx.ctypes.data_as(C.c_void_p), sy.ctypes.data_as(C.c_void_p)),
          "sgpu_shift_frames_device")
    return out


# interpolation enum (core/siril.h:333-340)
OPENCV_NEAREST, OPENCV_LINEAR, OPENCV_CUBIC, OPENCV_AREA, OPENCV_LANCZOS4, OPENCV_NONE = range(6)


def apply_reg(frames, Hs, ref_index: int, interpolation: int = OPENCV_LANCZOS4, out=None, ctx=None):
    """apply_reg (registration/applyreg.c:388-660) of translation
    registrations (REG_DFT's) at scale 1, FRAMING_CURRENT, with any
    interpolation: frames [N, H, W] CUDA tensor (float32 or 16-bit WORD
    storage), Hs [N, 3, 3] homographies.  Integer translations are exact
    shifts under every OpenCV kernel (sgpu_apply_reg_device); sub-pixel ones
    are refused except with OPENCV_NONE (rounded, shift_fit_from_reg)."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W]")
    n, h, w = frames.shape
    H = np.ascontiguousarray(np.asarray(Hs, np.float64).reshape(n, 9))
    out = torch.empty_like(frames) if out is None else out
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    check(lib().sgpu_apply_reg_device(ctx.h, C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()),
                                      frames.element_size(), n, w, h, h * w, H.ctypes.data_as(C.c_void_p), ref_index,
                                      int(interpolation)), "sgpu_apply_reg_device")
    return out


# ---- applying the registration with resampling (cvTransformImage) ----------
def warp_inverse_maps(Hs, ref_index: int, height: int) -> np.ndarray:
    """The destination -> source maps warp_frames uses ([N, 9] float64): the
    inverse of F * (Href^-1 * Hf) * F, F the row flip of a `height`-row frame
    (sgpu_warp_inverse_maps).  Singular or non-finite maps raise SgpuError."""
    H = np.ascontiguousarray(np.asarray(Hs, np.float64).reshape(-1, 9))
    M = np.zeros_like(H)
    check(lib().sgpu_warp_inverse_maps(H.shape[0], H.ctypes.data_as(C.c_void_p), int(ref_index), int(height),
                                       M.ctypes.data_as(C.c_void_p)), "sgpu_warp_inverse_maps")
    return M


def warp_table(interpolation: int) -> np.ndarray:
    """The [32, taps] float32 coefficient table of an interpolation
    (OPENCV_NEAREST..OPENCV_LANCZOS4), one row per 1/32-pixel phase."""
    tab = np.zeros(32 * 8, np.float32)
    taps = C.c_int(0)
    check(lib().sgpu_warp_table(int(interpolation), tab.ctypes.data_as(C.c_void_p), C.byref(taps)), "sgpu_warp_table")
    return tab[:32 * taps.value].reshape(32, taps.value).copy()


def warp_last_tiles(ctx) -> tuple:
    """(staged, direct): output tiles of ctx's last warp_frames call that read
    an LDS-staged source patch, and that gathered from global memory."""
    cnt = (C.c_long * 2)()
    check(lib().sgpu_warp_last_tiles(ctx.h, cnt), "sgpu_warp_last_tiles")
    return int(cnt[0]), int(cnt[1])


def warp_frames(frames, Hs, ref_index: int, interpolation: int = OPENCV_LANCZOS4, clamp: bool = True, out=None,
                ctx=None):
    """apply_reg with resampling (cvTransformImage at scale 1,
    FRAMING_CURRENT): frames [N, H, W] CUDA tensor (float32 or 16-bit WORD
    storage), Hs [N, 3, 3] homographies; frame f is warped through
    Href^-1 * Hf with OPENCV_NEAREST / LINEAR / CUBIC / AREA / LANCZOS4, zero
    outside the source frame; `clamp` applies Siril's undershoot clamp to
    CUBIC and LANCZOS4.  `out` must not alias `frames`.  The arithmetic is
    the specification in DESIGN.md "Frame warp" (OpenCV parity unpinned)."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W]")
    n, h, w = frames.shape
    H = np.ascontiguousarray(np.asarray(Hs, np.float64).reshape(n, 9))
    out = torch.empty_like(frames) if out is None else out
    if out.shape != frames.shape or out.dtype != frames.dtype or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA tensor like frames")
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    check(lib().sgpu_warp_frames_device(ctx.h, C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()),
                                        frames.element_size(), n, w, h, h * w, H.ctypes.data_as(C.c_void_p),
                                        int(ref_index), int(interpolation), int(bool(clamp))),
          "sgpu_warp_frames_device")
    return out


# ---- drizzle (seqapplyreg -drizzle) -----------------------------------------
DRIZZLE_KERNELS = {"point": 0, "turbo": 1, "square": 2}


def _drizzle_params(scale, pixfrac, kernel):
    from ._lib import DrizzleParams
    if isinstance(kernel, str):
        if kernel.lower() not in DRIZZLE_KERNELS:
            raise ValueError(f"drizzle kernel {kernel!r}: point, turbo or square")
        kernel = DRIZZLE_KERNELS[kernel.lower()]
    return DrizzleParams(float(scale), float(pixfrac), int(kernel), 0)


def drizzle_output_size(width: int, height: int, scale: float) -> tuple:
    """(out_w, out_h) = floor(size * scale + 0.5) per axis
    (sgpu_drizzle_output_size); a scale outside 0.1 .. 4 or an output
    dimension below 1 raises SgpuError."""
    ow, oh = C.c_int(0), C.c_int(0)
    check(lib().sgpu_drizzle_output_size(int(width), int(height), float(scale), C.byref(ow), C.byref(oh)),
          "sgpu_drizzle_output_size")
    return ow.value, oh.value


def drizzle_forward_maps(Hs, ref_index: int, height: int, width: Optional[int] = None, scale: float = 1.0,
                         pixfrac: float = 1.0, kernel="square") -> np.ndarray:
    """The input -> reference maps drizzle_frames uses ([N, 9] float64):
    F * ((Href^-1 * Hf) * F), F the row flip of a `height`-row frame
    (sgpu_drizzle_forward_maps).  Singular or non-finite maps raise SgpuError.
    With `width` the refusals that depend on the frame size are checked too
    (sgpu_drizzle_check_maps): a denominator that vanishes or changes sign
    over the input frame, or the inverse map's over the output frame."""
    H = np.ascontiguousarray(np.asarray(Hs, np.float64).reshape(-1, 9))
    A = np.zeros_like(H)
    check(lib().sgpu_drizzle_forward_maps(H.shape[0], H.ctypes.data_as(C.c_void_p), int(ref_index), int(height),
                                          A.ctypes.data_as(C.c_void_p)), "sgpu_drizzle_forward_maps")
    if width is not None:
        p = _drizzle_params(scale, pixfrac, kernel)
        check(lib().sgpu_drizzle_check_maps(A.shape[0], A.ctypes.data_as(C.c_void_p), int(width), int(height),
                                            C.byref(p)), "sgpu_drizzle_check_maps")
    return A


def drizzle_last_tiles(ctx) -> tuple:
    """(staged, direct): output tiles of ctx's last drizzle_frames call that
    read drops staged in LDS, and that mapped every candidate themselves."""
    cnt = (C.c_long * 2)()
    check(lib().sgpu_drizzle_last_tiles(ctx.h, cnt), "sgpu_drizzle_last_tiles")
    return int(cnt[0]), int(cnt[1])


def drizzle_frames(frames, Hs, ref_index: int, scale: float = 1.0, pixfrac: float = 1.0, kernel="square",
                   pixel_weights=None, out=None, out_weights=None, ctx=None, cfa=None):
    """Drizzle frames [N, H, W] (CUDA tensor, float32 or 16-bit WORD storage
    taken as (float)v) through Href^-1 * Hf onto the reference grid scaled by
    `scale` (0.1 .. 4), each input pixel shrunk to `pixfrac` (0 < pixfrac <= 1)
    of its side, with the "square", "turbo" or "point" kernel.  pixel_weights:
    [H, W] float32 CUDA tensor of weights >= 0 shared by the frames (0 skips
    the pixel), or None.  Returns (image, weights): float32 [N, out_h, out_w]
    each, fully overwritten; a pixel nothing landed on is 0 with weight 0, and
    `weights` is what Context.stack(drizzle=) takes.  The arithmetic is the
    specification in DESIGN.md "Drizzle" (Siril parity unpinned).
    cfa: the frames are colour-filter-array mosaics of this pattern (a 4- or
    36-letter string, or its compiled bytes, indexed in memory order like
    interpolate_nongreen's).  Every input pixel then lands in the plane of its
    own colour only, and image and weights are [N, 3, out_h, out_w] (R, G, B):
    channel c is, bit for bit, the drizzle with the pixel weights
    pixel_weights * [colour == c]; a colour the pattern lacks gives zeros."""
    import torch
    from .stacking import Context
    ctx = ctx or Context(frames.device.index or 0)
    if frames.dim() != 3 or not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous CUDA tensor [N, H, W]")
    if frames.element_size() not in (2, 4) or (frames.element_size() == 4 and frames.dtype != torch.float32):
        raise ValueError("frames must be float32 or 16-bit WORD storage")
    n, h, w = frames.shape
    H = np.ascontiguousarray(np.asarray(Hs, np.float64).reshape(n, 9))
    p = _drizzle_params(scale, pixfrac, kernel)
    ow, oh = drizzle_output_size(w, h, p.scale)
    pat, dim = _cfa_args(cfa)
    pwp = None
    if pixel_weights is not None:
        if (not pixel_weights.is_cuda or pixel_weights.dtype != torch.float32 or tuple(pixel_weights.shape) != (h, w)
                or not pixel_weights.is_contiguous() or pixel_weights.device != frames.device):
            raise ValueError("pixel_weights must be a contiguous float32 CUDA tensor [H, W] on the frames' device")
        pwp = C.c_void_p(pixel_weights.data_ptr())
    shape = (n, oh, ow) if pat is None else (n, 3, oh, ow)
    planes = []
    for t, name in ((out, "out"), (out_weights, "out_weights")):
        if t is None:
            t = torch.empty(shape, dtype=torch.float32, device=frames.device)
        if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or t.device != frames.device):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor {list(shape)}")
        planes.append(t)
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    if pat is not None:
        check(lib().sgpu_drizzle_cfa_frames_device(ctx.h, C.c_void_p(frames.data_ptr()), frames.element_size(), n, w, h,
                                                   h * w, pwp, pat.ctypes.data_as(C.c_void_p), dim,
                                                   H.ctypes.data_as(C.c_void_p), int(ref_index), C.byref(p),
                                                   C.c_void_p(planes[0].data_ptr()), C.c_void_p(planes[1].data_ptr()),
                                                   oh * ow, 3 * oh * ow), "sgpu_drizzle_cfa_frames_device")
        return planes[0], planes[1]
    check(lib().sgpu_drizzle_frames_device(ctx.h, C.c_void_p(frames.data_ptr()), frames.element_size(), n, w, h, h * w,
                                           pwp, H.ctypes.data_as(C.c_void_p), int(ref_index), C.byref(p),
                                           C.c_void_p(planes[0].data_ptr()), C.c_void_p(planes[1].data_ptr()),
                                           oh * ow), "sgpu_drizzle_frames_device")
    return planes[0], planes[1]


# ---- star detection and star-based global registration ---------------------
# sgpu_star (include/sirilgpu.h)
STAR_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("flux", "f8"), ("amp", "f8"), ("fwhm_major", "f8"),
                       ("fwhm_minor", "f8"), ("roundness", "f8"), ("px", "i4"), ("py", "i4"), ("npix", "i4"),
                       ("ext", "i4", 4), ("reject", "i4")])
MODELS = {"shift": 0, "similarity": 1, "affine": 2, "homography": 3}
STAR_PARAMS = ("ksigma", "radius", "smooth_sigma", "roundness_min", "min_amp", "cut", "min_fwhm", "sat", "max_stars")
MATCH_PARAMS = ("nbright", "tri_tol", "match_radius", "min_pairs", "model")


def star_params(**params):
    """sgpu_star_params with the defaults of DESIGN.md 6f, overridden by `params`."""
    from ._lib import StarParams
    p = StarParams()
    lib().sgpu_star_default_params(C.byref(p))
    for k, v in params.items():
        if k not in STAR_PARAMS + ("keep_candidates",):
            raise TypeError(f"find_stars: unknown parameter {k}")
        setattr(p, k, v)
    return p


def match_params(**params):
    """sgpu_match_params with its defaults, overridden by `params` (model by name or number)."""
    from ._lib import MatchParams
    p = MatchParams()
    lib().sgpu_match_default_params(C.byref(p))
    for k, v in params.items():
        if k not in MATCH_PARAMS:
            raise TypeError(f"match_stars: unknown parameter {k}")
        setattr(p, k, MODELS[v] if k == "model" and isinstance(v, str) else v)
    return p


def star_smooth_table(sigma: float) -> np.ndarray:
    """The normalised float32 smoothing table of find_stars, 2 * ceil(3 sigma) + 1 taps."""
    tab = np.zeros(13, np.float32)
    taps = C.c_int(0)
    check(lib().sgpu_star_smooth_table(float(sigma), tab.ctypes.data_as(C.c_void_p), C.byref(taps)),
          "sgpu_star_smooth_table")
    return tab[:taps.value].copy()


def frame_background(frames, ctx):
    """(bg, noise) per frame as find_stars defaults them: the median of the
    normalisation statistics and the background noise, in sample units."""
    from . import normalization as Nm
    fr = frames.contiguous()
    return Nm.norm_stats_device(ctx, fr, lite=True).median, Nm.bgnoise(ctx, fr)


def find_stars(frames, ctx=None, bg=None, noise=None, details=None, **params):
    """Stars of every frame of a CUDA tensor [N, H, W] (float32, or int16 /
    uint16 storage of WORD samples; the rows may be a window of larger
    frames): one STAR_DTYPE array per frame, brightest first, coordinates in
    memory order.  bg / noise: per-frame background and noise in sample units
    (default: frame_background).  params: ksigma, radius, smooth_sigma,
    roundness_min, min_amp, cut, min_fwhm, sat, max_stars (DESIGN.md 6f;
    modelled on Siril's star finder, parity unpinned).  `details`: a dict that
    receives ncandidates, kernel_ms (candidate pass, measurement) and
    candidates (every measured candidate per frame, raster order, with its
    reject code)."""
    import torch
    from .stacking import default_context
    ctx = ctx or default_context()
    if frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1 or \
            not (frames.dtype == torch.float32 or _is16(frames)):
        raise TypeError("frames must be a CUDA tensor [N, H, W], float32 or 16-bit, with unit column stride")
    n, h, w = frames.shape
    if bg is None or noise is None:
        b0, n0 = frame_background(frames, ctx)
        bg = b0 if bg is None else bg
        noise = n0 if noise is None else noise
    bg = np.ascontiguousarray(np.broadcast_to(np.asarray(bg, np.float64), (n,)))
    noise = np.ascontiguousarray(np.broadcast_to(np.asarray(noise, np.float64), (n,)))
    p = star_params(keep_candidates=int(details is not None), **params)
    ms = max(int(p.max_stars), 1)
    stars = np.zeros((n, ms), STAR_DTYPE)
    ns = np.zeros(n, np.int32)
    nc = np.zeros(n, np.int64)
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().sgpu_find_stars_device(ctx.h, C.c_void_p(frames.data_ptr()), frames.element_size(), n, w, h,
                                       frames.stride(1), frames.stride(0), vp(bg), vp(noise), C.byref(p), vp(stars),
                                       vp(ns), vp(nc)), "sgpu_find_stars_device")
    if details is not None:
        details["ncandidates"] = nc
        details["kernel_ms"] = star_last_kernel_ms(ctx)
        cands = []
        for f in range(n):
            cnt = C.c_long(0)
            check(lib().sgpu_star_last_candidates(ctx.h, f, None, 0, C.byref(cnt)), "sgpu_star_last_candidates")
            a = np.zeros(cnt.value, STAR_DTYPE)
            if cnt.value:
                check(lib().sgpu_star_last_candidates(ctx.h, f, vp(a), cnt.value, C.byref(cnt)),
                      "sgpu_star_last_candidates")
            cands.append(a)
        details["candidates"] = cands
    return [stars[f, :ns[f]].copy() for f in range(n)]


def star_last_kernel_ms(ctx) -> tuple:
    """(candidate pass, measurement): device milliseconds of ctx's last find_stars call."""
    kms = (C.c_float * 2)()
    check(lib().sgpu_star_last_kernel_ms(ctx.h, kms), "sgpu_star_last_kernel_ms")
    return float(kms[0]), float(kms[1])


# ---- PSF fit of found stars ------------------------------------
# sgpu_psf (include/sirilgpu.h)
PSF_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("bkg", "f8"), ("amp", "f8"), ("fwhm_major", "f8"),
                      ("fwhm_minor", "f8"), ("roundness", "f8"), ("angle", "f8"), ("beta", "f8"), ("rmse", "f8"),
                      ("a", "f8"), ("b", "f8"), ("c", "f8"), ("nused", "i4"), ("iterations", "i4"), ("status", "i4"),
                      ("reserved", "i4")])
PSF_PROFILES = {"gaussian": 0, "moffat": 1}
PSF_PARAMS = ("radius", "min_fwhm", "roundness_min", "sat", "max_iter")


def psf_params(profile="gaussian", beta=None, **params):
    """sgpu_psf_params with the defaults of DESIGN.md 6g, overridden by `params`
    (profile by name or number; beta None or <= 0: fitted)."""
    from ._lib import PsfParams
    p = PsfParams()
    lib().sgpu_psf_default_params(C.byref(p))
    if isinstance(profile, str):
        if profile not in PSF_PROFILES:
            raise ValueError(f"fit_stars: unknown profile {profile}")
        profile = PSF_PROFILES[profile]
    p.profile = int(profile)
    p.beta = 0.0 if beta is None else float(beta)
    for k, v in params.items():
        if k not in PSF_PARAMS:
            raise TypeError(f"fit_stars: unknown parameter {k}")
        setattr(p, k, v)
    return p


def fit_stars(frames, stars, ctx=None, bg=None, profile="gaussian", beta=None, **params):
    """Gaussian or Moffat PSF fit (modelled on Siril's PSF fit,
    parity unpinned) of the stars find_stars returned for the CUDA tensor
    `frames` [N, H, W]: one PSF_DTYPE array per frame, aligned with `stars`.
    `status` 0 marks a fitted, accepted star.  bg: per-frame background
    (default: frame_background).  profile "gaussian" or "moffat"; beta fixes
    the Moffat exponent (None: fitted).  params: radius, min_fwhm,
    roundness_min, sat, max_iter."""
    import torch
    from .stacking import default_context
    ctx = ctx or default_context()
    if frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1 or \
            not (frames.dtype == torch.float32 or _is16(frames)):
        raise TypeError("frames must be a CUDA tensor [N, H, W], float32 or 16-bit, with unit column stride")
    n, h, w = frames.shape
    if len(stars) != n:
        raise ValueError("fit_stars needs one star list per frame")
    if bg is None:
        bg = frame_background(frames, ctx)[0]
    bg = np.ascontiguousarray(np.broadcast_to(np.asarray(bg, np.float64), (n,)))
    p = psf_params(profile, beta, **params)
    ns = np.array([len(s) for s in stars], np.int32)
    ms = max(int(ns.max()), 1)
    flat = np.zeros((n, ms), STAR_DTYPE)
    for f in range(n):
        flat[f, :ns[f]] = stars[f]
    psf = np.zeros((n, ms), PSF_DTYPE)
    ctx.set_stream(torch.cuda.current_stream(frames.device).cuda_stream)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().sgpu_fit_stars_device(ctx.h, C.c_void_p(frames.data_ptr()), frames.element_size(), n, w, h,
                                      frames.stride(1), frames.stride(0), vp(bg), vp(flat), vp(ns), ms, C.byref(p),
                                      vp(psf)), "sgpu_fit_stars_device")
    return [psf[f, :ns[f]].copy() for f in range(n)]


def psf_last_kernel_ms(ctx) -> float:
    """Device milliseconds of the fit kernel of ctx's last fit_stars call."""
    ms = C.c_float(0)
    check(lib().sgpu_psf_last_kernel_ms(ctx.h, C.byref(ms)), "sgpu_psf_last_kernel_ms")
    return float(ms.value)


def _fitted_stars(stars, psf):
    """The stars whose fit has status 0, in the same (flux) order, with the
    fitted centre, widths and roundness in place of the moments' (PSF records
    of the same stars as the second list)."""
    out, kept = [], []
    for s, q in zip(stars, psf):
        m = q["status"] == 0
        s, q = s[m].copy(), q[m]
        for k in ("x", "y", "fwhm_major", "fwhm_minor", "roundness"):
            s[k] = q[k]
        out.append(s)
        kept.append(q)
    return out, kept


def _registration_values(stars, ref_index: int, npairs, reg, min_pairs: int):
    """(fwhm, wfwhm, roundness) of every frame from its star list: the mean of
    sqrt(fwhm_major * fwhm_minor), that value weighted by (nstars_ref -
    min_pairs) / (npairs - min_pairs) (0 when undefined), the mean roundness."""
    mean = lambda v: float(v.mean()) if len(v) else 0.0
    n = len(stars)
    fwhm = np.array([mean(np.sqrt(s["fwhm_major"] * s["fwhm_minor"])) for s in stars])
    nref = len(stars[ref_index])
    wfwhm = np.array([fwhm[f] * (nref - min_pairs) / (npairs[f] - min_pairs)
                      if reg[f] and npairs[f] > min_pairs and nref > min_pairs else 0.0 for f in range(n)])
    return fwhm, wfwhm, np.array([mean(s["roundness"]) for s in stars])


def _top_down_xy(stars, height: int) -> np.ndarray:
    """[n, 2] float64 top-down coordinates of a STAR_DTYPE array (memory-order
    y flipped), or of an [n, 2] array that already is top-down."""
    if isinstance(stars, np.ndarray) and stars.dtype.names:
        return np.ascontiguousarray(np.stack([stars["x"], (height - 1) - stars["y"]], 1), np.float64)
    return np.ascontiguousarray(np.asarray(stars, np.float64).reshape(-1, 2))


def match_stars(ref, img, width: int, height: int, **params):
    """Match the star list `img` of a frame to `ref` (find_stars arrays, or
    [n, 2] top-down coordinates; brightest first) and fit the transform
    (model "shift", "similarity", "affine" or "homography") that maps frame
    pixels to reference pixels in Siril's top-down convention, h22 = 1.
    Returns (H [3, 3], pairs [npairs, 2] of (img, ref) indices, registered);
    a frame that is not registered has H all zeros."""
    r, m = _top_down_xy(ref, height), _top_down_xy(img, height)
    p = match_params(**params)
    H = np.zeros(9, np.float64)
    pairs = np.zeros((max(1, min(len(r), len(m))), 2), np.int32)
    npairs = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = lib().sgpu_match_stars(vp(r), len(r), vp(m), len(m), int(width), int(height), C.byref(p), vp(H),
                                  C.byref(npairs), vp(pairs))
    if code not in (0, 1):
        check(code, "sgpu_match_stars")
    return H.reshape(3, 3), pairs[:npairs.value].copy(), code == 0


# Accepted steps the registration allows a fit.  A Moffat profile reaches a
# Gaussian only as beta grows without limit, so on Gaussian-like stars the
# fitted beta settles at its bound of 10, where every overshooting step is
# rejected first and the damping has to rise again: those fits converge, but
# need 54-93 steps on the frames of DESIGN.md 6g, more than fit_stars' default
# of 50, which would end them with status 1 and drop the star.
PSF_REGISTER_MAX_ITER = {"gaussian": 50, "moffat": 200}


def _psf_stage(frames, stars, ctx, bg, psf, sp):
    """The optional PSF stage of the registration: (stars, psf records) with
    the stars whose fit failed dropped and the fitted values in place; the
    finder's radius, min_fwhm, roundness_min and sat carry over to the fit."""
    if psf not in PSF_PROFILES:
        raise ValueError(f"register_stars: psf must be None, 'gaussian' or 'moffat', not {psf!r}")
    fp = {k: sp[k] for k in ("radius", "min_fwhm", "roundness_min", "sat") if k in sp}
    return _fitted_stars(stars, fit_stars(frames, stars, ctx=ctx, bg=bg, profile=psf,
                                          max_iter=PSF_REGISTER_MAX_ITER[psf], **fp))


def register_stars(frames, ref_index: int, ctx=None, model="homography", bg=None, noise=None, psf=None, **params):
    """Star-based global registration of a CUDA tensor [N, H, W] against frame
    ref_index.  Returns (Hs [N, 3, 3], info): Hs go straight into warp_frames
    (Hs[ref_index] is the identity; a frame that did not register has the
    null homography and must be left out).  info: per-frame nstars, npairs,
    registered, fwhm (mean of sqrt(fwhm_major * fwhm_minor) over the frame's
    stars), wfwhm (fwhm * (nstars_ref - min_pairs) / (npairs - min_pairs), 0
    when undefined; modelled on Siril's weighted FWHM, parity unpinned),
    roundness (mean), bkg, and the star lists.  psf "gaussian" or "moffat"
    (beta fitted, up to PSF_REGISTER_MAX_ITER accepted steps) fits every star
    (fit_stars): the stars whose fit did not end
    with status 0 are dropped, the matcher pairs the fitted centres, fwhm /
    wfwhm / roundness come from the fitted values, and info gains `psf`, the
    fit records of the kept stars."""
    from .stacking import default_context
    ctx = ctx or default_context()
    sp = {k: v for k, v in params.items() if k in STAR_PARAMS}
    mp = {k: v for k, v in params.items() if k in MATCH_PARAMS}
    unknown = set(params) - set(sp) - set(mp)
    if unknown:
        raise TypeError(f"register_stars: unknown parameters {sorted(unknown)}")
    n, h, w = frames.shape
    if bg is None or noise is None:
        b0, n0 = frame_background(frames, ctx)
        bg = b0 if bg is None else bg
        noise = n0 if noise is None else noise
    stars = find_stars(frames, ctx=ctx, bg=bg, noise=noise, **sp)
    fits = None
    if psf is not None:
        stars, fits = _psf_stage(frames, stars, ctx, bg, psf, sp)
    min_pairs = int(match_params(model=model, **mp).min_pairs)
    Hs = np.zeros((n, 3, 3), np.float64)
    npairs = np.zeros(n, np.int32)
    reg = np.zeros(n, bool)
    for f in range(n):
        if f == ref_index:
            Hs[f], npairs[f], reg[f] = np.eye(3), len(stars[f]), True
            continue
        Hs[f], pr, reg[f] = match_stars(stars[ref_index], stars[f], w, h, model=model, **mp)
        npairs[f] = len(pr)
    fwhm, wfwhm, roundness = _registration_values(stars, ref_index, npairs, reg, min_pairs)
    info = dict(nstars=np.array([len(s) for s in stars], np.int32), npairs=npairs, registered=reg, fwhm=fwhm,
                wfwhm=wfwhm, roundness=roundness,
                bkg=np.broadcast_to(np.asarray(bg, np.float64), (n,)).copy(), stars=stars)
    if fits is not None:
        info["psf"] = fits
    return Hs, info


# ---- the `register` command --------------------------------------------------
INTERPOLATIONS = {"nearest": OPENCV_NEAREST, "ne": OPENCV_NEAREST, "linear": OPENCV_LINEAR, "li": OPENCV_LINEAR,
                  "cubic": OPENCV_CUBIC, "cu": OPENCV_CUBIC, "area": OPENCV_AREA, "ar": OPENCV_AREA,
                  "lanczos4": OPENCV_LANCZOS4, "la": OPENCV_LANCZOS4}


def _parse_cfa_option(value: str) -> str:
    """The pattern of a -cfa= option: one of the four Bayer strings, or the 36
    letters (R, G, B) of an X-Trans pattern."""
    v = value.upper()
    if v not in BAYER_PATTERNS and not (len(v) == 36 and set(v) <= set("RGB")):
        raise ValueError(f"Unknown CFA pattern {value}: RGGB, BGGR, GBRG, GRBG or 36 letters of R, G, B")
    return v


class RegisterCommand:
    def __init__(self, seq: str):
        self.seq = seq
        self.layer = 0
        self.transf = "homography"
        self.minpairs = 10
        self.maxstars = 2000
        self.noout = False
        self.interp = OPENCV_LANCZOS4
        self.clamp = True
        self.prefix = "r_"
        self.psf = "moments"
        self.cfa = None


def parse_register_command(words) -> RegisterCommand:
    """`register <seq> [-layer=] [-transf=shift|similarity|affine|homography]
    [-minpairs=] [-maxstars=] [-noout] [-interp=ne|li|cu|ar|la] [-noclamp]
    [-prefix=r_] [-psf=moments|gaussian|moffat] [-cfa=PATTERN -noout]`.
    -cfa= (the frames are mosaics of that pattern) needs -noout: a warped
    mosaic is meaningless."""
    words = list(words)
    if words and words[0] == "register":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("register needs a sequence name")
    cmd = RegisterCommand(words[0])
    for o in words[1:]:
        if o.startswith("-layer="):
            cmd.layer = int(o[7:])
            if cmd.layer < 0:
                raise ValueError("-layer= must not be negative")
        elif o.startswith("-transf="):
            if o[8:] not in MODELS:
                raise ValueError(f"Unknown transformation type {o[8:]}, aborting.")
            cmd.transf = o[8:]
        elif o.startswith("-minpairs="):
            cmd.minpairs = int(o[10:])
            if cmd.minpairs < 1:
                raise ValueError("-minpairs= must be at least 1")
        elif o.startswith("-maxstars="):
            cmd.maxstars = int(o[10:])
            if not 1 <= cmd.maxstars <= 2000:
                raise ValueError("-maxstars= must be between 1 and 2000")
        elif o == "-noout":
            cmd.noout = True
        elif o.startswith("-interp="):
            if o[8:] not in INTERPOLATIONS:
                raise ValueError(f"Unknown interpolation {o[8:]}, aborting.")
            cmd.interp = INTERPOLATIONS[o[8:]]
        elif o == "-noclamp":
            cmd.clamp = False
        elif o.startswith("-prefix="):
            cmd.prefix = o[8:]
            if not cmd.prefix:
                raise ValueError("Missing prefix after -prefix=")
        elif o.startswith("-psf="):
            if o[5:] != "moments" and o[5:] not in PSF_PROFILES:
                raise ValueError(f"Unknown PSF profile {o[5:]}, aborting.")
            cmd.psf = o[5:]
        elif o.startswith("-cfa="):
            cmd.cfa = _parse_cfa_option(o[5:])
        else:
            raise ValueError(f"Unexpected argument to register `{o}', aborting.")
    if cmd.cfa is not None and not cmd.noout:
        raise ValueError("-cfa= needs -noout: CFA frames are not warped (seqapplyreg -drizzle -cfa= drizzles them)")
    return cmd


def _seq_reference(path: str) -> int:
    """reference_image of the S line (-1: none chosen)."""
    with open(path) as f:
        for line in f:
            if line.startswith("S "):
                rest = line[2:].strip()
                rest = rest[1:].split("'", 1)[1].split() if rest.startswith("'") else rest.split()[1:]
                return int(rest[4])
    raise ValueError(f"{path}: no S line")


def _frame_io(d, name, fixed, layer, dev):
    """(read, upload) of a regular FITS sequence: read(num) gives one frame's
    plane (layer `layer` of RGB frames; whole=True: the frame as the file
    holds it), upload(host) a device tensor (WORD frames as 16-bit storage)."""
    import os
    import torch
    from .sequence import frame_name, read_fits

    def read(num, whole=False):
        a = read_fits(os.path.join(d, frame_name(name, num, fixed)))
        if whole:
            return a
        if a.ndim == 3:
            if layer >= a.shape[0]:
                raise ValueError("-layer= is outside the frames' layers")
            a = a[layer]
        elif layer:
            raise ValueError("-layer= is outside the frames' layers")
        return np.ascontiguousarray(a)

    def upload(host):
        return torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)

    return read, upload


def _write_warped(d, name, fixed, nums, read, upload, good, ref_index, Hs, interp, clamp, prefix, batch, regdata,
                  layer, ctx):
    """The output stage of `register` and of `seqapplyreg` without -drizzle:
    the frames `good` warped onto the reference as 32-bit
    <prefix><name>NNNNN.fit, renumbered consecutively, and their .seq
    (identity H).  batch: frames of device memory to use.  Returns the .seq."""
    import os
    from .calibration import INV_USHRT_MAX
    from .sequence import frame_name, write_fits, write_seq
    per = max(1, batch // 2 - 1)                      # input and output frames, and the reference frame's slot
    for b0 in range(0, len(good), per):
        part = good[b0:b0 + per]
        idx = part if ref_index in part else part + [ref_index]
        t = upload(np.stack([read(nums[f]) for f in idx]))
        res = warp_frames(t, Hs[idx], idx.index(ref_index), interp, clamp, ctx=ctx).cpu().numpy()
        for j, f in enumerate(part):
            a = res[j]
            if a.dtype != np.float32:                 # WORD frames: [0, 1] units, as 32-bit FITS hold them
                a = a.view(np.uint16).astype(np.float32) * np.float32(INV_USHRT_MAX)
            write_fits(os.path.join(d, frame_name(prefix + name, nums[0] + b0 + j, fixed)), a)
    # the new sequence holds the registered frames only, renumbered from the first image number
    out_seq = os.path.join(d, prefix + name + ".seq")
    write_seq(out_seq, prefix + name, len(good), beg=nums[0], fixed=fixed, reference=good.index(ref_index),
              homographies=np.tile(np.eye(3), (len(good), 1, 1)), reg_layer=layer,
              **{k: v[good] for k, v in regdata.items()})
    return out_seq


def run_register(line, ctx=None, max_batch_bytes: int = 1 << 30):
    """Run one `register` command line (a string or its words) on a regular
    FITS sequence: finds the stars of every frame (layer -layer= of RGB
    frames), matches them against the reference frame's, rewrites <seq>.seq
    with the homographies and the registration values (frames that did not
    register are deselected) and, unless -noout, writes the warped frames as
    32-bit <prefix><name>NNNNN.fit (the registered frames, renumbered
    consecutively) with their .seq (identity H).  Stacking a
    -noout sequence whose H are more than translations needs that output:
    the .seq reader takes h02 / h12 only.  -psf=gaussian|moffat fits every
    star as register_stars(psf=) does.  With -cfa=PATTERN (one-layer mosaics;
    the pattern comes from the command line because this FITS reader keeps no
    BAYERPAT) the stars are looked for on a device copy of every frame passed
    through interpolate_nongreen, as Siril does on CFA data; the frames on
    disk are not touched.  Returns (path of the .seq written last, Hs,
    info)."""
    import os
    import torch
    from .calibration import _read_seq
    from .sequence import write_seq
    from .stacking import Context
    cmd = parse_register_command(line.split() if isinstance(line, str) else line)
    seq = cmd.seq if cmd.seq.endswith(".seq") else cmd.seq + ".seq"
    d = os.path.dirname(os.path.abspath(seq))
    name, fixed, nums = _read_seq(seq)
    if nums != list(range(nums[0], nums[0] + len(nums))):
        raise ValueError("register needs consecutively numbered images")
    n = len(nums)
    ref_index = _seq_reference(seq)
    ref_index = ref_index if 0 <= ref_index < n else 0
    ctx = ctx or Context(0)
    dev = torch.device("cuda", ctx.device)

    read, upload = _frame_io(d, name, fixed, cmd.layer, dev)

    if cmd.cfa is not None and read(nums[0], whole=True).ndim != 2:
        raise ValueError("-cfa= needs one-layer frames")
    first = read(nums[0])
    h, w = first.shape
    batch = max(1, int(max_batch_bytes // (h * w * 4)))
    stars, bkg, fits = [], [], []
    for b0 in range(0, n, batch):
        t = upload(np.stack([read(num) for num in nums[b0:b0 + batch]]))
        if cmd.cfa is not None:                       # the upload is the copy: the files stay as they are
            for k in range(t.shape[0]):
                interpolate_nongreen(t[k], cmd.cfa, ctx)
        bg, noise = frame_background(t, ctx)
        found = find_stars(t, ctx=ctx, bg=bg, noise=noise, max_stars=cmd.maxstars)
        if cmd.psf != "moments":
            found, q = _psf_stage(t, found, ctx, bg, cmd.psf, {})
            fits.extend(q)
        stars.extend(found)
        bkg.extend(bg)
    Hs = np.zeros((n, 3, 3))
    npairs = np.zeros(n, np.int32)
    reg = np.zeros(n, bool)
    for f in range(n):
        if f == ref_index:
            Hs[f], npairs[f], reg[f] = np.eye(3), len(stars[f]), True
            continue
        Hs[f], pr, reg[f] = match_stars(stars[ref_index], stars[f], w, h, model=cmd.transf, min_pairs=cmd.minpairs)
        npairs[f] = len(pr)
    fwhm, wfwhm, roundness = _registration_values(stars, ref_index, npairs, reg, cmd.minpairs)
    info = dict(nstars=np.array([len(s) for s in stars], np.int32), npairs=npairs, registered=reg,
                fwhm=fwhm, wfwhm=wfwhm, roundness=roundness, bkg=np.array(bkg, np.float64), stars=stars)
    if cmd.psf != "moments":
        info["psf"] = fits
    regdata = dict(fwhm=info["fwhm"], wfwhm=info["wfwhm"], roundness=info["roundness"], bkg=info["bkg"],
                   nstars=info["nstars"])
    write_seq(seq, name, n, beg=nums[0], fixed=fixed, reference=ref_index, included=reg, homographies=Hs,
              reg_layer=cmd.layer, **regdata)
    if cmd.noout:
        return seq, Hs, info
    good = [f for f in range(n) if reg[f]]
    out_seq = _write_warped(d, name, fixed, nums, read, upload, good, ref_index, Hs, cmd.interp, cmd.clamp, cmd.prefix,
                            batch, regdata, cmd.layer, ctx)
    return out_seq, Hs, info


# ---- seqapplyreg: apply an existing registration, by warp or by drizzle ------
class SeqApplyRegCommand:
    """Parsed `seqapplyreg` command."""

    def __init__(self, seq: str):
        self.seq = seq
        self.layer = 0
        self.drizzle = False
        self.scale = 1.0
        self.pixfrac = 1.0
        self.kernel = "square"
        self.flat = None
        self.cfa = None
        self.interp = OPENCV_LANCZOS4
        self.clamp = True
        self.prefix = "r_"


def parse_seqapplyreg_command(words) -> SeqApplyRegCommand:
    """`seqapplyreg <seq> [-layer=] [-prefix=r_] [-interp=ne|li|cu|ar|la]
    [-noclamp] | -drizzle [-scale=1] [-pixfrac=1] [-kernel=point|turbo|square]
    [-flat=FILE] [-cfa=RGGB|BGGR|GBRG|GRBG|<36 letters>]`.  The drizzle options
    need -drizzle, and -drizzle takes no interpolation."""
    words = list(words)
    if words and words[0] == "seqapplyreg":
        words = words[1:]
    if not words or words[0].startswith("-"):
        raise ValueError("seqapplyreg needs a sequence name")
    cmd = SeqApplyRegCommand(words[0])
    drizzle_only, warp_only = [], []
    for o in words[1:]:
        if o == "-drizzle":
            cmd.drizzle = True
        elif o.startswith("-layer="):
            cmd.layer = int(o[7:])
            if cmd.layer < 0:
                raise ValueError("-layer= must not be negative")
        elif o.startswith("-scale="):
            cmd.scale = float(o[7:])
            if not 0.1 <= cmd.scale <= 4.0:
                raise ValueError("-scale= must be between 0.1 and 4")
            drizzle_only.append(o)
        elif o.startswith("-pixfrac="):
            cmd.pixfrac = float(o[9:])
            if not 0.0 < cmd.pixfrac <= 1.0:
                raise ValueError("-pixfrac= must be above 0 and at most 1")
            drizzle_only.append(o)
        elif o.startswith("-kernel="):
            if o[8:] not in DRIZZLE_KERNELS:
                raise ValueError(f"Unknown drizzle kernel {o[8:]}, aborting.")
            cmd.kernel = o[8:]
            drizzle_only.append(o)
        elif o.startswith("-flat="):
            cmd.flat = o[6:]
            if not cmd.flat:
                raise ValueError("Missing file name after -flat=")
            drizzle_only.append(o)
        elif o.startswith("-cfa="):
            cmd.cfa = _parse_cfa_option(o[5:])
            drizzle_only.append(o)
        elif o.startswith("-interp="):
            if o[8:] not in INTERPOLATIONS:
                raise ValueError(f"Unknown interpolation {o[8:]}, aborting.")
            cmd.interp = INTERPOLATIONS[o[8:]]
            warp_only.append(o)
        elif o == "-noclamp":
            cmd.clamp = False
            warp_only.append(o)
        elif o.startswith("-prefix="):
            cmd.prefix = o[8:]
            if not cmd.prefix:
                raise ValueError("Missing prefix after -prefix=")
        else:
            raise ValueError(f"Unexpected argument to seqapplyreg `{o}', aborting.")
    if drizzle_only and not cmd.drizzle:
        raise ValueError(f"{drizzle_only[0]} needs -drizzle")
    if warp_only and cmd.drizzle:
        raise ValueError(f"{warp_only[0]} does not apply to -drizzle")
    return cmd


def read_seq_registration(path: str, layer: int = 0):
    """The registration a .seq holds for `layer`, as write_seq(homographies=)
    wrote it: (included [n] bool, Hs [n, 3, 3] with the null homography for a
    frame that is not registered, values) with values the per-frame fwhm,
    wfwhm, roundness, quality, bkg (float64) and nstars (int32).  ValueError
    when the file has no R<layer> lines with homographies or not one per
    image."""
    inc, rows = [], []
    tag = f"R{layer}"
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "I":
                inc.append(bool(int(t[2])))
            elif t[0] == tag:
                if len(t) != 17 or t[7] != "H":
                    raise ValueError(f"{path}: an {tag} line without a homography")
                rows.append([float(v) for v in t[1:7]] + [float(v) for v in t[8:17]])
    if not rows or len(rows) != len(inc):
        raise ValueError(f"{path}: no registration data for layer {layer}")
    r = np.array(rows, np.float64)
    values = dict(fwhm=r[:, 0], wfwhm=r[:, 1], roundness=r[:, 2], quality=r[:, 3], bkg=r[:, 4],
                  nstars=r[:, 5].astype(np.int32))
    return np.array(inc, bool), r[:, 6:].reshape(-1, 3, 3), values


def drizzle_flat_weights(flat: np.ndarray) -> np.ndarray:
    """The pixel-weight plane of a master flat: every sample as
    a double over the double mean of all samples, rounded to float32; a sample
    that is not above 0 or not finite weighs 0.  ValueError when the mean is
    not above 0."""
    f = np.asarray(flat).astype(np.float64)
    m = float(np.sum(f, dtype=np.float64)) / f.size
    if not (m > 0.0 and np.isfinite(m)):
        raise ValueError("the flat's mean must be above 0")
    w = (f / m).astype(np.float32)
    w[~(np.isfinite(w) & (f > 0.0))] = 0.0
    return w


def run_seqapplyreg(line, ctx=None, max_batch_bytes: int = 1 << 30):
    """Run one `seqapplyreg` command line (a string or its words) on a regular
    FITS sequence that `register -noout` registered: the included frames with
    a non-null homography are applied onto the reference frame.  Without
    -drizzle they are warped exactly as `register`'s output stage does.  With
    -drizzle they are drizzled (drizzle_frames) to 32-bit
    <prefix><name>NNNNN.fit of the scaled size (WORD input in [0, 1] units),
    their weight planes go to drizztmp/oweight_<prefix><name>NNNNN.fit beside
    them, and the new .seq (identity H, registration values carried over)
    has its drizzle_flag set.  -flat= weights the input pixels by a master
    flat over its mean.  With -cfa=PATTERN the frames are colour-filter-array
    mosaics (one layer, else ValueError): every input pixel lands in the plane
    of its own colour only (drizzle_frames(cfa=)), the frames and their weight
    files have three layers (R, G, B) and the .seq says nb_layers 3, so that
    `stack` weighs every layer by its own plane.  The pattern is given on the
    command line because this FITS reader keeps no BAYERPAT.  Returns (path
    of the new .seq, Hs, info)."""
    import os
    import torch
    from .calibration import INV_USHRT_MAX, _master_file, _read_seq
    from .sequence import frame_name, write_fits, write_seq
    from .stacking import Context
    cmd = parse_seqapplyreg_command(line.split() if isinstance(line, str) else line)
    seq = cmd.seq if cmd.seq.endswith(".seq") else cmd.seq + ".seq"
    d = os.path.dirname(os.path.abspath(seq))
    name, fixed, nums = _read_seq(seq)
    if nums != list(range(nums[0], nums[0] + len(nums))):
        raise ValueError("seqapplyreg needs consecutively numbered images")
    n = len(nums)
    inc, Hs, regdata = read_seq_registration(seq, cmd.layer)
    if len(inc) != n:
        raise ValueError(f"{seq}: registration data does not match the images")
    ref_index = _seq_reference(seq)
    ref_index = ref_index if 0 <= ref_index < n else 0
    good = [f for f in range(n) if inc[f] and Hs[f].any()]
    if ref_index not in good:
        raise ValueError("seqapplyreg: the reference image is not registered")
    ctx = ctx or Context(0)
    dev = torch.device("cuda", ctx.device)
    read, upload = _frame_io(d, name, fixed, cmd.layer, dev)
    if cmd.cfa is not None and read(nums[0], whole=True).ndim != 2:
        raise ValueError("-cfa= needs one-layer frames")
    h, w = read(nums[0]).shape
    info = dict(registered=np.array([f in good for f in range(n)]))
    if not cmd.drizzle:
        del regdata["quality"]                        # register carries no quality
        batch = max(1, int(max_batch_bytes // (h * w * 4)))
        out_seq = _write_warped(d, name, fixed, nums, read, upload, good, ref_index, Hs, cmd.interp, cmd.clamp,
                                cmd.prefix, batch, regdata, cmd.layer, ctx)
        return out_seq, Hs, info
    ow, oh = drizzle_output_size(w, h, cmd.scale)
    pw = None
    if cmd.flat is not None:
        flat = _master_file(cmd.flat, d)
        if flat.shape != (h, w):
            raise ValueError("-flat= does not have the frames' size")
        pw = torch.from_numpy(drizzle_flat_weights(flat)).to(dev)
    # device bytes per frame: the input plane and the two output planes (CFA: six) of scale^2 its pixels
    nout = 2 if cmd.cfa is None else 6
    per = max(1, int(max_batch_bytes // (h * w * 4 + nout * ow * oh * 4)) - 1)   # - 1: the reference frame's slot
    os.makedirs(os.path.join(d, "drizztmp"), exist_ok=True)
    tiles = [0, 0]
    for b0 in range(0, len(good), per):
        part = good[b0:b0 + per]
        idx = part if ref_index in part else part + [ref_index]
        t = upload(np.stack([read(nums[f]) for f in idx]))
        img, wts = drizzle_frames(t, Hs[idx], idx.index(ref_index), cmd.scale, cmd.pixfrac, cmd.kernel,
                                  pixel_weights=pw, ctx=ctx, cfa=cmd.cfa)
        st = drizzle_last_tiles(ctx)
        tiles = [tiles[0] + st[0], tiles[1] + st[1]]
        img, wts = img.cpu().numpy(), wts.cpu().numpy()
        for j, f in enumerate(part):
            a = img[j]
            if t.dtype != torch.float32:              # WORD frames: [0, 1] units, as 32-bit FITS hold them
                a = a * np.float32(INV_USHRT_MAX)
            fn = frame_name(cmd.prefix + name, nums[0] + b0 + j, fixed)
            write_fits(os.path.join(d, fn), a)
            write_fits(os.path.join(d, "drizztmp", "oweight_" + fn), wts[j])
    out_seq = os.path.join(d, cmd.prefix + name + ".seq")
    write_seq(out_seq, cmd.prefix + name, len(good), beg=nums[0], fixed=fixed, reference=good.index(ref_index),
              homographies=np.tile(np.eye(3), (len(good), 1, 1)), reg_layer=cmd.layer, drizzle=True,
              nb_layers=1 if cmd.cfa is None else 3,
              **{k: v[good] for k, v in regdata.items()})
    info.update(tiles=tuple(tiles), size=(ow, oh))
    return out_seq, Hs, info

"""The CFA drizzle of DESIGN.md 6h ("CFA frames") as its contract states it:
channel c is the mono drizzle (tests/drizzle_ref.py, unchanged) with the pixel
weights w * [colour == c], w the weight plane or 1.  Three passes of
drizzle_ref.drizzle_frame per frame and no arithmetic of its own.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_ref as DR  # noqa: E402

f32 = np.float32
XTRANS = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"


def pattern_bytes(pattern):
    """(entries, dim) of a 4- or 36-letter string or of a byte array."""
    if isinstance(pattern, str):
        pattern = ["RGB".index(ch) for ch in pattern.upper()]
    pat = np.asarray(pattern, np.uint8).ravel()
    dim = {4: 2, 36: 6}[pat.size]
    assert pat.max() <= 2
    return pat, dim


def colour_plane(pattern, width, height):
    """Colour of every memory-order pixel: pattern[(j % dim) * dim + i % dim]."""
    pat, dim = pattern_bytes(pattern)
    j, i = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return pat[(j % dim) * dim + (i % dim)]


def drizzle_frame_cfa(planes, A, scale, pixfrac, kernel, pattern, pw=None):
    """One frame.  planes: a list of 2-D arrays drizzled with one map.  Returns
    ([image [3, oh, ow] per plane], weights [3, oh, ow])."""
    h, w = planes[0].shape
    col = colour_plane(pattern, w, h)
    imgs, wts = [[] for _ in planes], []
    for c in range(3):
        mask = (col == c).astype(f32)
        outs, cnt = DR.drizzle_frame(list(planes), A, scale, pixfrac, kernel, mask if pw is None else pw * mask)
        for k, o in enumerate(outs):
            imgs[k].append(o)
        wts.append(cnt)
    return [np.stack(v) for v in imgs], np.stack(wts)


def drizzle_frames_cfa(frame_sets, Hs, ref_index, scale, pixfrac, kernel, pattern, pw=None):
    """frame_sets: a list of [N, H, W] arrays drizzled with the same maps.
    Returns ([images [N, 3, oh, ow] per set], weights [N, 3, oh, ow])."""
    n, h, w = frame_sets[0].shape
    A = DR.forward_maps(Hs, ref_index, h)
    for f in range(n):
        DR.check_map(A[f], w, h, scale, pixfrac, kernel)
    imgs, wts = [[] for _ in frame_sets], []
    for f in range(n):
        outs, cnt = drizzle_frame_cfa([fs[f] for fs in frame_sets], A[f], scale, pixfrac, kernel, pattern, pw)
        for k, o in enumerate(outs):
            imgs[k].append(o)
        wts.append(cnt)
    return [np.stack(v) for v in imgs], np.stack(wts)

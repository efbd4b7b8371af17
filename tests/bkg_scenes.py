"""Scenes and shared restatement results of the background-extraction tests
(tests/test_bkg.py pins the conditions, tests/test_bkg_gpu.py runs the GPU on
them): P = 3 planes per case, each with its own smooth gradient, noise, a few
bright "stars" and a patch raised by 0.2 over about 15 % of the plane (above
the selection threshold).  The restatement of a case is computed once and
shared; nobody writes to it."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402

# (width, height, samples, tolerance)
CASES = {"small_t1": (131, 77, 10, 1.0), "small_t3": (131, 77, 10, 3.0), "wide": (200, 150, 20, 1.0)}
NPLANES = 3


def plane(w, h, p, word, seed=0):
    rng = np.random.RandomState(1000 * seed + 10 * p + int(word))
    x, y = np.meshgrid(np.arange(w, dtype=np.float64) / w, np.arange(h, dtype=np.float64) / h)
    a = rng.uniform(0.5, 1.5, 4)        # each plane its own gradient
    v = 0.10 + 0.02 * p + 0.04 * (p + 1) * a[0] * x + 0.03 * (3 - p) * a[1] * y + 0.02 * a[2] * x * y + \
        0.015 * a[3] * (x - 0.5) ** 2
    v = v + rng.normal(0.0, 0.002, (h, w))
    # the raised patch: the right 30 % of the upper half
    v[: h // 2, int(0.7 * w):] += 0.2
    for _ in range(6):
        sx, sy = rng.randint(2, w - 2), rng.randint(2, h - 2)
        v[sy - 1:sy + 2, sx - 1:sx + 2] += 0.5
    if word:
        return np.round(v * 65535.0).astype(np.uint16)
    return v.astype(np.float32)


def frames(case, word):
    w, h, _, _ = CASES[case]
    return np.stack([plane(w, h, p, word) for p in range(NPLANES)])


@functools.lru_cache(maxsize=None)
def reference(case, word):
    """Per plane: the restatement's med, keep, kept, T and, per degree 1 .. 4,
    (status, coef, mean) and the same fit with the sums in descending order."""
    w, h, S, tol = CASES[case]
    g = BR.grid(w, h, S)
    fr = frames(case, word)
    out = []
    for p in range(NPLANES):
        med = BR.box_medians(fr[p], g)
        keep, kept, T, m, mad = BR.select(med, tol)
        fits = {d: BR.fit(med, keep, g, w, h, d) for d in (1, 2, 3, 4)}
        rev = {d: BR.fit(med, keep, g, w, h, d, descending=True) for d in (1, 2, 3, 4)}
        out.append(dict(med=med, keep=keep, kept=kept, T=T, fits=fits, rev=rev))
    return dict(grid=g, frames=fr, planes=out, w=w, h=h, S=S, tol=tol)

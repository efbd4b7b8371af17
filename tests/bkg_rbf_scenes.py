"""Cases and shared restatement results of the thin-plate-spline tests
(tests/test_bkg_rbf.py pins what the cases are, tests/test_bkg_rbf_gpu.py runs
the GPU on them).  The scenes are tests/bkg_scenes.py's; the edge planes and
the systems of the solve seam are made here.  The restatement of a case is
computed once and shared; nobody writes to it."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402
import bkg_rbf_ref as RR  # noqa: E402
import bkg_scenes as SC  # noqa: E402

# n of plane 0 of the float32 frames, and the condition of its system at smooth 0.5
SCENE_N = {"small_t1": 36, "small_t3": 39, "wide": 178}
CAP = (57, 55, 57, 1e9)          # K = n = 1023, order 1024
CAP_REFUSED = (57, 56, 57)       # K = 1056
ONE = (40, 30, 1, 1.0)           # K = n = 1


def edge_plane(w, h, word, seed=7):
    """A positive plane with a gradient and noise: every box median is above 0."""
    rng = np.random.RandomState(seed + int(word))
    x, y = np.meshgrid(np.arange(w, dtype=np.float64) / w, np.arange(h, dtype=np.float64) / h)
    v = 0.2 + 0.1 * x + 0.05 * y * y + 0.03 * np.sin(5.0 * x + 3.0 * y) + rng.normal(0.0, 0.002, (h, w))
    return np.round(v * 65535.0).astype(np.uint16) if word else v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def plane_reference(key, smooth=0.5, lam_rel=None):
    """The restatement of one plane.  key: ("scene", case, word, p), ("cap", word) or ("one", word)."""
    if key[0] == "scene":
        _, case, word, p = key
        w, h, S, tol = SC.CASES[case]
        plane = SC.frames(case, word)[p]
    elif key[0] == "cap":
        w, h, S, tol = CAP
        plane = edge_plane(w, h, key[1])
    else:
        w, h, S, tol = ONE
        plane = edge_plane(w, h, key[1])
    g = RR.check(w, h, S, tol, smooth)
    med = BR.box_medians(plane, g)
    keep, kept, T, m, mad = BR.select(med, tol)
    lr = RR.lam_rel(smooth) if lam_rel is None else lam_rel
    f = RR.fit(med, keep, g, w, h, lr)
    b = None if f["status"] else RR.background(f["x"], f["u"], f["v"], w, h)
    sub = RR.correct(plane, b, f["mean"], f["status"], False)
    div = RR.correct(plane, b, f["mean"], f["status"], True)
    return dict(plane=plane, w=w, h=h, S=S, tol=tol, grid=g, med=med, keep=keep, kept=kept, fit=f, bkg=b,
                weights=RR.weights_row(f), mean=f["mean"], status=f["status"], lam_rel=lr, sub=sub, div=div)


@functools.lru_cache(maxsize=None)
def grid_system(w, h, S, selection="all", smooth=0.5):
    """[A | rhs] of a grid of noiseless medians (the sky of scripts/subsky_bench.py, plane 0, with its
    raised patch): every box kept, or ("bench") the boxes tolerance 1.0 keeps."""
    g = RR.check(w, h, S, 1.0, smooth)
    cx, cy = BR.centres(g)
    med = np.zeros(g["K"], np.float32)
    for k in range(g["K"]):
        px, py = cx[k % g["nx"]], cy[k // g["nx"]]
        x, y = px / w, py / h
        med[k] = 0.1 + 0.04 * x + 0.03 * y + 0.02 * x * y + 0.015 * (x - 0.5) ** 2 + \
            (0.2 if (py < h // 2 and px >= int(0.7 * w)) else 0.0)
    keep = np.ones(g["K"], np.uint8) if selection == "all" else BR.select(med, 1.0)[0]
    u, v, z, _, _ = RR.samples(med, keep, g, w, h)
    return RR.system(u, v, z, RR.lam_rel(smooth))[0]


# ---- the systems of the solve seam: name -> float64 [nsys, N, N + 1] ----
TIE = np.array([[0.3, 0.7, 0.1, 0.1], [-0.9, 0.2, 0.5, 0.2], [0.9, 0.4, 0.6, 0.3]])


def _dense(n, seed, nsys=1):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((nsys, n, n + 1))


@functools.lru_cache(maxsize=None)
def seam_systems(name):
    if name == "order1":
        return np.array([[[2.0, 3.0]]])
    if name == "order2":
        return np.array([[[0.1, 0.2, 0.3], [0.3, 0.4, 0.5]]])
    if name == "tie":
        return TIE[None].copy()
    if name == "singular":
        return np.array([[[1.0, 2.0, 1.0], [2.0, 4.0, 2.0]]])
    if name == "nan":
        return np.array([[[1.0, np.nan, 1.0], [2.0, 3.0, 1.0]]])
    if name == "dense70":
        return _dense(70, 70)
    if name == "dense1025":
        return _dense(1025, 1025)
    if name == "eight":        # eight systems of order 33 in one call; system 5 has a repeated row
        a = _dense(33, 33, 8)
        a[5, 20] = a[5, 4]
        return a
    raise KeyError(name)


SEAM = ("order1", "order2", "tie", "singular", "nan", "dense70", "dense1025", "eight")
SEAM_STATUS = {"order1": [0], "order2": [0], "tie": [0], "singular": [2], "nan": [2], "dense70": [0], "dense1025": [0],
               "eight": [0, 0, 0, 0, 0, 2, 0, 0]}


@functools.lru_cache(maxsize=None)
def seam_reference(name):
    """(x float64 [nsys, N], status int32 [nsys]) of the restatement."""
    a = seam_systems(name)
    res = [RR.lu_solve(s) for s in a]
    return np.stack([r[1] for r in res]), np.array([r[0] for r in res], np.int32)

"""The background extraction's shared arithmetic (siril_amd/csrc/bkg_host.h:
grid and refusals, parameter checks, term table, ordered key, selection,
normal sums, Cholesky solve, closed-form mean, Horner evaluation, correction)
compiled without a device into a stand-alone program
(tests/hostsim/bkg_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program checks the grids, the
refusals and the statuses itself; this test compares what it prints for every
case with tests/bkg_ref.py: grid, medians, mask and count bit for bit, and the
coefficients, the mean, the background and the corrected samples bit for bit
too (host code without contraction must match the Python floats)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def scene(c, w, h, word):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    raised = np.where((x // 13 + 2 * (y // 13) + c) % 7 == 0, 13000, 0)
    v = 3000 + 7 * x * (c + 1) + 5 * y + ((x * 37 + y * 101 + 13 * c) % 97) * 3 + raised
    return v.astype(np.uint16) if word else v.astype(np.float32) * np.float32(1.0 / 65536.0)


def _dbl(t):
    return struct.unpack("<d", struct.pack("<Q", int(t, 16)))[0]


def _dbits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def test_bkg_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bkg_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "bkg_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "bkg host ok"
    lines = lines[:-1]
    assert len(lines) == 8 * 12
    cache = {}
    for k in range(0, len(lines), 8):
        head, gl, ml, kl, fl, cl, mean_l, bl = (ln.split() for ln in lines[k:k + 8])
        assert [t[0] for t in (head, gl, ml, kl, fl, cl, mean_l, bl)] == \
            ["case", "grid", "med", "keep", "fit", "coef", "mean", "bkg"]
        c, w, h, S, degree = (int(t) for t in head[1:6])
        tol, word = float(head[6]), int(head[7])
        if c not in cache:
            pl = scene(c, w, h, word)
            g = BR.grid(w, h, S)
            med = BR.box_medians(pl, g)
            cache[c] = (pl, g, med, BR.select(med, tol))
        pl, g, med, (keep, kept, T, m, mad) = cache[c]
        assert [int(t) for t in gl[1:]] == [g["nx"], g["ny"], g["dist"], g["startx"], g["starty"]]
        assert np.array_equal(np.array([int(t, 16) for t in ml[1:]], np.uint32), med.view(np.uint32)), ("med", c)
        assert np.array_equal(np.array([int(t) for t in kl[1:]], np.uint8), keep), ("keep", c)
        st, coef, mean = BR.fit(med, keep, g, w, h, degree)
        assert (int(fl[1]), int(fl[2])) == (kept, st) and st == 0 and kept >= BR.ncoef(degree)
        assert [int(t, 16) for t in cl[1:]] == [_dbits(v) for v in coef], ("coef", c, degree)
        assert int(mean_l[1], 16) == _dbits(mean), ("mean", c, degree)
        b = BR.background(coef, w, h)
        sub, div = BR.correct(pl, coef, mean), BR.correct(pl, coef, mean, divide=True)
        pts = [(0, 0), (w - 1, 0), (w // 2, h // 2), (3, h - 1), (w - 1, h - 1)]
        for j, (x, y) in enumerate(pts):
            assert int(bl[1 + 3 * j], 16) == _dbits(b[y, x]), ("bkg", c, degree, x, y)
            assert int(bl[2 + 3 * j], 16) == int(sub[y, x].view(np.uint32)), ("sub", c, degree, x, y)
            assert int(bl[3 + 3 * j], 16) == int(div[y, x].view(np.uint32)), ("div", c, degree, x, y)

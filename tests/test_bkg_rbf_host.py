"""The thin-plate-spline background's shared arithmetic
(siril_amd/csrc/bkg_rbf_host.h: refusals, coordinates, the logarithm built
from + - * /, the radial kernel, the system and its smoothing, the LU with its
tie rule, the mean, the background; bkg_host.h's medians, selection and
correction) compiled without a device into a stand-alone program
(tests/hostsim/bkg_rbf_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program checks the refusals and
the statuses itself; this test compares what it prints with
tests/bkg_rbf_ref.py bit for bit: the logarithms, the solutions of the
hand-made systems, and per case a row of Phi, the mean of |Phi|, lambda, the
weights, the mean, the background and the corrected samples (host code without
contraction must match numpy's float64)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402
import bkg_rbf_ref as RR  # noqa: E402
import bkg_rbf_scenes as RS  # noqa: E402

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


def _bits(a):
    return [int(v) for v in np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)]


def _hex(tokens):
    return [int(t, 16) for t in tokens]


def test_bkg_rbf_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bkg_rbf_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "bkg_rbf_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert lines[-1] == ["bkg", "rbf", "host", "ok"]
    # the logarithms
    assert lines[0][0] == "log"
    k = np.arange(256, dtype=np.float64)
    s = np.concatenate([(k + 1.0) * (k + 1.0) * 1.220703125e-4,
                        [1.0, 1.4142135623730951, 1.4142135623730954, 0.5, 2.0, 8.0, 1e-8, 0.70710678118654757]])
    assert _hex(lines[0][1:]) == _bits(RR.rbf_log(s))
    # the hand-made systems
    for ln, name in zip(lines[1:6], ("order1", "order2", "tie", "singular", "nan")):
        assert ln[:2] == ["solve", name]
        x, st = RS.seam_reference(name)
        assert int(ln[2]) == int(st[0]) == RS.SEAM_STATUS[name][0], name
        assert _hex(ln[3:]) == _bits(x[0]), name
    # the cases
    rest = lines[6:-1]
    assert len(rest) == 5 * 3
    for c in range(3):
        head, fl, pl_, xl, bl = rest[5 * c:5 * c + 5]
        assert [t[0] for t in (head, fl, pl_, xl, bl)] == ["case", "fit", "phi", "x", "bkg"]
        assert int(head[1]) == c
        w, h, S = (int(t) for t in head[2:5])
        tol, word, lam_rel = float(head[5]), int(head[6]), _dbl(head[7])
        smooth = (0.5, 0.0, 1.0)[c]
        assert abs(lam_rel / RR.lam_rel(smooth) - 1.0) < 1e-14     # libm's pow; the restatement takes the program's double
        plane = scene(c, w, h, word)
        out_sub, info = RR.subsky_rbf_plane(plane, S, tol, smooth, False, lam_rel_value=lam_rel)
        f = info["fit"]
        out_div = RR.correct(plane, info["bkg"], f["mean"], 0, True)
        assert (int(fl[1]), int(fl[2])) == (f["n"], 0) and f["status"] == 0 and f["n"] >= 20
        assert _hex(fl[3:]) == _bits([f["mean_abs"], f["lam"], f["mean"]]), ("fit", c)
        assert _hex(pl_[1:]) == _bits(f["aug"][0, :f["n"]] - np.where(np.arange(f["n"]) == 0, f["lam"], 0.0)), ("phi", c)
        assert _hex(xl[1:]) == _bits(f["x"]), ("x", c)
        pts = [(0, 0), (w - 1, 0), (w // 2, h // 2), (3, h - 1), (w - 1, h - 1), (int(f["px"][0]), int(f["py"][0]))]
        b = info["bkg"]
        for j, (x, y) in enumerate(pts):
            assert int(bl[1 + 3 * j], 16) == _bits(b[y, x])[0], ("bkg", c, x, y)
            assert int(bl[2 + 3 * j], 16) == int(out_sub[y, x].view(np.uint32)), ("sub", c, x, y)
            assert int(bl[3 + 3 * j], 16) == int(out_div[y, x].view(np.uint32)), ("div", c, x, y)

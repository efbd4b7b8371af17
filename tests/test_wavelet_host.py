"""The wavelets' shared arithmetic (siril_amd/csrc/wavelet_host.h: refusals,
conversion, reflection, the separable smoothing, details, the weighted
reconstruction) compiled without a device into a stand-alone program
(tests/hostsim/wavelet_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program checks the refusals,
the reflection and a constant plane itself; this test compares every sample it
prints, planes and reconstruction, with tests/wavelet_ref.py bit for bit (host
code without contraction must match the numpy floats)."""
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavelet_ref as WR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF = (3.0, 2.0, 1.5, 1.0, -0.5, 1.25)


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def scene(c, w, h, word):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    v = (x * 37 + y * 101 + 13 * c + (x * y) % 29 * 31) % 997
    return (v * 61).astype(np.uint16) if word else v.astype(np.float32) * np.float32(1.0 / 1024.0)


def test_wavelet_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wavelet_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "wavelet_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "wavelet host ok"
    lines = lines[:-1]
    assert len(lines) == 3 * 5
    for k in range(0, len(lines), 3):
        head, pl, rl = (ln.split() for ln in lines[k:k + 3])
        assert (head[0], pl[0], rl[0]) == ("case", "planes", "recon")
        c, w, h, n, type_, word = (int(t) for t in head[1:])
        x = scene(c, w, h, word)
        want = WR.transform(x, n, type_)
        got = np.array([int(t, 16) for t in pl[1:]], np.uint32).reshape(n, h, w)
        assert np.array_equal(got, want.view(np.uint32)), ("planes", c)
        rec = WR.reconstruct(want, COEF[:n])
        got = np.array([int(t, 16) for t in rl[1:]], np.uint32).reshape(h, w)
        assert np.array_equal(got, rec.view(np.uint32)), ("recon", c)

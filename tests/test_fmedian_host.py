"""The median filter's shared code (siril_amd/csrc/median_host.h: refusals,
conversion, the reference median of a window, modulation, the selection
networks) compiled without a device into a stand-alone program
(tests/hostsim/fmedian_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program checks the refusals,
the order and the modulation itself, proves the 9- and 25-input networks by
the 0-1 principle on all 2^9 and 2^25 zero-one inputs, and runs the 49-input
network on 10^6 random zero-one inputs of every weight and 10^5 random key
vectors against nth_element; this test compares every sample it prints with
tests/median_ref.py bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_ref as MR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def scene(c, w, h, word):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    v = (x * 37 + y * 101 + 13 * c + (x * y) % 29 * 31) % 997
    return (v * 61).astype(np.uint16) if word else v.astype(np.float32) * np.float32(1.0 / 1024.0)


def test_fmedian_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fmedian_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "fmedian_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "fmedian host ok"
    lines = lines[:-1]
    assert len(lines) == 2 * 6
    seen = set()
    for k in range(0, len(lines), 2):
        head, out = (ln.split() for ln in lines[k:k + 2])
        assert (head[0], out[0]) == ("case", "out")
        c, w, h, ksize = (int(t) for t in head[1:5])
        mod = np.array([int(head[5], 16)], np.uint32).view(np.float32)[0]
        it, word = int(head[6]), int(head[7])
        want = MR.fmedian(scene(c, w, h, word), ksize, mod, it)
        got = np.array([int(t, 16) for t in out[1:]], np.uint32).reshape(h, w)
        assert np.array_equal(got, want.view(np.uint32)), c
        seen.add((ksize, float(mod) == 1.0, it, word, (w, h) == (8, 8)))
    # what the cases have to cover
    assert {s[0] for s in seen} == {3, 7, 15} and {s[1] for s in seen} == {True, False}
    assert {s[2] for s in seen} == {1, 2} and {s[3] for s in seen} == {0, 1}
    assert any(s[0] == 15 and s[4] for s in seen)

"""The guided filter's shared code (siril_amd/csrc/epf_host.h: refusals, the
window rule, the coefficients, the host reference) compiled without a device into a stand-alone
program (tests/hostsim/epf_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program checks the refusals and
the small pieces itself; this test compares every sample it prints with
tests/epf_ref.py bit for bit.  Nothing loaded into Python runs under a
sanitizer."""
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epf_ref as ER  # noqa: E402

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


def test_epf_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "epf_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "epf_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "epf host ok"
    lines = lines[:-1]
    assert len(lines) == 2 * 7
    seen = set()
    for k in range(0, len(lines), 2):
        head, out = (ln.split() for ln in lines[k:k + 2])
        assert (head[0], out[0]) == ("case", "out")
        c, w, h, d = (int(t) for t in head[1:5])
        si, ss = (np.array([int(t, 16)], np.uint64).view(np.float64)[0] for t in head[5:7])
        mod = np.array([int(head[7], 16)], np.uint32).view(np.float32)[0]
        word, guide = int(head[8]), int(head[9])
        g = scene(c + 7, w, h, guide) if guide >= 0 else None
        want = ER.epf(scene(c, w, h, word), d, float(si), float(ss), mod, guide=g)
        got = np.array([int(t, 16) for t in out[1:]], np.uint32).reshape(h, w)
        assert np.array_equal(got, want.view(np.uint32)), c
        seen.add((ER.window(d, ss), float(mod) == 1.0, word, guide, (w, h) == (13, 13)))
    # what the cases have to cover
    assert {s[0] for s in seen} >= {3, 9, 25} and {s[1] for s in seen} == {True, False}
    assert {s[2] for s in seen} == {0, 1} and {s[3] for s in seen} == {-1, 0, 1}
    assert any(s[0] == 25 and s[4] for s in seen) and any(not s[4] for s in seen)

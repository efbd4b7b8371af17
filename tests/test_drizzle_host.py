"""The drizzle's shared arithmetic (siril_amd/csrc/drizzle_host.h: map, sgarea,
boxer, the three drops, the update, candidate windows, argument checks and
refusals) compiled without a device into a stand-alone program
(tests/hostsim/drizzle_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program compares its sequential
scatter with its gather bit for bit; this test compares the image and weight
plane it prints for every case with tests/drizzle_ref.py, bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_ref as DR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def _sample_planes(c, w, h, word):
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    v = ((i * 37 + j * 101 + 13 * c) % 1000) * 60 + 5
    fr = v.astype(np.uint16) if word else (v.astype(np.float32) + np.float32(0.25))
    pw = np.where((i + 2 * j) % 5 == 0, 0.0, 0.25 * ((i * 3 + j) % 8 + 1)).astype(np.float32)
    return fr, pw


def _plane(words, oh, ow):
    return np.array([int(t, 16) for t in words], np.uint32).reshape(oh, ow)


def test_drizzle_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "drizzle_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "drizzle_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "drizzle host ok"
    lines = lines[:-1]
    assert len(lines) % 5 == 0 and len(lines) >= 5 * 12
    kernels = set()
    for k in range(0, len(lines), 5):
        head, hl, size, img, wts = (ln.split() for ln in lines[k:k + 5])
        assert head[0] == "case" and hl[0] == "H" and size[0] == "size" and img[0] == "img" and wts[0] == "wts"
        c, w, h = int(head[1]), int(head[2]), int(head[3])
        scale, pixfrac = float(head[4]), float(head[5])
        kernel, word, use_pw = int(head[6]), int(head[7]), int(head[8])
        kernels.add(kernel)
        H = np.array([float(t) for t in hl[1:]]).reshape(3, 3)
        ow, oh = int(size[1]), int(size[2])
        assert (ow, oh) == DR.output_size(w, h, scale)
        fr, pw = _sample_planes(c, w, h, word)
        A = DR.forward_maps(np.stack([np.eye(3), H]), 0, h)[1]
        DR.check_map(A, w, h, scale, pixfrac, kernel)
        ref, cnt = DR.drizzle_frame(fr, A, scale, pixfrac, kernel, pw if use_pw else None)
        assert np.array_equal(_plane(img[1:], oh, ow), ref.view(np.uint32)), ("image", c)
        assert np.array_equal(_plane(wts[1:], oh, ow), cnt.view(np.uint32)), ("weights", c)
    assert kernels == {DR.POINT, DR.TURBO, DR.SQUARE}

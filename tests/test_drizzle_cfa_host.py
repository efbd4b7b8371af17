"""The CFA drizzle's shared arithmetic (siril_amd/csrc/drizzle_host.h: the
colour lookup, the pattern check, the CFA gather of one output pixel and the
CFA sequential scatter) compiled without a device into a stand-alone program
(tests/hostsim/drizzle_cfa_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once.  The program compares its CFA scatter
with its CFA gather and with the three masked mono scatters bit for bit; this
test compares the three image and weight planes it prints for every case with
tests/drizzle_cfa_ref.py, bit for bit."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_cfa_ref as CR  # noqa: E402
import drizzle_ref as DR  # noqa: E402
from test_drizzle_host import _compiler, _sample_planes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planes(words, oh, ow):
    return np.array([int(t, 16) for t in words], np.uint32).reshape(3, oh, ow)


def test_drizzle_cfa_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "drizzle_cfa_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "drizzle_cfa_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "drizzle cfa host ok"
    lines = lines[:-1]
    assert len(lines) % 5 == 0 and len(lines) >= 5 * 11
    kernels, patterns, absent = set(), set(), 0
    for k in range(0, len(lines), 5):
        head, hl, size, img, wts = (ln.split() for ln in lines[k:k + 5])
        assert head[0] == "case" and hl[0] == "H" and size[0] == "size" and img[0] == "img" and wts[0] == "wts"
        c, w, h = int(head[1]), int(head[2]), int(head[3])
        scale, pixfrac = float(head[4]), float(head[5])
        kernel, word, use_pw, pattern = int(head[6]), int(head[7]), int(head[8]), head[9]
        kernels.add(kernel)
        patterns.add(pattern)
        H = np.array([float(t) for t in hl[1:]]).reshape(3, 3)
        ow, oh = int(size[1]), int(size[2])
        assert (ow, oh) == DR.output_size(w, h, scale)
        fr, pw = _sample_planes(c, w, h, word)
        A = DR.forward_maps(np.stack([np.eye(3), H]), 0, h)[1]
        DR.check_map(A, w, h, scale, pixfrac, kernel)
        (ref,), cnt = CR.drizzle_frame_cfa([fr], A, scale, pixfrac, kernel, pattern, pw if use_pw else None)
        assert np.array_equal(_planes(img[1:], oh, ow), ref.view(np.uint32)), ("image", c)
        assert np.array_equal(_planes(wts[1:], oh, ow), cnt.view(np.uint32)), ("weights", c)
        for col in range(3):
            if "RGB"[col] not in pattern:
                absent += 1
                assert not ref[col].any() and not cnt[col].any()
            else:
                assert cnt[col].any()
    assert kernels == {DR.POINT, DR.TURBO, DR.SQUARE}
    assert {"RGGB", "BGGR", "GBRG", "GRBG", CR.XTRANS} <= patterns and absent == 1

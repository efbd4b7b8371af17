"""The stretches' shared code (siril_amd/csrc/stretch_host.h: refusals,
conversion, exp / pow / asinh on 6k's logarithm, the midtones transfer function,
the autostretch parameters, the generalised hyperbolic stretch with its
coefficient block and inverse, the colour models) compiled without a device
into a stand-alone program (tests/hostsim/stretch_host_main.cpp) with
AddressSanitizer and UndefinedBehaviorSanitizer, and run once.  The program
checks the refusals and a few identities itself; this test compares every
coefficient block, every sample and every autostretch parameter it prints with
tests/stretch_ref.py bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def scene(nplanes, w, h, word):
    """The scene of stretch_host_main.cpp: [nplanes, h, w]."""
    p, y, x = np.meshgrid(np.arange(nplanes), np.arange(h), np.arange(w), indexing="ij")
    v = (x * 37 + y * 101 + 13 * p + (x * y) % 29 * 31) % 997
    if word:
        s = (v * 65).astype(np.uint16)
        one = 65535
    else:
        s = v.astype(np.float32) * np.float32(1.0 / 900.0) - np.float32(0.05)
        one = 1.0
    f = s.reshape(nplanes, -1)
    f[:, 0] = 0
    if w * h > 1:
        f[:, 1] = one
    if w * h > 5:
        f[:, 5] = 0
    if not word and nplanes > 1 and w * h > 3:
        f[1, 3] = np.nan
    return f.reshape(nplanes, h, w)


def _doubles(words):
    return np.array([int(t, 16) for t in words], np.uint64).view(np.float64)


def test_stretch_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stretch_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "stretch_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "stretch host ok"
    lines = [ln.split() for ln in lines[:-1]]
    seen, autos, k = set(), set(), 0
    while k < len(lines):
        if lines[k][0] == "auto":
            head, res = lines[k:k + 2]
            k += 2
            assert res[0] == "params"
            nimages, nch, linked = (int(t) for t in head[1:4])
            unit, clip, target = _doubles(head[4:7])
            stats = _doubles(head[7:]).reshape(-1, 4)
            want = R.autostretch_params(stats[:, 0] / unit, stats[:, 1] / unit, nimages, nch, bool(linked), clip, target)
            assert np.array_equal(_doubles(res[1:]).view(np.uint64), want.ravel().view(np.uint64)), head
            autos.add((linked, bool((stats[:, 0] / unit > 0.5).any()), unit))
            continue
        head, coef, out = lines[k:k + 3]
        k += 3
        assert (head[0], coef[0], out[0]) == ("case", "coef", "out")
        fn, model, clipmode, mask, nimages, nch, w, h, word = (int(t) for t in head[1:10])
        d = _doubles(head[10:])
        p = R.Params(fn, model, clipmode, mask, *[float(v) for v in d])
        c, regime = R.coeffs(p)
        assert int(coef[1]) == regime, head
        assert np.array_equal(_doubles(coef[2:]).view(np.uint64), c.view(np.uint64)), head
        x = scene(nimages * nch, w, h, word)
        x = x.reshape((nimages, nch, h, w) if nch > 1 else (nimages, h, w))
        want = R.stretch(p, x)
        got = np.array([int(t, 16) for t in out[1:]], np.uint32).view(np.float32).reshape(want.shape)
        assert R.float32_bits_equal(got, want), head
        if not word and nimages * nch > 1:
            assert np.isnan(want).any()
        if R.joint(p, nch) and not word:
            i = np.argwhere(np.isnan(want))
            # the NaN is in channel 1: every stretched channel of its pixel is NaN, and channel 1 whatever the mask
            sel = sorted({ch for ch in range(3) if mask >> ch & 1} | {1})
            assert {tuple(t) for t in i[:, [0, 2, 3]]} == {(0, 3 // w, 3 % w)} and sorted(set(i[:, 1])) == sel
        seen.add((fn, regime if fn >= R.GHT else -1, model if nch == 3 else -1,
                  clipmode if R.joint(p, nch) and fn != R.ASINH else -1, word, nch, mask))
    # what the cases have to cover
    for fn in (R.GHT, R.INVGHT):
        assert {s[1] for s in seen if s[0] == fn} >= {R.Q_LOG, R.Q_NEG, R.Q_EXP, R.Q_POS}
    assert any(s[0] == R.GHT and s[1] == R.Q_IDENTITY for s in seen)
    assert {s[0] for s in seen} == set(range(7))
    for fn in (R.GHT, R.MODASINH):
        assert {(s[2], s[3]) for s in seen if s[0] == fn and s[3] >= 0} == \
            {(m, c) for m in (R.HUMAN, R.EVEN) for c in (R.CLIP, R.RESCALE, R.RGBBLEND)}
    assert {(s[4], s[5]) for s in seen if s[0] == R.ASINH} == {(0, 1), (1, 1), (0, 3), (1, 3)}
    assert {s[4] for s in seen} == {0, 1} and {s[6] for s in seen} >= {7, 5, 2, 6}
    assert {a[0] for a in autos} == {0, 1} and any(a[1] for a in autos) and {a[2] for a in autos} == {1.0, 65535.0}

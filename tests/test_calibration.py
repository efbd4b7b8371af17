"""Calibration, CPU side: the numpy restatement of the specification
(tests/calib_ref.py) against hand-computed cases, the `calibrate` command
line, and the dark-optimisation search on synthetic frames.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as CR  # noqa: E402

f32 = np.float32


def test_s1_conversion():
    a = np.array([[0, 1, 65535]], np.uint16)
    inv = f32(1.0) / f32(65535.0)
    assert np.array_equal(CR.to_float(a), np.array([[0, inv, f32(65535) * inv]], f32))


def test_s2_hand_computed_4x4():
    """Every value is a small dyadic number, so each step is exact:
    (x - bias - k*dark) / flat * norm, zero where the flat is zero."""
    frame = np.full((4, 4), 0.5, f32)
    frame[1, 2] = 0.125                       # goes negative
    bias = np.full((4, 4), 0.125, f32)
    dark = np.full((4, 4), 0.125, f32)
    flat = np.full((4, 4), 0.5, f32)
    flat[1, 2] = 2.0
    flat[3, 0] = 0.0                          # no data
    out = CR.s2(frame, bias=bias, dark=dark, k=2.0, flat=flat, norm=0.5)
    want = np.full((4, 4), 0.125, f32)        # (0.5 - 0.125 - 0.25) / 0.5 * 0.5
    want[1, 2] = -0.0625                      # (0.125 - 0.125 - 0.25) / 2 * 0.5
    want[3, 0] = 0.0
    assert out.dtype == np.float32 and np.array_equal(out, want)
    # a level in place of the plane, no dark, no flat
    assert np.array_equal(CR.s2(frame, level=0.25), frame - f32(0.25))
    # WORD input goes through S1 first
    w = np.full((4, 4), 65535, np.uint16)
    assert np.array_equal(CR.s2(w, level=0.5), np.full((4, 4), 0.5, f32))
    # no clamp: values above 1 and NaN pass through
    big = np.array([[3.0, np.nan]], f32)
    r = CR.s2(big, flat=np.array([[0.5, 1.0]], f32), norm=1.0)
    assert r[0, 0] == 6.0 and np.isnan(r[0, 1])


def test_s4_counts_only_nonzero_finite():
    p = np.array([[1, 0, 3], [np.nan, 5, 0]], f32)
    n, mean, sigma = CR.region_stats(p)
    assert n == 3 and mean == 3.0
    assert sigma == np.sqrt(35.0 / 3 - 9.0)
    assert CR.region_stats(np.zeros((2, 2), f32)) == (0, 0.0, 0.0)
    assert CR.region_stats(np.array([[2.0]], f32)) == (1, 2.0, 0.0)


@pytest.mark.parametrize("diag", [0, 1])
def test_s5_sites_and_green_choice_8x6(diag):
    """8 x 6: the evaluation region is x in [2, 4), y in [2, 4): one sample
    per site.  Site s = (y & 1) * 2 + (x & 1)."""
    m = [0.5, 0.25, 1.0, 0.5] if diag == 0 else [0.25, 0.5, 0.5, 1.0]
    flat = np.zeros((6, 8), f32)
    for s in range(4):
        flat[s >> 1::2, s & 1::2] = m[s]
    # samples outside the region must not matter
    flat[0, :] *= 3
    flat[:, 6:] *= 5
    out, d, c1, c2 = CR.equalize_cfa(flat)
    assert d == diag
    assert (c1, c2) == (2.0, 0.5)
    want = flat.copy()
    if diag == 0:       # sites 0 and 3 green: c1 = m0/m1 on site 1, c2 = m0/m2 on site 2
        want[0::2, 1::2] *= f32(2.0)
        want[1::2, 0::2] *= f32(0.5)
    else:               # sites 1 and 2 green: c1 = m1/m0 on site 0, c2 = m1/m3 on site 3
        want[0::2, 0::2] *= f32(2.0)
        want[1::2, 1::2] *= f32(0.5)
    assert np.array_equal(out, want)
    assert np.all(out[2:4, 2:4] == 0.5)
    assert CR.flat_norm(np.full((6, 8), 0.25, f32)) == f32(0.25)


def _literal_cosmetic(frame, lst, step):
    """The sequential loop written out: sorted() medians with the even-size
    conventions (n < 9: float add, then halved in double; else double add)."""
    img = np.array(frame, f32)
    h, w = img.shape
    for pos, typ in lst:
        y, x = divmod(int(pos), w)
        r = 1 if typ == CR.HOT else 2
        vals = []
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                yy, xx = y + dy * step, x + dx * step
                if (dx or dy) and 0 <= yy < h and 0 <= xx < w:
                    vals.append(img[yy, xx])
        n = len(vals)
        if typ == CR.HOT:
            s = 0.0
            for v in vals:
                s += float(v)
            img[y, x] = f32(s / n)
        else:
            s = sorted(vals)
            if n % 2:
                med = float(s[n // 2])
            elif n < 9:
                med = float(f32(s[n // 2 - 1] + s[n // 2])) / 2.0
            else:
                med = (float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0
            img[y, x] = f32(med)
    return img


@pytest.mark.parametrize("cfa", [False, True])
def test_s7_sequential_order_12x9(cfa, oracle):
    """An earlier COLD entry whose window holds a later HOT entry two steps
    away reads that pixel uncorrected; the later HOT entry then reads the
    corrected COLD pixel's neighbourhood.  Corners (n = 8), edges (14) and the
    interior (24) all occur."""
    rng = np.random.default_rng(11)
    w, h = 12, 9
    step = 2 if cfa else 1
    frame = rng.random((h, w)).astype(f32)
    cold_p = 4 * w + 4
    hot_p = cold_p + 2 * step                 # same row, two steps to the right: inside the COLD window only
    frame.ravel()[hot_p] = 50.0
    # the HOT pixel's own neighbours are low, so its corrected value falls
    # below the COLD window's median: the order of the two entries shows
    j = 0
    for dy in (-step, 0, step):
        for dx in (-step, 0, step):
            if dx or dy:
                j += 1
                frame[4 + dy, hot_p - 4 * w + dx] = 0.001 * j
    lst = [(0, CR.COLD), (w - 1, CR.HOT), (5, CR.COLD), (cold_p, CR.COLD), (hot_p, CR.HOT),
           ((h - 1) * w, CR.COLD), ((h - 1) * w + w - 1, CR.COLD)]
    lst = sorted(lst)
    got = CR.cosmetic(frame, np.array(lst, np.int32), cfa)
    want = _literal_cosmetic(frame, lst, step)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the COLD entry saw the uncorrected 50.0 (order matters): correcting the
    # HOT pixel first gives another frame whenever 50.0 moved the median
    swapped = [e for e in lst if e[0] != hot_p]
    swapped.insert(swapped.index((cold_p, CR.COLD)), (hot_p, CR.HOT))
    other = _literal_cosmetic(frame, swapped, step)
    assert got.ravel()[hot_p] != 50.0
    assert got.ravel()[cold_p] != other.ravel()[cold_p]
    untouched = np.ones(h * w, bool)
    untouched[[p for p, _ in lst]] = False
    assert np.array_equal(got.ravel()[untouched], frame.ravel()[untouched])


def test_calibrate_command_parsing():
    from siril_amd.calibration import parse_calibrate_command as P
    c = P("calibrate light -dark=dark_stacked -flat=pp_flat_stacked -cc=dark 3 3 -cfa -equalize_cfa -opt".split())
    assert (c.seq, c.dark, c.flat, c.bias, c.bias_level) == ("light", "dark_stacked", "pp_flat_stacked", None, None)
    assert c.cc and c.cc_sigma == (3.0, 3.0) and c.cfa and c.equalize_cfa and c.opt and c.prefix == "pp_"
    c = P(["light", "-bias=bias_stacked", "-prefix=cal_"])
    assert c.bias == "bias_stacked" and c.prefix == "cal_" and not c.cc and not c.opt and c.dark is None
    c = P(["light", '-bias="=500"'])
    assert c.bias is None and f32(c.bias_level) == f32(500) * (f32(1.0) / f32(65535.0))
    c = P(["light", "-dark=d", "-cc=dark", "-1", "2.5", "-cfa"])
    assert c.cc_sigma == (-1.0, 2.5) and c.cfa
    c = P(["light", "-dark=d", "-cc=dark"])
    assert c.cc and c.cc_sigma == (3.0, 3.0)
    for bad in (["light", "-cc=dark"], ["light", "-opt"], ["light", "-cc=bpm"], ["light", "-debayer"],
                ["light", "-dark=d", "-cc=dark", "3"], ["light", "-frobnicate"], ["-dark=d"], []):
        with pytest.raises(ValueError):
            P(bad)


def test_cli_dispatches_on_the_first_word(monkeypatch):
    from siril_amd import calibration, cli
    seen = []
    monkeypatch.setattr(calibration, "run_calibrate", lambda words: (seen.append(list(words)), ("x.seq", None))[1])
    assert cli.main(["calibrate", "light", "-dark=d"]) == 0
    assert seen == [["calibrate", "light", "-dark=d"]]
    assert cli.main(["frobnicate"]) == 2


def test_s3_search_recovers_k():
    k_true = (0.6, 1.0, 1.45)
    frames, dark = CR.synth_optim_case(k_true=k_true)
    for fr, kt in zip(frames, k_true):
        cnt = []
        k = CR.dark_optimize(fr, dark, count=cnt)
        assert k.dtype == np.float32
        assert cnt == [15]
        assert abs(float(k) - kt) < 0.01, (float(k), kt)


def test_s3_area_is_the_central_square():
    assert CR.optim_area(530, 516) == (9, 2, 512, 512)
    assert CR.optim_area(97, 53) == (0, 0, 97, 53)
    assert CR.optim_area(513, 512) == (0, 0, 513, 512)

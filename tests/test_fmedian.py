"""The median filter without a GPU: the refusals of sgpu_fmedian_check at
their exact boundary, the parser of `fmedian`, and the restatement
(tests/median_ref.py) itself on answers known beforehand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_ref as MR  # noqa: E402

F = np.float32


# ---- refusals ------------------------------------------------------------------
def test_check_refusals_and_exact_boundary():
    from siril_amd import SgpuError
    from siril_amd.filters import check_fmedian
    check_fmedian(8, 8, 15)                         # r = 7 = min - 1
    for w, h in ((7, 9), (9, 7)):
        with pytest.raises(SgpuError) as e:
            check_fmedian(w, h, 15)
        assert e.value.code != 0 and "too small" in str(e.value)
        check_fmedian(w, h, 13)
    for ksize in (1, 2, 4, 14, 16, 17, 0, -3):
        with pytest.raises(SgpuError):
            check_fmedian(100, 100, ksize)
    for ksize in (3, 5, 7, 9, 11, 13, 15):
        check_fmedian(100, 100, ksize)
    for mod in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(SgpuError):
            check_fmedian(100, 100, 3, mod)
    for mod in (0.0, 1.0, 0.3):
        check_fmedian(100, 100, 3, mod)
    for it in (0, 9, -1):
        with pytest.raises(SgpuError):
            check_fmedian(100, 100, 3, 1.0, it)
    check_fmedian(100, 100, 3, 1.0, 1)
    check_fmedian(100, 100, 3, 1.0, 8)
    check_fmedian(65535, 2, 3)
    for w, h in ((65536, 4), (4, 65536), (0, 4), (4, 0)):
        with pytest.raises(SgpuError):
            check_fmedian(w, h, 3)
    for w in range(1, 12):
        for ksize in range(1, 18):
            ok = MR.check(w, w + 2, ksize) is None
            try:
                check_fmedian(w, w + 2, ksize)
                assert ok, (w, ksize)
            except SgpuError:
                assert not ok, (w, ksize)


# ---- parser --------------------------------------------------------------------
def test_parse_fmedian():
    from siril_amd.filters import parse_fmedian_command as P
    c = P("fmedian stack 3 1".split())
    assert (c.image, c.ksize, c.modulation, c.iterations, c.out) == ("stack", 3, 1.0, 1, "")
    c = P(["stack.fit", "15", "0.25", "-iter=8", "-out=/tmp/clean.fit"])
    assert (c.image, c.ksize, c.modulation, c.iterations, c.out) == ("stack.fit", 15, 0.25, 8, "/tmp/clean.fit")
    for bad in ("fmedian", "fmedian stack", "fmedian stack 3", "fmedian stack 4 1", "fmedian stack 1 1",
                "fmedian stack 17 1", "fmedian stack x 1", "fmedian stack 3 y", "fmedian stack 3 1.001",
                "fmedian stack 3 -0.001", "fmedian stack 3 nan", "fmedian stack 3 1 -iter=0", "fmedian stack 3 1 -iter=9",
                "fmedian stack 3 1 -iter=two", "fmedian stack 3 1 -out=", "fmedian stack 3 1 -bogus",
                "fmedian stack 3 1 extra", "fmedian -out=a 3 1"):
        with pytest.raises(ValueError):
            P(bad.split())


# ---- the restatement on known answers -------------------------------------------
def test_constant_plane_is_unchanged():
    x = np.full((2, 9, 11), 0.375, F)
    for ksize in (3, 9, 15):
        for mod in (1.0, 0.3):
            assert MR.same(MR.fmedian(x, ksize, mod, 2), x)


def test_one_hot_pixel():
    x = np.full((12, 13), 0.25, F)
    hot = F(0.875)
    x[5, 6] = hot
    assert MR.same(MR.fmedian(x, 3, 1.0), np.full((12, 13), 0.25, F))
    got = MR.fmedian(x, 3, 0.5)
    want = np.full((12, 13), 0.25, F)
    want[5, 6] = F(0.5) * F(0.25) + F(0.5) * hot
    assert MR.same(got, want)
    # ... and at a modulation whose complement rounds: the three operations one by one
    got = MR.fmedian(x, 3, 0.3)
    keep = F(1.0) - F(0.3)
    assert got[5, 6] == F(F(0.3) * F(0.25)) + F(keep * hot)
    assert got[0, 0] == F(F(0.3) * F(0.25)) + F(keep * F(0.25))


def test_centre_of_nine_distinct_values():
    x = np.array([[9, 2, 7], [4, 8, 1], [6, 3, 5]], F)
    assert MR.fmedian(x, 3)[1, 1] == F(5)
    # the corner's window, reflected, holds 8 four times, 2 and 4 twice and 9 once: the fifth smallest is 8
    assert MR.fmedian(x, 3)[0, 0] == F(8)


def test_order_of_special_values():
    bits = np.array([0xFFC00001, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00001],
                    np.uint32)
    k = MR.key(bits.view(F))
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(MR.unkey(k).view(np.uint32), bits)
    # a row of these nine, ksize 3: the median of each window keeps its bits, the NaN payloads too
    row = np.array([0x7FC00001, 0x7FC00001, 0x80000000, 0x00000000, 0xFFC00001], np.uint32).view(F)
    x = np.tile(row, (3, 1))
    got = MR.fmedian(x, 3).view(np.uint32)
    assert got[1, 1] == 0x7FC00001 and got[1, 2] == 0x00000000 and got[1, 3] == 0x80000000


def test_iterations_compose():
    x = MR.scene(20, 23, seed=1)
    assert MR.same(MR.fmedian(x, 5, 0.3, 3), MR.fmedian(MR.fmedian(MR.fmedian(x, 5, 0.3), 5, 0.3), 5, 0.3))
    w = MR.scene(20, 23, seed=2, word=True)
    assert MR.same(MR.fmedian(w, 3), MR.fmedian(MR.to_float(w), 3))

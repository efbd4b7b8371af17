"""The edge-preserving (guided) filter without a GPU: the refusals of
sgpu_epf_check at their exact boundary, the d = 0 rule, the parser of `epf`,
and the restatement (tests/epf_ref.py) itself on answers known beforehand.
The tests of the restatement alone need nothing of the library; they pin the
contract the other epf tests compare the library with."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epf_ref as ER  # noqa: E402
import median_ref as MR  # noqa: E402

F = np.float32
NAN, INF = float("nan"), float("inf")
G = ER.GUIDED


def _refused(*args):
    from siril_amd import SgpuError
    from siril_amd.filters import check_epf
    try:
        check_epf(*args)
        return None
    except SgpuError as e:
        assert e.code != 0
        return str(e)


# ---- refusals ------------------------------------------------------------------
def test_check_refusals_and_exact_boundary():
    assert _refused(13, 13, G, 25, 0.1, 3.0) is None            # r = 12 = min - 1
    for w, h in ((12, 14), (14, 12)):
        assert "too small" in _refused(w, h, G, 25, 0.1, 3.0)
        assert _refused(w, h, G, 23, 0.1, 3.0) is None
    for d in (1, 2, 4, 24, 26, 27, -3):
        assert "d must be" in _refused(100, 100, G, d, 0.1, 3.0)
    for d in (0,) + tuple(range(3, 26, 2)):
        assert _refused(100, 100, G, d, 0.1, 3.0) is None
    for mode in (-1, 2):
        assert "mode" in _refused(100, 100, mode, 3, 0.1, 3.0)
    assert "bilateral filter is not built" in _refused(100, 100, ER.BILATERAL, 3, 0.1, 3.0)
    for si in (0.0, -0.1, NAN, INF, -INF):
        assert "si must" in _refused(100, 100, G, 3, si, 3.0)
    assert _refused(100, 100, G, 3, 5e-324, 3.0) is None
    for ss in (0.0, -1.0, NAN, INF):
        assert "ss must" in _refused(100, 100, G, 0, 0.1, ss)     # d = 0 reads ss
        assert _refused(100, 100, G, 3, 0.1, ss) is None          # a d of its own does not
    for mod in (-0.001, 1.001, NAN, INF, -INF):
        assert "modulation" in _refused(100, 100, G, 3, 0.1, 3.0, mod)
    for mod in (0.0, 1.0, 0.3):
        assert _refused(100, 100, G, 3, 0.1, 3.0, mod) is None
    assert _refused(65535, 2, G, 3, 0.1, 3.0) is None
    for w, h in ((65536, 4), (4, 65536), (0, 4), (4, 0)):
        assert _refused(w, h, G, 3, 0.1, 3.0) is not None
    for w in range(1, 15):
        for d in range(-1, 28):
            for mode in (0, 1):
                assert (ER.check(w, w + 2, mode, d, 0.1, 9.0) is None) == (_refused(w, w + 2, mode, d, 0.1, 9.0) is None)


def test_the_window_of_d_zero():
    for ss, d in ((0.3, 3), (1.0, 5), (3.0, 11), (9.0, 25), (0.01, 3), (1e300, 25), (0.5, 3), (0.9, 3), (1.1, 5)):
        assert ER.window(0, ss) == d
        r = (d - 1) // 2
        assert _refused(r + 1, r + 1, G, 0, 0.1, ss) is None
        assert "too small" in _refused(r, r + 1, G, 0, 0.1, ss)
        assert "too small" in _refused(r + 1, r, G, 0, 0.1, ss)
    assert ER.window(7, 9.0) == 7


# ---- parser --------------------------------------------------------------------
def test_parse_epf():
    from siril_amd.filters import parse_epf_command as P
    c = P("epf stack".split())
    assert (c.image, c.guided, c.d, c.si, c.ss, c.modulation, c.guideimage, c.out) == \
        ("stack", False, 0, 0.02, 3.0, 1.0, "", "")
    c = P(["stack.fit", "-guided", "-d=25", "-si=0.1", "-ss=2.5", "-mod=0.25", "-guideimage=lum.fit",
           "-out=/tmp/smooth.fit"])
    assert (c.image, c.guided, c.d, c.si, c.ss, c.modulation, c.guideimage, c.out) == \
        ("stack.fit", True, 25, 0.1, 2.5, 0.25, "lum.fit", "/tmp/smooth.fit")
    assert P("epf stack -d=0".split()).d == 0
    for bad in ("epf", "epf -guided", "epf stack -d=4", "epf stack -d=1", "epf stack -d=27", "epf stack -d=x",
                "epf stack -d=", "epf stack -si=0", "epf stack -si=-1", "epf stack -si=nan", "epf stack -si=inf",
                "epf stack -si=y", "epf stack -ss=0", "epf stack -ss=nan", "epf stack -mod=1.001", "epf stack -mod=-0.1",
                "epf stack -mod=nan", "epf stack -mod=", "epf stack -out=", "epf stack -guided -guideimage=",
                "epf stack -bogus", "epf stack extra", "epf stack -guideimage=lum.fit"):
        with pytest.raises(ValueError):
            P(bad.split())
    with pytest.raises(ValueError, match="needs -guided"):
        P("epf stack -guideimage=lum.fit".split())


def test_a_line_without_guided_is_refused():
    from siril_amd.filters import run_epf
    with pytest.raises(ValueError, match="bilateral filter is not built"):
        run_epf("epf stack -d=5")


# ---- the restatement on known answers -------------------------------------------
def test_constant_plane_is_unchanged():
    for x in (np.full((2, 14, 15), 0.25, F), np.full((2, 14, 15), 16384, np.uint16)):
        for d in (3, 9, 25):
            for si in (0.01, 0.1, 1.0):
                for mod in (1.0, 0.3):
                    got = ER.epf(x, d, si, 3.0, mod)
                    assert got.dtype == F and MR.same(got, ER.centre(x)), (x.dtype, d, si, mod)
    assert ER.centre(np.array([16384], np.uint16))[0] == F(16384.0 / 65535.0)


def test_modulation_zero_returns_the_input():
    x = MR.scene(20, 23, seed=3)
    w = MR.scene(20, 23, seed=4, word=True)
    assert MR.same(ER.epf(x, 5, 0.1, 2.0, 0.0), x)
    assert MR.same(ER.epf(w, 5, 0.1, 2.0, 0.0), ER.centre(w))


def test_a_nan_spreads_over_its_windows():
    """E3 has no special path: the NaN reaches a and b of every window that holds it, and the result of every window
    that holds one of those."""
    x = MR.scene(20, 23, seed=5).copy()
    x.view(np.uint32)[7, 9] = 0x7FC01234
    got = ER.epf(x, 3, 0.1, 3.0)
    want = np.zeros(x.shape, bool)
    want[5:10, 7:12] = True
    assert np.array_equal(np.isnan(got), want)


def test_guided_by_itself_equals_guided_by_a_copy():
    x = MR.scene(20, 23, seed=6)
    w = MR.scene(20, 23, seed=7, word=True)
    for v in (x, w):
        assert MR.same(ER.epf(v, 5, 0.1), ER.epf(v, 5, 0.1, guide=v.copy()))
    # another guide gives another result
    assert not MR.same(ER.epf(x, 5, 0.1), ER.epf(x, 5, 0.1, guide=w))

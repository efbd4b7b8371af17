"""Frame warp, host side (no GPU): the coefficient tables and the
destination -> source maps of sgpu_warp_frames_device against the numpy
restatement of the specification (tests/warp_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as WR  # noqa: E402
from warp_ref import perspective_H, rotation_H, translation_H  # noqa: E402


@pytest.mark.parametrize("interp,taps", [(0, 1), (1, 2), (2, 4), (3, 2), (4, 8)])
def test_warp_table(interp, taps):
    """Tap counts 2, 2 (AREA), 4, 8 (and the trivial 1 of NEAREST); phase 0
    exactly a unit impulse; every phase within 1 float ulp of the numpy
    formula (the double sin/cos may differ in their last bit)."""
    from siril_amd import registration as Rg
    tab = Rg.warp_table(interp)
    assert tab.shape == (32, taps) and tab.dtype == np.float32
    impulse = np.zeros(taps, np.float32)
    impulse[max(taps // 2 - 1, 0)] = 1
    assert np.array_equal(tab[0], impulse)
    ref = WR.table(interp)
    ulp = np.spacing(np.maximum(np.abs(tab), np.abs(ref)))
    assert np.all(np.abs(tab.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    if interp in (1, 3):
        assert np.array_equal(tab, Rg.warp_table(1))
    if interp != 4:                      # float-only formulas: no libm in them
        assert np.array_equal(tab.view(np.uint32), ref.view(np.uint32))
    assert np.allclose(tab.sum(1), 1, atol=1e-6)


def test_warp_table_refuses_none():
    from siril_amd import registration as Rg
    from siril_amd._lib import SgpuError
    for interp in (-1, 5):
        with pytest.raises(SgpuError) as e:
            Rg.warp_table(interp)
        assert e.value.code == -21          # SGPU_BAD_ARGUMENT


@pytest.mark.parametrize("ref_index", [0, 1, 2])
@pytest.mark.parametrize("height", [53, 5, 1, 4000])
def test_warp_inverse_maps(ref_index, height):
    """Bit-equal to the restatement: identity, integer and sub-pixel
    translations, the 1.5 degree rotation plus shift, the mild perspective."""
    from siril_amd import registration as Rg
    w = 97
    sets = [
        [np.eye(3), translation_H(3, -7), translation_H(-12, 5)],
        [translation_H(0.25, -0.5), translation_H(2, 1), translation_H(-3.75, 2.125)],
        [rotation_H(w, height, 1.5, 2.3, -4.1), translation_H(1, 2), rotation_H(w, height, -1.5, 0.5, 0.25)],
        [perspective_H(w, height), rotation_H(w, height, 0.2, 0, 0), translation_H(0.5, 0.5)],
    ]
    for Hs in sets:
        got = Rg.warp_inverse_maps(Hs, ref_index, height)
        ref = WR.inverse_maps(Hs, ref_index, height)
        assert got.shape == (3, 9)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    # the reference frame maps onto itself; an integer translation is the gather form of
    # shift_frames: dest (x, y) <- src (x - h02, y + h12) in bottom-up rows
    M = Rg.warp_inverse_maps(sets[0], 0, height)
    assert np.array_equal(M[0], np.eye(3).ravel())
    assert np.array_equal(M[1], [1, 0, -3, 0, 1, -7, 0, 0, 1])


def test_warp_inverse_maps_refusals():
    from siril_amd import registration as Rg
    from siril_amd._lib import SgpuError
    sing = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]])
    nan = np.eye(3)
    nan[1, 2] = np.nan
    for Hs, ref in (([np.eye(3), sing], 0), ([np.eye(3), sing], 1), ([nan, np.eye(3)], 1),
                    ([np.eye(3), np.zeros((3, 3))], 0)):
        with pytest.raises(SgpuError) as e:
            Rg.warp_inverse_maps(Hs, ref, 53)
        assert e.value.code == -21          # SGPU_BAD_ARGUMENT
        with pytest.raises(ValueError):
            WR.inverse_maps(Hs, ref, 53)

"""The `epf` command end to end on the GPU: the written image read back equals
filters.epf on the same array and the restatement (tests/epf_ref.py), for a
16-bit mono and a 32-bit three-layer image, with and without -guideimage=;
-out= and the default output name; bad lines, a line without -guided among
them, are refused with a message that says why, and write nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epf_ref as ER  # noqa: E402
import median_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def test_word_mono_image(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.filters import epf
    from siril_amd.sequence import read_fits, write_fits
    x = MR.scene(71, 97, seed=60, word=True)
    write_fits(str(tmp_path / "stack.fit"), x)
    assert cli.main(["epf", str(tmp_path / "stack"), "-guided"]) == 0
    assert "stack_epf.fit" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == ["stack.fit", "stack_epf.fit"]
    got = read_fits(str(tmp_path / "stack_epf.fit"))
    want = epf(_dev(x[None]), guided=True)[0].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(ER.epf(x)))         # the defaults: d = 0, si = 0.02, ss = 3


def test_three_layer_float_image_guided_and_out(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.filters import epf, run_epf
    from siril_amd.sequence import read_fits, write_fits
    x = np.stack([MR.scene(65, 80, seed=61 + c) for c in range(3)])
    write_fits(str(tmp_path / "rgb.fit"), x)
    out = str(tmp_path / "smooth.fit")
    assert cli.main(["epf", str(tmp_path / "rgb.fit"), "-guided", "-d=7", "-si=0.1", "-mod=0.3", f"-out={out}"]) == 0
    assert out in capsys.readouterr().out
    got = read_fits(out)
    want = epf(_dev(x[None]), 7, 0.1, modulation=0.3, guided=True)[0].cpu().numpy()
    assert got.shape == (3, 65, 80) and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(ER.epf(x, 7, 0.1, modulation=0.3)))
    assert not os.path.exists(tmp_path / "rgb_epf.fit")
    res = run_epf(f"epf {tmp_path / 'rgb'} -guided -d=0 -si=0.05 -ss=1.5")
    assert res == str(tmp_path / "rgb_epf.fit")
    assert np.array_equal(_bits(read_fits(res)), _bits(ER.epf(x, 0, 0.05, 1.5)))


def test_guide_image(tmp_path):
    from siril_amd.filters import run_epf
    from siril_amd.sequence import read_fits, write_fits
    x = np.stack([MR.scene(65, 80, seed=61 + c) for c in range(3)])
    g = np.stack([MR.scene(65, 80, seed=71 + c, word=True) for c in range(3)])
    m = MR.scene(65, 80, seed=64, word=True)
    write_fits(str(tmp_path / "rgb.fit"), x)
    write_fits(str(tmp_path / "lum.fit"), g)
    write_fits(str(tmp_path / "mono.fit"), m)
    write_fits(str(tmp_path / "monoguide.fit"), x[0])
    res = run_epf(f"epf {tmp_path / 'rgb'} -guided -d=9 -si=0.2 -guideimage={tmp_path / 'lum'}")
    assert res == str(tmp_path / "rgb_epf.fit")
    assert np.array_equal(_bits(read_fits(res)), _bits(ER.epf(x, 9, 0.2, guide=g)))
    res = run_epf(f"epf {tmp_path / 'mono.fit'} -guided -d=3 -guideimage={tmp_path / 'monoguide.fit'}")
    assert res == str(tmp_path / "mono_epf.fit")
    assert np.array_equal(_bits(read_fits(res)), _bits(ER.epf(m, 3, guide=x[0])))


def test_bad_lines(tmp_path):
    from siril_amd.filters import run_epf
    from siril_amd.sequence import write_fits
    write_fits(str(tmp_path / "tiny.fit"), MR.scene(5, 40, seed=64))
    write_fits(str(tmp_path / "other.fit"), MR.scene(6, 40, seed=65))
    write_fits(str(tmp_path / "layers.fit"), np.stack([MR.scene(5, 40, seed=66 + c) for c in range(3)]))
    t = tmp_path / "tiny"
    for line, why in ((f"epf {t} -guided -d=11", "too small"),      # 5 rows are too few for a radius of 5
                      (f"epf {t} -guided", "too small"),            # ... and for the default window of 11
                      (f"epf {t} -d=3", "bilateral filter is not built"),
                      (f"epf {tmp_path / 'absent'} -guided", "no such image"),
                      (f"epf {t} -guided -bogus", "Unexpected argument"),
                      (f"epf {t} -guided -d=4", "-d= must be"),
                      (f"epf {t} -guided -d=3 -si=0", "-si= must be"),
                      (f"epf {t} -guided -d=3 -mod=1.5", "-mod= must be"),
                      (f"epf {t} -d=3 -guideimage={tmp_path / 'other'}", "needs -guided"),
                      (f"epf {t} -d=3 -guided -guideimage={tmp_path / 'absent'}", "no such image"),
                      (f"epf {t} -d=3 -guided -guideimage={tmp_path / 'other'}", "the guide image is"),
                      (f"epf {t} -d=3 -guided -guideimage={tmp_path / 'layers'}", "the guide image is"),
                      ("epf", "needs an image")):
        with pytest.raises(ValueError, match=why):
            run_epf(line)
    assert not [f for f in os.listdir(tmp_path) if "epf" in f]

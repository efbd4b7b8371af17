"""The `fmedian` command end to end on the GPU: the written image read back
equals filters.fmedian on the same array, for a 16-bit mono and a 32-bit
three-layer image; -iter=, -out= and the default output name; bad lines are
refused and write nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def test_word_mono_image(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.filters import fmedian
    from siril_amd.sequence import read_fits, write_fits
    x = MR.scene(71, 97, seed=60, word=True)
    write_fits(str(tmp_path / "stack.fit"), x)
    assert cli.main(["fmedian", str(tmp_path / "stack"), "3", "1"]) == 0
    assert "stack_fmedian.fit" in capsys.readouterr().out
    got = read_fits(str(tmp_path / "stack_fmedian.fit"))
    want = fmedian(_dev(x[None]), 3)[0].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(MR.fmedian(x, 3)))


def test_three_layer_float_image_iter_and_out(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.filters import fmedian, run_fmedian
    from siril_amd.sequence import read_fits, write_fits
    x = np.stack([MR.scene(65, 80, seed=61 + c) for c in range(3)])
    write_fits(str(tmp_path / "rgb.fit"), x)
    out = str(tmp_path / "clean.fit")
    assert cli.main(["fmedian", str(tmp_path / "rgb.fit"), "7", "0.3", "-iter=2", f"-out={out}"]) == 0
    assert out in capsys.readouterr().out
    got = read_fits(out)
    want = fmedian(_dev(x[None]), 7, 0.3, 2)[0].cpu().numpy()
    assert got.shape == (3, 65, 80) and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(MR.fmedian(x, 7, 0.3, 2)))
    assert not os.path.exists(tmp_path / "rgb_fmedian.fit")
    res = run_fmedian(f"fmedian {tmp_path / 'rgb'} 5 0.5")
    assert res == str(tmp_path / "rgb_fmedian.fit")
    assert np.array_equal(_bits(read_fits(res)), _bits(fmedian(_dev(x[None]), 5, 0.5)[0].cpu().numpy()))


def test_bad_lines(tmp_path):
    from siril_amd.filters import run_fmedian
    from siril_amd.sequence import write_fits
    write_fits(str(tmp_path / "tiny.fit"), MR.scene(5, 40, seed=64))
    for line in (f"fmedian {tmp_path / 'tiny'} 11 1",           # 5 rows are too few for a radius of 5
                 f"fmedian {tmp_path / 'absent'} 3 1",
                 f"fmedian {tmp_path / 'tiny'} 3 1 -bogus",
                 f"fmedian {tmp_path / 'tiny'} 4 1",
                 f"fmedian {tmp_path / 'tiny'} 3 1.5",
                 f"fmedian {tmp_path / 'tiny'} 3 1 -iter=9",
                 f"fmedian {tmp_path / 'tiny'} 3"):
        with pytest.raises(ValueError):
            run_fmedian(line)
    assert not [f for f in os.listdir(tmp_path) if "fmedian" in f]

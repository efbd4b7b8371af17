"""The `wavelet` and `wrecons` commands end to end on the GPU: the written
planes read back equal wavelets.atrous on the same array, the written
reconstruction equals the fused call, for a float mono image, a three-layer
float image and a WORD image; bad lines are refused."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavelet_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def test_wavelet_then_read_back(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.sequence import read_fits, write_fits
    from siril_amd.wavelets import atrous
    x = WR.scene(71, 97, seed=40)
    write_fits(str(tmp_path / "moon.fit"), x)
    assert cli.main(["wavelet", str(tmp_path / "moon"), "4", "2"]) == 0
    assert "moon_wavelet1.fit" in capsys.readouterr().out
    want = atrous(_dev(x[None]), 4, 2)[0].cpu().numpy()
    assert np.array_equal(_bits(want), _bits(WR.transform(x, 4, 2)))
    for k in range(4):
        got = read_fits(str(tmp_path / f"moon_wavelet{k + 1}.fit"))
        assert got.dtype == np.float32 and got.shape == x.shape
        assert np.array_equal(_bits(got), _bits(want[k])), k
    assert not os.path.exists(tmp_path / "moon_wavelet5.fit")


def test_three_layer_image_and_prefix(tmp_path):
    from siril_amd.sequence import read_fits, write_fits
    from siril_amd.wavelets import atrous, run_wavelet, run_wrecons, wrecons
    x = np.stack([WR.scene(65, 80, seed=41 + c) for c in range(3)])
    write_fits(str(tmp_path / "rgb.fit"), x)
    out = run_wavelet(f"wavelet {tmp_path / 'rgb.fit'} 3 1 -prefix=w_")
    assert out == [str(tmp_path / f"w_rgb_wavelet{k}.fit") for k in (1, 2, 3)]
    want = atrous(_dev(x[None]), 3, 1)[0].cpu().numpy()         # [3, n, H, W]
    for k in range(3):
        got = read_fits(out[k])
        assert got.shape == (3, 65, 80) and np.array_equal(_bits(got), _bits(want[:, k])), k
    res = run_wrecons(["wrecons", str(tmp_path / "rgb"), "2.5", "1.5", "1", "-type=1"])
    assert res == str(tmp_path / "rgb_wrecons.fit")
    assert np.array_equal(_bits(read_fits(res)), _bits(wrecons(_dev(x[None]), (2.5, 1.5, 1.0), 1)[0].cpu().numpy()))


def test_wrecons_of_a_word_image(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.sequence import read_fits, write_fits
    from siril_amd.wavelets import wrecons
    x = WR.scene(71, 97, seed=45, word=True)
    write_fits(str(tmp_path / "sun.fit"), x)
    out = str(tmp_path / "sharp.fit")
    assert cli.main(["wrecons", str(tmp_path / "sun.fit"), "3", "2", "1.5", "1", "1", "1", f"-out={out}"]) == 0
    assert out in capsys.readouterr().out
    got = read_fits(out)
    want = wrecons(_dev(x[None]), (3, 2, 1.5, 1, 1, 1))[0].cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(WR.wrecons(x, (3, 2, 1.5, 1, 1, 1))))


def test_bad_lines(tmp_path):
    from siril_amd.sequence import write_fits
    from siril_amd.wavelets import run_wavelet, run_wrecons
    write_fits(str(tmp_path / "tiny.fit"), WR.scene(20, 40, seed=46))
    for line in (f"wavelet {tmp_path / 'tiny'} 6 2",            # 20 rows are too few for six layers
                 f"wavelet {tmp_path / 'absent'} 3 2",
                 f"wavelet {tmp_path / 'tiny'} 3 2 -bogus",
                 f"wavelet {tmp_path / 'tiny'} 3"):
        with pytest.raises(ValueError):
            run_wavelet(line)
    for line in (f"wrecons {tmp_path / 'tiny'} 1 1 1 1 1 1",
                 f"wrecons {tmp_path / 'absent'} 1 1",
                 f"wrecons {tmp_path / 'tiny'} 1 1 -clamp",
                 f"wrecons {tmp_path / 'tiny'}"):
        with pytest.raises(ValueError):
            run_wrecons(line)
    assert not [f for f in os.listdir(tmp_path) if "wavelet" in f or "wrecons" in f]

"""The stretch commands end to end on the GPU: each of `mtf`, `autostretch`,
`linstretch`, `asinh`, `ght`, `invght`, `modasinh`, `invmodasinh` on a small
FITS file, 16- and 32-bit, one and three layers; the written image read back
equals the Python call on the same array bit for bit; the default output name
and -out=; bad lines are refused and write nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _image(layers, h, w, word, seed):
    rng = np.random.RandomState(seed)
    k = np.stack([rng.permutation(h * w) for _ in range(max(layers, 1))])
    x = np.array([0.1, 0.2, 0.15])[:max(layers, 1), None] + 0.2 * (k / float(h * w)) ** 2
    x = np.rint(x * 65535.0).astype(np.uint16) if word else x.astype(np.float32)
    return x.reshape((layers, h, w) if layers else (h, w))


def _calls():
    from siril_amd import stretch as ST
    return (("mtf {img} 0.05 0.2 0.9", lambda t: ST.mtf(t, 0.05, 0.2, 0.9)),
            ("mtf {img} 0 0.3 1 RB", lambda t: ST.mtf(t, 0.0, 0.3, 1.0, channels="RB")),
            ("autostretch {img}", lambda t: ST.autostretch(t)[0]),
            ("autostretch {img} -linked -1.5 0.3", lambda t: ST.autostretch(t, True, -1.5, 0.3)[0]),
            ("linstretch {img} -BP=0.08", lambda t: ST.linstretch(t, 0.08)),
            ("asinh {img} 50", lambda t: ST.asinh(t, 50.0)),
            ("asinh {img} -human 200 0.05", lambda t: ST.asinh(t, 200.0, 0.05, human=True)),
            ("ght {img} -D=5 -B=3 -LP=0.01 -SP=0.1 -HP=0.9", lambda t: ST.ght(t, 5.0, 3.0, 0.01, 0.1, 0.9)),
            ("ght {img} -D=5 -B=-1.5 -SP=0.1 -human", lambda t: ST.ght(t, 5.0, -1.5, SP=0.1, model="human")),
            ("ght {img} -D=5 -SP=0.1 -even -clipmode=rescale G",
             lambda t: ST.ght(t, 5.0, SP=0.1, model="even", clipmode="rescale", channels="G")),
            ("invght {img} -D=2 -B=3 -SP=0.1 -human -clipmode=clip",
             lambda t: ST.invght(t, 2.0, 3.0, SP=0.1, model="human", clipmode="clip")),
            ("modasinh {img} -D=4 -SP=0.1 -HP=0.8", lambda t: ST.modasinh(t, 4.0, SP=0.1, HP=0.8)),
            ("invmodasinh {img} -D=4 -SP=0.1 -HP=0.8 -independent", lambda t: ST.invmodasinh(t, 4.0, SP=0.1, HP=0.8)))


@pytest.mark.parametrize("layers,word", ((0, True), (0, False), (3, True), (3, False)))
def test_every_command_writes_what_the_python_call_returns(tmp_path, capsys, layers, word):
    from siril_amd import cli
    from siril_amd.sequence import read_fits, write_fits
    x = _image(layers, 21, 33, word, seed=70 + layers + word)
    write_fits(str(tmp_path / "stack.fit"), x)
    for line, call in _calls():
        words = line.format(img=str(tmp_path / "stack")).split()
        assert cli.main(words) == 0
        default = tmp_path / f"stack_{words[0]}.fit"
        assert str(default) in capsys.readouterr().out
        got = read_fits(str(default))
        want = call(_dev(x[None]))[0].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == x.shape
        assert R.float32_bits_equal(got, want), line
        assert got.min() >= 0.0 and got.max() <= 1.0
        os.remove(default)


def test_out_names_the_file_and_the_result_is_the_restatements(tmp_path, capsys):
    from siril_amd import cli
    from siril_amd.sequence import read_fits, write_fits
    from siril_amd.stretch import run_stretch
    x = _image(3, 21, 33, False, seed=80)
    write_fits(str(tmp_path / "rgb.fit"), x)
    out = str(tmp_path / "shown.fit")
    assert cli.main(["ght", str(tmp_path / "rgb.fit"), "-D=5", "-B=3", "-SP=0.1", "-human", f"-out={out}"]) == 0
    assert out in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "rgb_ght.fit")
    want = R.stretch(R.Params(R.GHT, D=5.0, B=3.0, SP=0.1, model=R.HUMAN), x[None])[0]
    assert R.float32_bits_equal(read_fits(out), want)
    res = run_stretch(f"invght {tmp_path / 'shown'} -D=5 -B=3 -SP=0.1 -human")
    assert res == str(tmp_path / "shown_invght.fit")
    back = R.stretch(R.Params(R.INVGHT, D=5.0, B=3.0, SP=0.1, model=R.HUMAN), want[None])[0]
    assert R.float32_bits_equal(read_fits(res), back)


def test_bad_lines(tmp_path):
    from siril_amd.sequence import write_fits
    from siril_amd.stretch import run_stretch
    flat = np.full((9, 12), 0.25, np.float32)
    write_fits(str(tmp_path / "flat.fit"), flat)
    write_fits(str(tmp_path / "tiny.fit"), _image(0, 9, 12, False, seed=81))
    for line in (f"autostretch {tmp_path / 'flat'}",                # no spread: MAD = 0
                 f"mtf {tmp_path / 'absent'} 0 0.5 1",
                 f"mtf {tmp_path / 'tiny'} 0.5 0.5 0.5",
                 f"ght {tmp_path / 'tiny'} -D=11",
                 f"ght {tmp_path / 'tiny'} -D=1 -bogus",
                 f"ght {tmp_path / 'tiny'}",
                 f"modasinh {tmp_path / 'tiny'} -D=1 -B=2",
                 f"asinh {tmp_path / 'tiny'} 0.5",
                 f"linstretch {tmp_path / 'tiny'}"):
        with pytest.raises(ValueError):
            run_stretch(line)
    assert sorted(os.listdir(tmp_path)) == ["flat.fit", "tiny.fit"]

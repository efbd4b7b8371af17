"""The `seqsubsky` command end to end on the GPU: a 4-frame 16-bit mono
sequence and a 2-frame 3-layer float sequence, every written plane bit for bit
against background.subsky on the same arrays, the .seq against write_seq; the
refusals; a planted linear gradient is removed to below 1 % of its slope; a
frame whose fit fails stops the command before the .seq is written."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_scenes as BS  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def test_mono_word_sequence(tmp_path, capsys):
    from siril_amd import cli, synth
    from siril_amd.background import subsky
    from siril_amd.sequence import read_fits, write_seq
    w, h = 200, 150
    frames = np.stack([BS.plane(w, h, p % 3, True, seed=p // 3) for p in range(4)])
    seq = synth.write_sequence(str(tmp_path), frames, name="pp_light_")
    assert cli.main(["seqsubsky", seq[:-4], "2", "-samples=20", "-nodither"]) == 0
    line = capsys.readouterr().out.strip()
    want, info = subsky(_dev(frames), 2, 20, 1.0)
    want = want.cpu().numpy()
    assert "bkg_pp_light_.seq" in line and f"{int(info['kept'].min())} .. {int(info['kept'].max())}" in line
    for f in range(4):
        got = read_fits(str(tmp_path / f"bkg_pp_light_{f + 1:05d}.fit"))
        assert got.dtype == np.float32 and got.shape == (h, w)
        assert np.array_equal(_bits(got), _bits(want[f])), f
    write_seq(str(tmp_path / "want.seq"), "bkg_pp_light_", 4)
    assert open(tmp_path / "bkg_pp_light_.seq").read() == open(tmp_path / "want.seq").read()


def test_rgb_float_sequence_in_batches(tmp_path):
    from siril_amd import synth
    from siril_amd.background import run_seqsubsky, subsky
    from siril_amd.sequence import read_fits, write_seq
    w, h = 131, 77
    frames = np.stack([np.stack([BS.plane(w, h, p, False, seed=f) for p in range(3)]) for f in range(2)])
    seq = synth.write_sequence(str(tmp_path), frames, name="rgb_")
    # one frame per batch
    out_seq, info = run_seqsubsky(f"seqsubsky {seq} 1 -samples=10 -tolerance=3 -prefix=b_", max_batch_bytes=1)
    assert out_seq == str(tmp_path / "b_rgb_.seq") and info["kept"].shape == (2, 3) and not info["status"].any()
    want, winfo = subsky(_dev(frames), 1, 10, 3.0)
    want = want.cpu().numpy()
    assert np.array_equal(info["kept"], winfo["kept"])
    for f in range(2):
        got = read_fits(str(tmp_path / f"b_rgb_{f + 1:05d}.fit"))
        assert got.dtype == np.float32 and got.shape == (3, h, w)
        assert np.array_equal(_bits(got), _bits(want[f])), f
    write_seq(str(tmp_path / "want.seq"), "b_rgb_", 2, nb_layers=3)
    assert open(out_seq).read() == open(tmp_path / "want.seq").read()


def test_refusals_and_failed_fit(tmp_path):
    from siril_amd import synth
    from siril_amd.background import run_seqsubsky
    w, h = 131, 77
    frames = np.stack([BS.plane(w, h, p, False) for p in range(3)])
    frames[1] = 0.0                             # nothing to fit: status 1
    seq = synth.write_sequence(str(tmp_path), frames, name="l_")
    for opt, word in (("-rbf", "-rbf"), ("-smooth=0.5", "-smooth"), ("-dither", "-dither")):
        with pytest.raises(ValueError) as e:
            run_seqsubsky(f"seqsubsky {seq} 1 {opt}")
        assert word in str(e.value)
    with pytest.raises(ValueError) as e:
        run_seqsubsky(f"seqsubsky {seq} 1 -samples=10")
    assert "l_00002.fit" in str(e.value) and "status 1" in str(e.value)
    assert not (tmp_path / "bkg_l_.seq").exists()
    ser = synth.write_sequence(str(tmp_path / "ser"), np.zeros((2, 30, 40), np.uint16), name="s_", kind="ser")
    with pytest.raises(ValueError) as e:
        run_seqsubsky(f"seqsubsky {ser} 1")
    assert "SER" in str(e.value)


def test_planted_gradient_is_removed(tmp_path):
    """A linear gradient of amplitude 0.05 across the frame plus noise: the
    slope of the least-squares plane through the output is below 1 % of the
    planted one, and the level is kept."""
    from siril_amd import synth
    from siril_amd.background import run_seqsubsky
    from siril_amd.sequence import read_fits
    w, h = 200, 150
    rng = np.random.RandomState(3)
    x = np.arange(w, dtype=np.float64)[None, :] / (w - 1)
    frames = (0.2 + 0.05 * x + rng.normal(0.0, 0.001, (2, h, w))).astype(np.float32)
    seq = synth.write_sequence(str(tmp_path), frames, name="g_")
    run_seqsubsky(f"seqsubsky {seq} 1")
    xx, yy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    A = np.stack([xx.ravel(), yy.ravel(), np.ones(w * h)], axis=1)
    for f in range(2):
        got = read_fits(str(tmp_path / f"bkg_g_{f + 1:05d}.fit")).astype(np.float64)
        planted = np.linalg.lstsq(A, frames[f].astype(np.float64).ravel(), rcond=None)[0]
        left = np.linalg.lstsq(A, got.ravel(), rcond=None)[0]
        assert abs(planted[0] * (w - 1) - 0.05) < 1e-3
        assert abs(left[0]) < 0.01 * abs(planted[0]) and abs(left[1]) * (h - 1) < 0.01 * 0.05
        assert abs(got.mean() - frames[f].mean()) < 1e-4

"""`register ... -psf=moments|gaussian|moffat`: the option's parsing (no GPU)
and, on the GPU, the fitted fwhm / roundness in the .seq of a four-frame
128 x 96 FITS sequence."""
import numpy as np
import pytest

W, H, N = 128, 96, 4
BG, NOISE = 0.05, 0.002


def test_psf_option_parses_and_defaults_to_moments():
    from siril_amd import registration as Rg
    assert Rg.parse_register_command(["register", "light_"]).psf == "moments"
    for word in ("moments", "gaussian", "moffat"):
        c = Rg.parse_register_command(["register", "light_", "-noout", f"-psf={word}"])
        assert c.psf == word and c.noout and c.transf == "homography"
    for bad in ("-psf=", "-psf=lorentzian", "-psf=Gaussian", "-psf", "-psf=gaussian,moffat"):
        with pytest.raises(ValueError) as e:
            Rg.parse_register_command(["register", "light_", bad])
        assert "aborting" in str(e.value)
    with pytest.raises(ValueError) as e:
        Rg.parse_register_command(["s", "-psf=airy"])
    assert str(e.value) == "Unknown PSF profile airy, aborting."


def test_cli_help_names_the_option():
    from siril_amd import cli
    assert "-psf=moments|gaussian|moffat" in cli.__doc__


def _frames():
    """Four frames of 16 Gaussian stars (sigma 1.4) on a jittered grid, each frame shifted by a sub-pixel."""
    rng = np.random.default_rng(23)
    gx, gy = np.meshgrid(np.linspace(24, W - 24, 4), np.linspace(22, H - 22, 4))
    pts = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-3, 3, (16, 2))
    amps = rng.uniform(0.1, 0.5, 16)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for f, (dx, dy) in enumerate(((0, 0), (1.3, -0.6), (-0.8, 1.7), (2.2, 0.9))):
        img = BG + np.random.default_rng(100 + f).normal(0, NOISE, (H, W))
        for (x, y), a in zip(pts, amps):
            img += a * np.exp(-((xx - x - dx) ** 2 + (yy - y - dy) ** 2) / (2 * 1.4 ** 2))
        out.append(img.astype(np.float32))
    return np.stack(out)


@pytest.mark.gpu
def test_register_psf_writes_the_fitted_values(tmp_path):
    import torch
    from siril_amd import registration as Rg, synth
    from siril_amd.stacking import Context
    frames = _frames()
    ctx = Context(0)
    try:
        seq = synth.write_sequence(str(tmp_path), frames, name="light_")
        out, Hs, info = Rg.run_register(f"register {seq} -psf=gaussian -noout", ctx=ctx)
        Hw, want = Rg.register_stars(torch.from_numpy(frames).cuda(), 0, ctx=ctx, psf="gaussian")
        seq_m = synth.write_sequence(str(tmp_path / "m"), frames, name="light_")
        _, _, info_m = Rg.run_register(f"register {seq_m} -noout", ctx=ctx)
    finally:
        ctx.close()
    assert out == seq and info["registered"].all() and (info["nstars"] >= 14).all()
    assert Hs.tobytes() == Hw.tobytes()
    for k in ("fwhm", "wfwhm", "roundness", "nstars", "npairs"):
        assert np.array_equal(info[k], want[k]), k
    assert len(info["psf"]) == N and all((q["status"] == 0).all() for q in info["psf"])
    rl = [ln.split() for ln in open(seq).read().splitlines() if ln.startswith("R0")]
    assert len(rl) == N
    for f in range(N):
        assert [np.float32(float(v)) for v in rl[f][1:4]] == [np.float32(want[k][f]) for k in
                                                              ("fwhm", "wfwhm", "roundness")]
        assert int(rl[f][6]) == want["nstars"][f]
        assert not (tmp_path / f"r_light_{f + 1:05d}.fit").exists()
    # the fit, not the moments: sigma 1.4 is FWHM 3.297; thresholded moments fall short of it
    assert np.all(np.abs(info["fwhm"] / (1.4 * 2.3548200450309493) - 1) < 0.01)
    assert "psf" not in info_m and np.all(info_m["fwhm"] < 0.95 * info["fwhm"])

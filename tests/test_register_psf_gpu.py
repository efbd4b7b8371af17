"""Star registration with the PSF stage (register_stars(psf=...)) on the three
256 x 192 frames of the star registration test (same recipe, seed 1).

Worst corner displacement of the recovered H from the truth when the
restatements alone run the pipeline on these frames (star_ref finder, psf_ref
fit, stars with status 0, star_ref matcher):

    moments (no fit)   frame 1 0.068 px   frame 2 0.084 px
    psf="gaussian"     frame 1 0.0141 px  frame 2 0.0141 px   (all 30 stars fitted and paired; mean FWHM 3.53,
                                                               planted 3.532; the moments give 3.07)
    psf="moffat"       frame 1 0.0148 px  frame 2 0.0148 px   (29, 29 and 30 stars with status 0, one status 6
                                                               in frames 0 and 1; 28 and 29 pairs; mean FWHM 3.42)

The bound is twice the restatement's figure.  The planted stars are Gaussians,
and a Moffat profile reaches a Gaussian only as beta grows without limit: the
free beta of psf="moffat" runs to its bound of 10, where every overshooting
step is rejected first, and the fits converge there after 54-93 accepted steps.
fit_stars' default cap of 50 would end every one of them with status 1 (all 90
stars dropped, no frame registers), which is why the registration gives the
Moffat stage 200 steps (registration.PSF_REGISTER_MAX_ITER); the restatement
pipeline below runs with the same caps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as PR  # noqa: E402
import psf_scenes as PS  # noqa: E402
import star_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N = PS.RW, PS.RH, PS.RN
BG, NOISE = PS.BG, PS.NOISE
CORNERS = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], float)
RECORDED_CORNER_ERROR = {"gaussian": 0.0142, "moffat": 0.0149}      # measured as above; moments: 0.084
MAX_ITER = {"gaussian": 50, "moffat": 200}        # accepted steps the registration allows a fit


def _corner_error(Hm, Ht):
    return float(np.sqrt(((SR.apply_H(Hm, CORNERS) - SR.apply_H(Ht, CORNERS)) ** 2).sum(1)).max())


@pytest.fixture(scope="module")
def scene():
    return PS.register_scene()


@pytest.fixture(scope="module")
def found(scene):
    """The restatement's star lists, once."""
    return [SR.find_stars(fr, BG, NOISE)[0] for fr in scene[0]]


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_frames(scene):
    import torch
    return torch.from_numpy(scene[0].copy()).cuda()


def _reference_pipeline(scene, found, profile):
    """[(registered, H, npairs)] for frames 1 and 2, and the fitted lists."""
    frames, _ = scene
    lists, td = [], []
    for f in range(N):
        q = PR.fit_stars(frames[f], found[f], BG, profile, max_iter=MAX_ITER[profile])
        m = q["status"] == 0
        lists.append(q[m])
        td.append(np.stack([q["x"][m], (H - 1) - q["y"][m]], 1))
    return [SR.match_stars(td[0], td[f]) for f in (1, 2)], lists


@pytest.mark.parametrize("profile", ["gaussian", "moffat"])
def test_every_frame_registers_within_the_bound(ctx, scene, found, device_frames, profile):
    from siril_amd import registration as Rg
    _, truth = scene
    assert Rg.PSF_REGISTER_MAX_ITER == MAX_ITER
    ref, lists = _reference_pipeline(scene, found, profile)
    Hs, info = Rg.register_stars(device_frames, 0, ctx=ctx, bg=BG, noise=NOISE, psf=profile)
    print(profile, "stars kept", info["nstars"], "restatement keeps", [len(q) for q in lists])
    assert np.array_equal(info["nstars"], [len(q) for q in lists])
    assert info["registered"].all()
    assert np.array_equal(Hs[0], np.eye(3))
    for j, f in enumerate((1, 2)):
        ok, Hr, pairs = ref[j]
        assert ok
        want, err = _corner_error(Hr, truth[f]), _corner_error(Hs[f], truth[f])
        print(f"{profile} frame {f}: corner error {err:.4f} px (restatement {want:.4f}), pairs {info['npairs'][f]}")
        assert want <= RECORDED_CORNER_ERROR[profile]
        assert err < 2 * want and info["npairs"][f] == len(pairs)
    # the registration values come from the fit
    assert info["psf"] is not None and len(info["psf"]) == N
    for f in range(N):
        q, s = info["psf"][f], info["stars"][f]
        assert (q["status"] == 0).all() and len(q) == len(s) == info["nstars"][f] >= 20
        assert np.array_equal(s["x"], q["x"]) and np.array_equal(s["fwhm_major"], q["fwhm_major"])
        assert np.all(np.diff(s["flux"]) <= 0)                                   # still in flux order
        assert info["fwhm"][f] == float(np.sqrt(q["fwhm_major"] * q["fwhm_minor"]).mean())
        assert info["roundness"][f] == float(q["roundness"].mean())
    planted = 1.5 * PR.FWHM_K                                                    # sigma 1.5: FWHM 3.532
    if profile == "gaussian":
        assert np.all(np.abs(info["fwhm"] / planted - 1) < 0.01)
    else:                               # a Moffat at beta = 10 is not quite a Gaussian: nearer than the moments' 3.07
        assert np.all(np.abs(info["fwhm"] - planted) < 0.5 * (planted - 3.07))
        assert all((q["beta"] > 9.9).all() and q["iterations"].max() > 50 for q in info["psf"])
    assert info["wfwhm"][0] > 0 and np.all(info["wfwhm"][1:] >= info["fwhm"][1:] * 0.999)


def test_without_psf_nothing_changes(ctx, scene, found, device_frames):
    """psf=None is the registration as it was: the finder's lists bit for bit,
    the values from the moments, no `psf` entry."""
    from siril_amd import registration as Rg
    Hs, info = Rg.register_stars(device_frames, 0, ctx=ctx, bg=BG, noise=NOISE)
    Hn, infn = Rg.register_stars(device_frames, 0, ctx=ctx, bg=BG, noise=NOISE, psf=None)
    assert Hs.tobytes() == Hn.tobytes() and "psf" not in info and "psf" not in infn
    assert set(info) == {"nstars", "npairs", "registered", "fwhm", "wfwhm", "roundness", "bkg", "stars"}
    for k in ("nstars", "npairs", "registered", "fwhm", "wfwhm", "roundness", "bkg"):
        assert info[k].tobytes() == infn[k].tobytes() and info[k].dtype == infn[k].dtype
    min_pairs = 10
    for f in range(N):
        s = found[f]
        assert info["stars"][f].tobytes() == s.tobytes() == infn["stars"][f].tobytes()
        fw = float(np.sqrt(s["fwhm_major"] * s["fwhm_minor"]).mean())
        assert info["fwhm"][f] == fw and info["roundness"][f] == float(s["roundness"].mean())
        assert info["wfwhm"][f] == fw * (len(found[0]) - min_pairs) / (info["npairs"][f] - min_pairs)
    with pytest.raises(ValueError):
        Rg.register_stars(device_frames, 0, ctx=ctx, bg=BG, noise=NOISE, psf="lorentzian")

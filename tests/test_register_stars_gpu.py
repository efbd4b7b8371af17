"""Star-based global registration end to end on the GPU: find_stars ->
match_stars -> warp_frames on three 256 x 192 frames of 30 planted stars
(mutually >= 14 px apart, rendered analytically through a known H per frame:
frame 1 a 1.5 degree rotation plus a sub-pixel shift, frame 2 with mild
perspective as well), seeded noise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import star_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N = 256, 192, 3
BG, NOISE = 0.05, 0.002
SEED = 1
CORNERS = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], float)
# Worst corner displacement (Euclidean, pixels) of the recovered H from the
# truth when tests/star_ref.py alone runs finder and matcher on these frames
# (seed 1: frame 1 0.068 px, frame 2 0.084 px; all 30 stars paired in both).
# The GPU star lists equal the restatement's bit for bit, so this is a
# property of the method (0.02-0.03 px median centroid error), not of the GPU.
RECORDED_CORNER_ERROR = 0.084
BOUND = 2 * RECORDED_CORNER_ERROR


def _truth():
    cx, cy = (W - 1) / 2, (H - 1) / 2
    c, s = np.cos(np.deg2rad(1.5)), np.sin(np.deg2rad(1.5))
    R = np.array([[c, -s, cx - c * cx + s * cy + 2.3], [s, c, cy - s * cx - c * cy - 1.6], [0, 0, 1.0]])
    c, s = np.cos(np.deg2rad(-1.0)), np.sin(np.deg2rad(-1.0))
    P = np.array([[c, -s, cx - c * cx + s * cy - 1.7], [s, c, cy - s * cx - c * cy + 2.4], [2e-5, -1.5e-5, 1.0]])
    return [np.eye(3), R, P]


@pytest.fixture(scope="module")
def scene():
    """(frames float32 [N, H, W], planted reference positions in memory order, truth Hs)."""
    rng = np.random.default_rng(SEED)
    pts = []
    while len(pts) < 30:
        p = rng.uniform([24, 24], [W - 24, H - 24])
        if all(np.hypot(*(p - q)) >= 14 for q in pts):
            pts.append(p)
    ref_td = np.array(pts)
    amps = rng.uniform(0.1, 0.6, 30)
    Hs = _truth()
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for f in range(N):
        td = SR.apply_H(np.linalg.inv(Hs[f]), ref_td)          # H maps frame pixels to reference pixels
        img = BG + np.random.default_rng(SEED + 100 + f).normal(0, NOISE, (H, W))
        for (x, y), a in zip(td, amps):
            img += a * np.exp(-((xx - x) ** 2 + (yy - ((H - 1) - y)) ** 2) / (2 * 1.5 ** 2))
        frames.append(img.astype(np.float32))
    frames = np.stack(frames)
    frames.setflags(write=False)
    return frames, np.stack([ref_td[:, 0], (H - 1) - ref_td[:, 1]], 1), Hs


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def registered(ctx, scene):
    import torch
    from siril_amd import registration as Rg
    d = torch.from_numpy(scene[0].copy()).cuda()
    Hs, info = Rg.register_stars(d, 0, ctx=ctx, bg=BG, noise=NOISE)
    return d, Hs, info


def _corner_error(Hm, Ht):
    return float(np.sqrt(((SR.apply_H(Hm, CORNERS) - SR.apply_H(Ht, CORNERS)) ** 2).sum(1)).max())


def test_every_frame_registers_within_the_bound(scene, registered):
    frames, _, truth = scene
    _, Hs, info = registered
    assert info["registered"].all()
    assert np.array_equal(Hs[0], np.eye(3))
    assert (info["npairs"][1:] >= 20).all() and (info["nstars"] >= 20).all()
    for f in (1, 2):
        err = _corner_error(Hs[f], truth[f])
        print(f"frame {f}: corner error {err:.4f} px, pairs {info['npairs'][f]}")
        assert err < BOUND
    assert np.all(info["fwhm"] > 2.5) and np.all(info["fwhm"] < 4.5)          # sigma 1.5: FWHM 3.5
    assert np.all(info["roundness"] > 0.8) and np.allclose(info["bkg"], BG)
    assert info["wfwhm"][0] > 0 and np.all(info["wfwhm"][1:] >= info["fwhm"][1:] * 0.999)


def test_star_lists_and_pairs_equal_the_restatement(scene, registered):
    """The reason the bound is a property of the method: same stars bit for
    bit, same pairs, and the restatement's own H is within the recorded error."""
    frames, _, truth = scene
    _, Hs, info = registered
    td = []
    for f in range(N):
        want, _ = SR.find_stars(frames[f], BG, NOISE)
        assert info["stars"][f].tobytes() == want.tobytes()
        td.append(np.stack([want["x"], (H - 1) - want["y"]], 1))
    for f in (1, 2):
        ok, Hr, pairs = SR.match_stars(td[0], td[f])
        assert ok and len(pairs) == info["npairs"][f] >= 20
        assert _corner_error(Hr, truth[f]) <= RECORDED_CORNER_ERROR
        assert _corner_error(Hr, Hs[f]) < 1e-4


def test_warped_stars_land_on_their_reference_positions(ctx, scene, registered):
    from siril_amd import registration as Rg
    _, ref_mem, _ = scene
    d, Hs, _ = registered
    out = Rg.warp_frames(d, Hs, 0, ctx=ctx)
    stars = Rg.find_stars(out, ctx=ctx, bg=BG, noise=NOISE)
    for f in range(N):
        xy = np.stack([stars[f]["x"], stars[f]["y"]], 1)
        dist = np.sqrt(((ref_mem[:, None, :] - xy[None]) ** 2).sum(2)).min(1)
        found = dist < 2.0                                    # this planted star was found in the warped frame
        assert found.sum() >= 20
        print(f"frame {f}: {int(found.sum())} stars, worst residual {dist[found].max():.4f} px")
        assert dist[found].max() < BOUND


def test_unregistered_frame_has_the_null_homography(ctx, scene):
    """A mirrored frame does not register: null H, zero weighted FWHM."""
    import torch
    from siril_amd import registration as Rg
    fr = scene[0][:2].copy()
    fr[1] = fr[1][:, ::-1]
    Hs, info = Rg.register_stars(torch.from_numpy(fr).cuda(), 0, ctx=ctx, bg=BG, noise=NOISE)
    assert list(info["registered"]) == [True, False]
    assert not Hs[1].any() and info["wfwhm"][1] == 0.0


def test_register_command_end_to_end(ctx, scene, tmp_path):
    """`register` on a FITS sequence: the .seq gains the homographies and the
    registration values, the r_ frames are warp_frames of the same H."""
    import torch
    from siril_amd import registration as Rg, synth
    from siril_amd.sequence import read_fits, stack_frames
    frames, _, truth = scene
    seq = synth.write_sequence(str(tmp_path), frames, name="light_")
    out_seq, Hs, info = Rg.run_register(["register", seq], ctx=ctx)
    assert out_seq == str(tmp_path / "r_light_.seq") and info["registered"].all()
    for f in (1, 2):
        assert _corner_error(Hs[f], truth[f]) < BOUND
    rl = [ln.split() for ln in open(seq).read().splitlines() if ln.startswith("R0")]
    assert len(rl) == N
    for f in range(N):
        assert np.array_equal(np.array([float(v) for v in rl[f][8:]]).reshape(3, 3), Hs[f])
        assert int(rl[f][6]) == info["nstars"][f] >= 20 and float(rl[f][1]) > 2.5
    want = Rg.warp_frames(torch.from_numpy(frames.copy()).cuda(), Hs, 0, ctx=ctx).cpu().numpy()
    for f in range(N):
        got = read_fits(str(tmp_path / f"r_light_{f + 1:05d}.fit"))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[f].view(np.uint32))
    assert stack_frames(out_seq) == ([0, 1, 2], 0)
    # -noout writes no frames; a mirrored frame is deselected and left out of the output
    fr = frames.copy()
    fr[2] = fr[2][:, ::-1]
    seq2 = synth.write_sequence(str(tmp_path / "m"), fr, name="m_")
    out2, Hs2, info2 = Rg.run_register(f"register {seq2} -noout -transf=affine", ctx=ctx)
    assert out2 == seq2 and list(info2["registered"]) == [True, True, False] and not Hs2[2].any()
    assert Hs2[1][2, 0] == 0 and Hs2[1][2, 1] == 0
    assert [ln for ln in open(seq2).read().splitlines() if ln.startswith("I ")] == ["I 1 1", "I 2 1", "I 3 0"]
    assert not (tmp_path / "m" / "r_m_00001.fit").exists()
    out3, _, _ = Rg.run_register(f"register {seq2} -interp=li", ctx=ctx)
    assert stack_frames(out3) == ([0, 1], 0) and not (tmp_path / "m" / "r_m_00003.fit").exists()

"""The one-shot-colour path through the commands, on the GPU:
`seqapplyreg -drizzle -cfa=` on a hand-written sequence of five 48 x 36 WORD
mosaics, one of which did not register (files, sizes, layers and the .seq
against drizzle_frames(cfa=)), `stack` of what it wrote (every layer weighed by
its own layer of the weight files, against Context.stack(drizzle=) per layer),
the refusals, and `register -cfa= -noout`.

The register case runs on the three 256 x 192 star frames of
tests/test_register_stars_gpu.py (its scene, by import) turned into RGGB
mosaics: the finder measures stars in boxes of radius 10 and the matcher wants
ten pairs, which a 48 x 36 frame cannot hold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_cfa_ref as CR  # noqa: E402
from test_register_stars_gpu import scene  # noqa: E402,F401  (the fixture)
from warp_ref import rotation_H, translation_H  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N = 48, 36, 5
GOOD = [0, 2, 3, 4]          # frame 1 carries the null homography
REF = 3
SCALE, PIXFRAC = 1.5, 0.7
OW, OH = 72, 54


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return a.view(np.uint32)


def _mosaics():
    """Five dithered WORD mosaics of one smooth scene, the colours at different gains."""
    rng = np.random.default_rng(17)
    gain = np.array([0.6, 1.0, 0.8])[CR.colour_plane("RGGB", W, H)]
    yy, xx = np.mgrid[0:H, 0:W]
    base = 20000 + 15000 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
    return np.stack([(base * gain + rng.normal(0, 300, (H, W))) for _ in range(N)]).astype(np.uint16)


def _homographies():
    return np.stack([translation_H(0.25, 0.25), np.zeros((3, 3)), rotation_H(W, H, 1.5, 0.8, -0.6), np.eye(3),
                     translation_H(-1.4, 0.7)])


@pytest.fixture(scope="module")
def drizzled(ctx, tmp_path_factory):
    """(directory, input .seq, output .seq, frames, Hs, info) of one
    `seqapplyreg -drizzle -cfa=RGGB` run, two frames per batch."""
    from siril_amd import registration as Rg, synth
    from siril_amd.sequence import write_seq
    d = tmp_path_factory.mktemp("cfa")
    frames = _mosaics()
    seq = synth.write_sequence(str(d), frames, name="pp_")
    Hs = _homographies()
    rng = np.random.default_rng(3)
    vals = dict(fwhm=rng.uniform(2, 4, N), wfwhm=rng.uniform(2, 4, N), roundness=rng.uniform(0.5, 1, N),
                quality=rng.uniform(0, 1, N), bkg=rng.uniform(0, 0.1, N), nstars=np.arange(10, 10 + N))
    write_seq(seq, "pp_", N, reference=REF, homographies=Hs, **vals)
    # one input plane and six output planes per frame: room for three, one of them the reference's slot
    out_seq, _, info = Rg.run_seqapplyreg(f"seqapplyreg {seq} -drizzle -cfa=rggb -scale={SCALE} -pixfrac={PIXFRAC}",
                                          ctx=ctx, max_batch_bytes=3 * (H * W * 4 + 6 * OW * OH * 4))
    return d, seq, out_seq, frames, Hs, info


def _written(d):
    from siril_amd.sequence import read_fits
    img = np.stack([read_fits(str(d / f"r_pp_{j + 1:05d}.fit")) for j in range(len(GOOD))])
    wts = np.stack([read_fits(str(d / "drizztmp" / f"oweight_r_pp_{j + 1:05d}.fit")) for j in range(len(GOOD))])
    return img, wts


def test_files_and_seq_equal_drizzle_frames(ctx, drizzled):
    import torch
    from siril_amd import registration as Rg
    from siril_amd.calibration import INV_USHRT_MAX
    d, seq, out_seq, frames, Hs, info = drizzled
    assert out_seq == str(d / "r_pp_.seq") and info["size"] == (OW, OH)
    assert list(info["registered"]) == [True, False, True, True, True]
    assert sum(info["tiles"]) == (len(GOOD) + 1) * ((OW + 21) // 22) * ((OH + 10) // 11)   # the second batch adds the reference
    want, wantw = Rg.drizzle_frames(torch.from_numpy(frames[GOOD].view(np.int16)).cuda(), Hs[GOOD], GOOD.index(REF),
                                    SCALE, PIXFRAC, "square", ctx=ctx, cfa="RGGB")
    want = want.cpu().numpy() * np.float32(INV_USHRT_MAX)
    wantw = wantw.cpu().numpy()
    img, wts = _written(d)
    assert img.dtype == wts.dtype == np.float32 and img.shape == wts.shape == (len(GOOD), 3, OH, OW)
    assert np.array_equal(_bits(img), _bits(want)) and np.array_equal(_bits(wts), _bits(wantw))
    assert img.max() <= 1.0 and all((wts[:, c] > 0).any() and (wts[:, c] == 0).any() for c in range(3))
    assert not (d / "r_pp_00005.fit").exists()
    lines = open(out_seq).read().splitlines()
    assert lines[2] == "S 'r_pp_' 1 4 4 5 2 4 0 0 1"                   # reference renumbered, drizzle_flag set
    assert "L 3" in lines
    inc, H2, v2 = Rg.read_seq_registration(out_seq)
    assert inc.all() and np.array_equal(H2, np.tile(np.eye(3), (4, 1, 1))) and list(v2["nstars"]) == [10, 12, 13, 14]


def test_stack_weighs_every_layer_by_its_own_plane(ctx, drizzled, tmp_path):
    """`stack ... mean` of the three-layer sequence: layer l equals
    Context.stack(frames[:, l], drizzle=weights[:, l]) bit for bit, through the
    command line without rejection and Winsorized over blocks of 10 rows; a
    one-layer weight file serves every layer as before; a two-layer one is the
    sequence error."""
    import shutil
    from siril_amd import SgpuError
    from siril_amd import sequence as Q
    from siril_amd.sequence import _hdu_bytes, read_fits, write_fits
    from siril_amd.stacking import Rejection, StackingArgs
    src = drizzled[0]
    d = tmp_path / "s"
    shutil.copytree(src, d)
    out_seq = str(d / "r_pp_.seq")
    img, wts = _written(d)
    n = img.shape[0]
    assert not np.array_equal(wts[:, 0], wts[:, 1])                    # the layers' weights do differ
    out, _ = Q.run_command(f"stack {out_seq} rej n -nonorm -32b -out={d}/mean.fit", ctx=ctx)
    got = read_fits(out)
    assert got.shape == (3, OH, OW)
    none = StackingArgs(Rejection.NO_REJEC, (3.0, 3.0))
    for layer in range(3):
        want = ctx.stack(np.ascontiguousarray(img[:, layer]), none, drizzle=np.ascontiguousarray(wts[:, layer]))
        assert np.array_equal(_bits(got[layer]), _bits(want.result)), layer
    wz = StackingArgs(Rejection.WINSORIZED, (3.0, 3.0))
    out, counts = Q.stack_seq(out_seq, wz, out=str(d / "wz.fit"), use_32bit_output=True, ctx=ctx,
                              max_block_bytes=n * OW * 8 * 10)
    got = read_fits(out)
    irej = np.zeros(2, np.int64)
    for layer in range(3):
        want = ctx.stack(np.ascontiguousarray(img[:, layer]), wz, drizzle=np.ascontiguousarray(wts[:, layer]))
        assert np.array_equal(_bits(got[layer]), _bits(want.result)), layer
        irej += np.array(want.irej, np.int64)
    assert tuple(counts) == tuple(int(v) for v in irej)
    # one-layer weight files: layer 0 of the file for every layer of the frames
    for j in range(n):
        write_fits(str(d / "drizztmp" / f"oweight_r_pp_{j + 1:05d}.fit"), np.ascontiguousarray(wts[j, 1]))
    out, _ = Q.stack_seq(out_seq, wz, out=str(d / "one.fit"), use_32bit_output=True, ctx=ctx)
    got = read_fits(out)
    for layer in range(3):
        want = ctx.stack(np.ascontiguousarray(img[:, layer]), wz, drizzle=np.ascontiguousarray(wts[:, 1]))
        assert np.array_equal(_bits(got[layer]), _bits(want.result)), layer
    # two layers: neither one plane nor one per layer
    with open(d / "drizztmp" / "oweight_r_pp_00002.fit", "wb") as f:
        f.write(_hdu_bytes(np.ascontiguousarray(wts[1, :2]), True))
    with pytest.raises(SgpuError) as e:
        Q.stack_seq(out_seq, wz, out=str(d / "x.fit"), use_32bit_output=True, ctx=ctx)
    assert e.value.code == -2


def test_parse_refusals(ctx, drizzled, tmp_path):
    from siril_amd import registration as Rg, synth
    seq = drizzled[1]
    assert Rg.parse_seqapplyreg_command(f"seqapplyreg x -drizzle -cfa={CR.XTRANS.lower()}".split()).cfa == CR.XTRANS
    assert Rg.parse_seqapplyreg_command("seqapplyreg x -drizzle".split()).cfa is None
    assert Rg.parse_register_command("register x -cfa=GBRG -noout".split()).cfa == "GBRG"
    for line in (f"seqapplyreg {seq} -cfa=RGGB",                       # -cfa= needs -drizzle
                 f"seqapplyreg {seq} -drizzle -cfa=RGBG",              # no Bayer string
                 f"seqapplyreg {seq} -drizzle -cfa=",
                 f"seqapplyreg {seq} -drizzle -cfa=RGGBRGGB",
                 f"seqapplyreg {seq} -drizzle -cfa={CR.XTRANS[:35]}X"):
        with pytest.raises(ValueError):
            Rg.run_seqapplyreg(line, ctx=ctx)
    for line in (f"register {seq} -cfa=RGGB",                          # -cfa= needs -noout
                 f"register {seq} -cfa=RGGB -interp=li",
                 f"register {seq} -noout -cfa=RGB",
                 f"register {seq} -drizzle -noout"):                    # stays refused
        with pytest.raises(ValueError):
            Rg.run_register(line, ctx=ctx)
    # three-layer frames are no mosaics
    rgb = np.random.default_rng(2).random((2, 3, H, W)).astype(np.float32)
    seq3 = synth.write_sequence(str(tmp_path), rgb, name="rgb_")
    from siril_amd.sequence import write_seq
    write_seq(seq3, "rgb_", 2, nb_layers=3, homographies=np.tile(np.eye(3), (2, 1, 1)))
    with pytest.raises(ValueError, match="one-layer"):
        Rg.run_seqapplyreg(f"seqapplyreg {seq3} -drizzle -cfa=RGGB", ctx=ctx)
    with pytest.raises(ValueError, match="one-layer"):
        Rg.run_register(f"register {seq3} -cfa=RGGB -noout", ctx=ctx)


def test_register_cfa_noout(ctx, scene, tmp_path):  # noqa: F811
    """`register -cfa=RGGB -noout` looks for stars on a copy of every frame
    passed through interpolate_nongreen: the .seq holds exactly the
    homographies register_stars returns for such copies, every frame
    registers, and the files are left as they were."""
    import torch
    from siril_amd import registration as Rg, synth
    frames = scene[0]
    n, h, w = frames.shape
    mosaics = (frames * np.array([0.55, 1.0, 0.7], np.float32)[CR.colour_plane("RGGB", w, h)]).astype(np.float32)
    seq = synth.write_sequence(str(tmp_path), mosaics, name="cfa_")
    names = sorted(p for p in os.listdir(tmp_path) if p.endswith(".fit"))
    before = [open(tmp_path / p, "rb").read() for p in names]
    out, Hs, info = Rg.run_register(f"register {seq} -cfa=RGGB -noout", ctx=ctx)
    assert out == seq and info["registered"].all()
    assert sorted(p for p in os.listdir(tmp_path) if p.endswith(".fit")) == names
    assert [open(tmp_path / p, "rb").read() for p in names] == before
    t = torch.from_numpy(mosaics.copy()).cuda()
    for k in range(n):
        Rg.interpolate_nongreen(t[k], "RGGB", ctx)
    assert not torch.equal(t, torch.from_numpy(mosaics).cuda())
    want, winfo = Rg.register_stars(t, 0, ctx=ctx, model="homography", max_stars=2000, min_pairs=10)
    assert winfo["registered"].all() and np.array_equal(Hs, want)
    assert np.array_equal(info["nstars"], winfo["nstars"]) and np.array_equal(info["npairs"], winfo["npairs"])
    inc, Hseq, _ = Rg.read_seq_registration(seq)
    assert inc.all() and np.array_equal(Hseq, want)
    raw, _ = Rg.register_stars(torch.from_numpy(mosaics.copy()).cuda(), 0, ctx=ctx, model="homography",
                               max_stars=2000, min_pairs=10)
    assert not np.array_equal(raw, want)                                # the interpolation was not a no-op

"""The `seqapplyreg` command end to end on the GPU: `register -noout` then
`seqapplyreg -drizzle` on the three 256 x 192 star frames of
tests/test_register_stars_gpu.py (its scene, by import), the files, sizes and
the .seq flag, frames and weight planes against drizzle_frames; without
-drizzle the output equals `register`'s bit for bit; WORD frames, -flat= and an
unregistered frame on a small hand-written sequence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_register_stars_gpu import N, scene  # noqa: E402,F401  (the fixture)
from warp_ref import rotation_H, translation_H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return a.view(np.uint32)


def test_register_noout_then_drizzle(ctx, scene, tmp_path):  # noqa: F811
    import torch
    from siril_amd import registration as Rg, synth
    from siril_amd.sequence import read_fits
    frames = scene[0]
    h, w = frames.shape[1:]
    seq = synth.write_sequence(str(tmp_path), frames, name="light_")
    _, Hs, info = Rg.run_register(f"register {seq} -noout", ctx=ctx)
    assert info["registered"].all()
    out_seq, Hs2, info2 = Rg.run_seqapplyreg(f"seqapplyreg {seq} -drizzle -scale=2", ctx=ctx)
    assert out_seq == str(tmp_path / "r_light_.seq") and np.array_equal(Hs2, Hs)
    assert info2["size"] == (2 * w, 2 * h) and info2["registered"].all()
    assert sum(info2["tiles"]) == N * ((2 * w + 21) // 22) * ((2 * h + 10) // 11)
    want, wantw = Rg.drizzle_frames(torch.from_numpy(frames.copy()).cuda(), Hs, 0, 2.0, 1.0, "square", ctx=ctx)
    want, wantw = want.cpu().numpy(), wantw.cpu().numpy()
    assert (wantw > 0).mean() > 0.9
    for f in range(N):
        got = read_fits(str(tmp_path / f"r_light_{f + 1:05d}.fit"))
        gotw = read_fits(str(tmp_path / "drizztmp" / f"oweight_r_light_{f + 1:05d}.fit"))
        assert got.dtype == np.float32 and got.shape == (2 * h, 2 * w) and gotw.shape == (2 * h, 2 * w)
        assert np.array_equal(_bits(got), _bits(want[f])) and np.array_equal(_bits(gotw), _bits(wantw[f]))
    lines = open(out_seq).read().splitlines()
    assert lines[2] == f"S 'r_light_' 1 {N} {N} 5 0 4 0 0 1"           # drizzle_flag set
    src = [ln.split() for ln in open(seq).read().splitlines() if ln.startswith("R0")]
    dst = [ln.split() for ln in lines if ln.startswith("R0")]
    assert len(dst) == N
    for f in range(N):
        assert dst[f][:8] == src[f][:8]                                 # registration values carried over
        assert [float(v) for v in dst[f][8:]] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("opts", ["", " -interp=cu -noclamp -prefix=w_"])
def test_without_drizzle_equals_register_output(ctx, scene, tmp_path, opts):  # noqa: F811
    from siril_amd import registration as Rg, synth
    frames = scene[0].copy()
    frames[2] = frames[2][:, ::-1]                  # does not register: left out by both
    a = synth.write_sequence(str(tmp_path / "a"), frames, name="light_")
    b = synth.write_sequence(str(tmp_path / "b"), frames, name="light_")
    out_a, _, info = Rg.run_register(f"register {a}{opts}", ctx=ctx)
    assert list(info["registered"]) == [True, True, False]
    Rg.run_register(f"register {b} -noout", ctx=ctx)
    out_b, _, info_b = Rg.run_seqapplyreg(f"seqapplyreg {b}{opts}", ctx=ctx)
    assert list(info_b["registered"]) == [True, True, False]
    assert open(a).read() == open(b).read()
    assert os.path.basename(out_a) == os.path.basename(out_b) and open(out_a).read() == open(out_b).read()
    names = sorted(n for n in os.listdir(tmp_path / "a") if n.endswith(".fit"))
    assert names == sorted(n for n in os.listdir(tmp_path / "b") if n.endswith(".fit")) and len(names) == 3 + 2
    for n in names:
        assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read(), n
    assert not (tmp_path / "b" / "drizztmp").exists()


def test_drizzle_word_frames_with_flat(ctx, tmp_path):
    """A hand-written .seq: WORD frames (output in [0, 1] units), a master flat
    as pixel weights, a deselected frame, a frame with the null homography,
    the reference in the middle, two frames per batch."""
    import torch
    from siril_amd import registration as Rg, synth
    from siril_amd.calibration import INV_USHRT_MAX
    from siril_amd.sequence import read_fits, write_fits, write_seq
    w, h, n = 45, 23, 5
    rng = np.random.default_rng(8)
    frames = (rng.random((n, h, w)) * 60000).astype(np.uint16)
    seq = synth.write_sequence(str(tmp_path), frames, name="pp_")
    Hs = np.stack([translation_H(0.25, 0.25), np.zeros((3, 3)), rotation_H(w, h, 1.5, 0.8, -0.6), np.eye(3),
                   translation_H(-1.4, 0.7)])
    vals = dict(fwhm=rng.uniform(2, 4, n), wfwhm=rng.uniform(2, 4, n), roundness=rng.uniform(0.5, 1, n),
                quality=rng.uniform(0, 1, n), bkg=rng.uniform(0, 0.1, n), nstars=np.arange(10, 10 + n))
    write_seq(seq, "pp_", n, reference=2, included=[True, False, True, False, True], homographies=Hs, **vals)
    flat = rng.uniform(0.5, 1.5, (h, w)).astype(np.float32)
    flat[2, 3] = 0.0
    write_fits(str(tmp_path / "flat.fit"), flat)
    out_seq, _, info = Rg.run_seqapplyreg(f"seqapplyreg {seq} -drizzle -scale=1.5 -pixfrac=0.7 -kernel=turbo "
                                          "-flat=flat -prefix=dz_", ctx=ctx,
                                          max_batch_bytes=3 * (h * w * 4 + 2 * 68 * 35 * 4))
    good = [0, 2, 4]
    assert list(info["registered"]) == [True, False, True, False, True] and info["size"] == (68, 35)
    pw = Rg.drizzle_flat_weights(flat)
    assert pw[2, 3] == 0 and abs(float(pw.mean()) - 1) < 0.02
    want, wantw = Rg.drizzle_frames(torch.from_numpy(frames[good].view(np.int16)).cuda(), Hs[good], 1, 1.5, 0.7,
                                    "turbo", pixel_weights=torch.from_numpy(pw).cuda(), ctx=ctx)
    want = want.cpu().numpy() * np.float32(INV_USHRT_MAX)
    wantw = wantw.cpu().numpy()
    for j in range(3):
        got = read_fits(str(tmp_path / f"dz_pp_{j + 1:05d}.fit"))
        gotw = read_fits(str(tmp_path / "drizztmp" / f"oweight_dz_pp_{j + 1:05d}.fit"))
        assert got.shape == (35, 68) and got.max() <= 1.0
        assert np.array_equal(_bits(got), _bits(want[j])) and np.array_equal(_bits(gotw), _bits(wantw[j]))
    assert not (tmp_path / "dz_pp_00004.fit").exists()
    lines = open(out_seq).read().splitlines()
    assert lines[2] == "S 'dz_pp_' 1 3 3 5 1 4 0 0 1"
    inc, H2, v2 = Rg.read_seq_registration(out_seq)
    assert inc.all() and np.array_equal(H2, np.tile(np.eye(3), (3, 1, 1)))
    assert list(v2["nstars"]) == [10, 12, 14] and np.array_equal(v2["quality"], vals["quality"][good])
    with pytest.raises(FileNotFoundError):
        Rg.run_seqapplyreg(f"seqapplyreg {seq} -drizzle -flat=missing_flat", ctx=ctx)


def test_stack_of_a_drizzled_sequence(ctx, oracle, tmp_path):
    """The headless `stack` of what `seqapplyreg -drizzle` wrote reads the
    rows of drizztmp/oweight_* with each block as the stack's drizzle weights:
    equal to Context.stack(..., drizzle=) of the same arrays bit for bit
    (several blocks; without rejection through the command line, Winsorized),
    the median stack ignores the planes, -feather= adds its mask planes
    (against the oracle over Siril's block plan), and a missing weight file is
    the sequence error."""
    from oracle import feather_ref as F
    from siril_amd import SgpuError
    from siril_amd import registration as Rg, sequence as Q, synth
    from siril_amd.sequence import read_fits, write_seq
    from siril_amd.stacking import METHOD_MEDIAN, Rejection, StackingArgs
    w, h, n = 45, 23, 6
    rng = np.random.default_rng(4)
    scene = (rng.random((h, w)) * 0.5 + 0.2).astype(np.float32)
    frames = np.stack([scene + rng.normal(0, 0.01, (h, w)).astype(np.float32) for _ in range(n)]).astype(np.float32)
    seq = synth.write_sequence(str(tmp_path), frames, name="l_")
    dith = rng.uniform(-1.5, 1.5, (n, 2))
    dith[0] = 0
    write_seq(seq, "l_", n, homographies=np.stack([translation_H(dx, dy) for dx, dy in dith]))
    out_seq, _, info = Rg.run_seqapplyreg(f"seqapplyreg {seq} -drizzle -scale=2 -pixfrac=0.7", ctx=ctx)
    ow, oh = info["size"]
    img = np.stack([read_fits(str(tmp_path / f"r_l_{f + 1:05d}.fit")) for f in range(n)])
    wts = np.stack([read_fits(str(tmp_path / "drizztmp" / f"oweight_r_l_{f + 1:05d}.fit")) for f in range(n)])
    assert img.shape == (n, oh, ow) and (wts == 0).any() and (wts > 0).mean() > 0.5
    wz = StackingArgs(Rejection.WINSORIZED, (3.0, 3.0))
    out, counts = Q.stack_seq(out_seq, wz, out=str(tmp_path / "wz.fit"), use_32bit_output=True, ctx=ctx,
                              max_block_bytes=n * ow * 8 * 10)              # blocks of 10 rows
    want = ctx.stack(img, wz, drizzle=wts)
    assert np.array_equal(_bits(read_fits(out)), _bits(want.result)) and counts == tuple(want.irej)
    plain = ctx.stack(img, wz)
    assert not np.array_equal(plain.result, want.result)                     # the weights weighted something
    out, _ = Q.run_command(f"stack {out_seq} rej n -nonorm -32b -out={tmp_path}/mean.fit", ctx=ctx)
    want = ctx.stack(img, StackingArgs(Rejection.NO_REJEC, (3.0, 3.0)), drizzle=wts)
    assert np.array_equal(_bits(read_fits(out)), _bits(want.result))
    out, _ = Q.stack_seq(out_seq, StackingArgs(), METHOD_MEDIAN, out=str(tmp_path / "med.fit"),
                         use_32bit_output=True, ctx=ctx)
    want = ctx.stack(img, StackingArgs(), METHOD_MEDIAN)
    assert np.array_equal(_bits(read_fits(out)), _bits(want.result))
    # -feather= too: both planes, over the block plan of 2 threads
    out, _ = Q.stack_seq(out_seq, wz, out=str(tmp_path / "fe.fit"), use_32bit_output=True, ctx=ctx, feather=3,
                         block_threads=2)
    masks = np.stack([F.downscale_blend_mask(img[i]) for i in range(n)])
    ref = np.zeros((oh, ow), np.float32)
    for c, s, bh in F.stack_blocks(oh, (ow, oh, 1), 2):
        r0 = oh - s - bh
        planes = F.block_planes(masks, ow, oh, s, bh, 3.0, shifty=[0] * n, fits_order=True)
        ref[r0:r0 + bh] = oracle.stack_rows(np.ascontiguousarray(img[:, r0:r0 + bh]), 5, (3.0, 3.0), mask=planes,
                                            drizz=np.ascontiguousarray(wts[:, r0:r0 + bh]), nthreads=8)[0]
    assert np.array_equal(_bits(read_fits(out)), _bits(ref))
    os.remove(tmp_path / "drizztmp" / "oweight_r_l_00003.fit")
    with pytest.raises(SgpuError) as e:
        Q.stack_seq(out_seq, wz, out=str(tmp_path / "x.fit"), use_32bit_output=True, ctx=ctx)
    assert e.value.code == -2

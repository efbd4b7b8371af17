"""The wavelet kernels (siril_amd/csrc/wavelet.hip) against the restatement
(tests/wavelet_ref.py), bit for bit: every number of layers and both filters,
shapes one pixel past a tile edge (64 wide, 32 high) each way, several tiles, WORD
input, unaligned and padded strides, NaN / inf / negative samples, the fused
reconstruction against the stored planes, the refusals and the empty call.

The launch forms and the cases that cross their tile edges in both directions:
the grouped tile launch (scales 0-1) and the separate row and column launches
(scales 2 and up, 1024 pixels of a row per workgroup) by 65 x 129, 129 x 65
and 130 x 200 at n = 6, and the row launch's own edge by 9 x 1100 at n = 4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavelet_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

COEF = (3.0, 2.0, 1.5, 1.0, 1.0, 1.0)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _check(x, n, type_, coefs=None):
    """atrous, reconstruct and wrecons of frames x [N, H, W] against the restatement."""
    from siril_amd import wavelets as WV
    coefs = COEF[:n] if coefs is None else coefs
    want = WR.transform(x, n, type_)
    d = _dev(x)
    planes = WV.atrous(d, n, type_)
    _same(planes.cpu().numpy(), want)
    rec = WR.reconstruct(want, coefs)
    _same(WV.reconstruct(planes, coefs).cpu().numpy(), rec)
    _same(WV.wrecons(d, coefs, type_).cpu().numpy(), rec)


def test_every_tap_of_the_last_scale_reflects():
    _check(WR.scene(33, 33, seed=1)[None], 6, 2)


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_every_layer_count_and_type(n, type_):
    _check(np.stack([WR.scene(71, 97, seed=2), WR.scene(71, 97, seed=3)]), n, type_)


@pytest.mark.parametrize("shape", [(65, 129), (129, 65), (130, 200), (9, 1100)])
def test_past_the_tile_edges(shape):
    n = 6 if min(shape) > 32 else 4
    _check(WR.scene(*shape, seed=4)[None], n, 2)
    _check(WR.scene(*shape, seed=5)[None], n, 1)


def test_word_input():
    _check(np.stack([WR.scene(71, 97, seed=6, word=True), WR.scene(71, 97, seed=7, word=True)]), 6, 2)
    _check(WR.scene(72, 136, seed=8, word=True)[None], 5, 1)        # the 8-byte loads


def test_four_dimensional_frames():
    from siril_amd import wavelets as WV
    x = np.stack([WR.scene(40, 52, seed=s) for s in range(6)]).reshape(2, 3, 40, 52)
    planes = WV.atrous(_dev(x), 4)
    assert tuple(planes.shape) == (2, 3, 4, 40, 52)
    _same(planes.cpu().numpy(), WR.transform(x, 4))
    _same(WV.wrecons(_dev(x), COEF[:4]).cpu().numpy(), WR.wrecons(x, COEF[:4]))


@pytest.mark.parametrize("w,pad,offset", [(97, 3, 1), (136, 3, 1), (136, 8, 0), (136, 8, 4)])
def test_strides_and_offsets(w, pad, offset):
    """P = 3 with plane_stride = W*H + pad and the base `offset` samples into its
    buffer: pad 3 / offset 1 takes the one-sample route at either width, pad 8 /
    offset 0 and 4 the 16-byte route."""
    import torch
    from siril_amd import wavelets as WV
    from siril_amd.stacking import Context
    h, P, n = 71, 3, 5
    ps = w * h + pad
    x = np.stack([WR.scene(h, w, seed=10 + p) for p in range(P)])
    want = WR.transform(x, n)
    rec = WR.reconstruct(want, COEF[:n])
    buf = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    for p in range(P):
        buf[offset + p * ps: offset + p * ps + w * h] = _dev(x[p]).reshape(-1)
    ops, ois = ps, n * ps + 4 * (pad % 4 == 0)
    out = torch.full((offset + P * ois,), -7.0, dtype=torch.float32, device="cuda")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    WV.atrous_device(ctx, buf.data_ptr() + 4 * offset, 4, P, w, h, ps, n, 2, out.data_ptr() + 4 * offset, ops, ois)
    got = out.cpu().numpy()
    seen = np.zeros(got.shape, bool)
    for p in range(P):
        for k in range(n):
            a = offset + p * ois + k * ops
            _same(got[a:a + w * h].reshape(h, w), want[p, k])
            seen[a:a + w * h] = True
    assert np.all(got[~seen] == -7.0)               # the padding is not written
    acc = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    WV.wrecons_device(ctx, buf.data_ptr() + 4 * offset, 4, P, w, h, ps, COEF[:n], 2, acc.data_ptr() + 4 * offset, ps)
    rec2 = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    WV.reconstruct_device(ctx, out.data_ptr() + 4 * offset, P, w, h, ops, ois, COEF[:n], rec2.data_ptr() + 4 * offset, ps)
    for res in (acc.cpu().numpy(), rec2.cpu().numpy()):
        seen = np.zeros(res.shape, bool)
        for p in range(P):
            a = offset + p * ps
            _same(res[a:a + w * h].reshape(h, w), rec[p])
            seen[a:a + w * h] = True
        assert np.all(res[~seen] == -7.0)
    ctx.close()


def test_nan_inf_and_negative_samples():
    x = WR.scene(71, 97, seed=20) - np.float32(0.4)
    x[5, 7] = np.nan
    x[40, 90] = np.inf
    x[70, 0] = -np.inf
    x[30, 30] = -3.0e38
    assert (x < 0).sum() > 100
    _check(x[None], 5, 2)
    _check(x[None], 5, 1)


@pytest.mark.parametrize("coefs", [(3.0, 2.0, 1.5, 1.0, 1.0, 1.0), (0.0,) * 6, (-1.0, 2.5, -0.75, 1.0, -2.0, 0.5),
                                   (1.0,) * 6])
def test_coefficient_sets(coefs):
    from siril_amd import wavelets as WV
    x = WR.scene(72, 136, seed=21)[None]
    want = WR.wrecons(x, coefs)
    d = _dev(x)
    got = WV.wrecons(d, coefs)
    _same(got.cpu().numpy(), want)
    _same(WV.reconstruct(WV.atrous(d, 6), coefs).cpu().numpy(), want)
    if coefs == (1.0,) * 6:
        assert np.max(np.abs(want - x)) <= 4 * 5 * 2.0 ** -24 * np.max(np.abs(x))


def test_fused_equals_planes_and_runs_repeat():
    import torch
    from siril_amd import wavelets as WV
    x = _dev(np.stack([WR.scene(130, 200, seed=22), WR.scene(130, 200, seed=23)]))
    for type_ in (1, 2):
        a = WV.wrecons(x, COEF, type_)
        b = WV.reconstruct(WV.atrous(x, 6, type_), COEF)
        c = WV.wrecons(x, COEF, type_, out=torch.full_like(a, 9.0))      # the accumulator's old contents do not matter
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
        assert torch.equal(WV.atrous(x, 6, type_).view(torch.int32), WV.atrous(x, 6, type_).view(torch.int32))


def test_refusals_and_empty_call():
    import torch
    from siril_amd import SgpuError
    from siril_amd import wavelets as WV
    from siril_amd.stacking import Context
    w, h, n = 64, 48, 3
    ctx = Context(0)
    buf = torch.zeros(8 * w * h, dtype=torch.float32, device="cuda")
    p0 = buf.data_ptr()
    # in place, and an output that ends inside the input
    for out in (p0, p0 - 4 * (n * w * h - 8)):
        with pytest.raises(SgpuError):
            WV.atrous_device(ctx, p0, 4, 1, w, h, w * h, n, 2, out, w * h, n * w * h)
    with pytest.raises(SgpuError):
        WV.wrecons_device(ctx, p0, 4, 1, w, h, w * h, (1, 1, 1), 2, p0 + 4 * (w * h - 1), w * h)
    with pytest.raises(SgpuError):
        WV.reconstruct_device(ctx, p0, 1, w, h, w * h, n * w * h, (1, 1, 1), p0 + 4 * 2 * w * h, w * h)
    WV.wrecons_device(ctx, p0, 4, 1, w, h, w * h, (1, 1, 1), 2, p0 + 4 * w * h, w * h)     # adjacent is fine
    # strides, coefficients, sizes
    for call in (lambda: WV.atrous_device(ctx, p0, 4, 1, w, h, w * h - 1, n, 2, p0 + 4 * w * h, w * h, n * w * h),
                 lambda: WV.atrous_device(ctx, p0, 4, 1, w, h, w * h, n, 2, p0 + 4 * w * h, w * h - 1, n * w * h),
                 lambda: WV.atrous_device(ctx, p0, 4, 1, w, h, w * h, n, 2, p0 + 4 * w * h, w * h, n * w * h - 1),
                 lambda: WV.atrous_device(ctx, p0, 3, 1, w, h, w * h, n, 2, p0 + 4 * w * h, w * h, n * w * h),
                 lambda: WV.atrous_device(ctx, p0, 4, 1, w, h, w * h, 7, 2, p0 + 4 * w * h, w * h, 7 * w * h),
                 lambda: WV.atrous_device(ctx, p0, 4, 1, w, 33, w * 33, 6, 3, p0 + 4 * w * h, w * 33, 6 * w * 33),
                 lambda: WV.atrous_device(ctx, p0, 4, 1, w, 32, w * 32, 6, 2, p0 + 4 * w * h, w * 32, 6 * w * 32),
                 lambda: WV.wrecons_device(ctx, p0, 4, 1, w, h, w * h, (1, float("nan"), 1), 2, p0 + 4 * w * h, w * h),
                 lambda: WV.wrecons_device(ctx, p0, 4, 1, w, h, w * h, (1, float("inf"), 1), 2, p0 + 4 * w * h, w * h),
                 lambda: WV.reconstruct_device(ctx, p0, 1, w, h, w * h, n * w * h, (1, 1, float("-inf")),
                                               p0 + 4 * n * w * h, w * h),
                 lambda: WV.atrous_device(ctx, 0, 4, 1, w, h, w * h, n, 2, p0, w * h, n * w * h)):
        with pytest.raises(SgpuError) as e:
            call()
        assert e.value.code != 0
    # the empty call: nothing is touched, nothing was launched
    WV.atrous_device(ctx, 0, 4, 0, w, h, w * h, n, 2, 0, w * h, n * w * h)
    WV.wrecons_device(ctx, 0, 2, 0, w, h, w * h, (1, 1, 1), 2, 0, w * h)
    WV.reconstruct_device(ctx, 0, 0, w, h, w * h, n * w * h, (1, 1, 1), 0, w * h)
    assert WV.last_kernel_ms(ctx) == []
    e = torch.empty((0, h, w), dtype=torch.float32, device="cuda")
    assert tuple(WV.atrous(e, n).shape) == (0, n, h, w) and tuple(WV.wrecons(e, (1, 1, 1)).shape) == (0, h, w)
    with pytest.raises(ValueError):
        WV.wrecons(buf[:w * h].reshape(1, h, w), (1, 1, 1), out=buf[:w * h].reshape(1, h, w).double())
    with pytest.raises(SgpuError):
        x = buf[:w * h].reshape(1, h, w)
        WV.wrecons(x, (1, 1, 1), out=x)
    ctx.close()


def test_launch_forms_of_a_call():
    """What ran: the grouped tile launch, then a row and a column launch per further scale."""
    import torch
    from siril_amd import wavelets as WV
    from siril_amd.stacking import Context
    ctx = Context(0)
    x = _dev(WR.scene(130, 200, seed=30)[None])
    WV.wrecons(x, COEF, ctx=ctx)
    torch.cuda.synchronize()
    ran = WV.last_kernel_ms(ctx)
    assert [r[0] for r in ran].count("tile") >= 1 and sum(r[2] for r in ran if r[0] != "row") == 5
    assert ran[0][:2] == ("tile", 0) and all(r[3] >= 0.0 for r in ran)
    scales = [j for r in ran if r[0] != "row" for j in range(r[1], r[1] + r[2])]
    assert scales == [0, 1, 2, 3, 4]
    WV.reconstruct(WV.atrous(x, 3, ctx=ctx), (1, 1, 1), ctx=ctx)
    assert [r[0] for r in WV.last_kernel_ms(ctx)] == ["recon"]
    ctx.close()

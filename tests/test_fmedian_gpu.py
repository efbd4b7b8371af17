"""The median kernels (siril_amd/csrc/median.hip) against the restatement
(tests/median_ref.py), bit for bit: NaN at the same places and every other
sample equal as uint32 (with modulation 1 the NaN payloads too, the output
being one of the inputs); no tolerance anywhere.

The kernels' tile is 64 wide and 32 high, so the shapes are the issue's: 8 x 8
at ksize 15 (every tap reflects), 4 x 5 at ksize 7, 71 x 97 at every ksize,
and 65 x 129, 129 x 65, 130 x 200, 9 x 1100 one pixel or more past a tile edge
each way.  References are computed once per (scene, parameters) and shared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
KSIZES = (3, 5, 7, 9, 11, 13, 15)
NETWORK_KSIZES = (3, 5, 7)


def _dev(a):
    import torch
    a = np.array(a)         # a copy: the shared scenes are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _same(got, want, payload=True):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    if payload:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _scene(kind, h, w, seed):
    if kind == "plain":
        return _readonly(np.stack([MR.scene(h, w, seed=seed), MR.scene(h, w, seed=seed + 1)]))
    if kind == "word":
        return _readonly(np.stack([MR.scene(h, w, seed=seed, word=True), MR.scene(h, w, seed=seed + 1, word=True)]))
    if kind == "levels":        # four levels: every window is full of duplicates
        return _readonly((np.floor(MR.scene(h, w, seed=seed) * 4.0) / 4.0).astype(F)[None])
    if kind == "three":         # constant but for three pixels
        x = np.full((1, h, w), 0.5, F)
        x[0, 3, 4], x[0, 3, 5], x[0, h - 1, w - 1] = 0.75, 0.25, 0.0
        return _readonly(x)
    assert kind == "special"    # NaN of both signs, +-inf, -0 against +0, negative samples, about 2 % in all
    rng = np.random.RandomState(3000 + seed)
    x = MR.scene(h, w, seed=seed).copy()
    x[rng.rand(h, w) < 0.3] = 0.0       # plenty of +0 for the -0 to be ordered against
    bits = x.view(np.uint32)
    special = np.array([0x7FC00000, 0xFFC00000, 0x7FC01234, 0xFFC04321, 0x7F800000, 0xFF800000, 0x80000000,
                        0xBE800000, 0xBF000000, 0x80000001], np.uint32)
    hit = rng.rand(h, w) < 0.02
    bits[hit] = rng.choice(special, size=int(hit.sum()))
    x[0, 0] = np.array([0xFFC00001], np.uint32).view(F)[0]
    return _readonly(x[None])


@functools.lru_cache(maxsize=None)
def _want(kind, h, w, seed, ksize, mod, it):
    return _readonly(MR.fmedian(_scene(kind, h, w, seed), ksize, mod, it))


def _check(kind, h, w, seed, ksize, mod=1.0, it=1, route=0):
    from siril_amd import filters as FL
    got = FL.fmedian(_dev(_scene(kind, h, w, seed)), ksize, mod, it, route=route).cpu().numpy()
    _same(got, _want(kind, h, w, seed, ksize, mod, it), payload=(mod == 1.0 or kind != "special"))
    return got


def test_every_tap_reflects():
    _check("plain", 8, 8, 1, 15)
    _check("plain", 8, 8, 1, 15, 0.3, 2)
    _check("plain", 4, 5, 3, 7)
    _check("plain", 2, 2, 3, 3)


@pytest.mark.parametrize("mod", [1.0, 0.3])
@pytest.mark.parametrize("ksize", KSIZES)
def test_every_ksize(ksize, mod):
    _check("plain", 71, 97, 5, ksize, mod)


@pytest.mark.parametrize("ksize", [3, 5, 9, 15])
@pytest.mark.parametrize("shape", [(65, 129), (129, 65), (130, 200), (9, 1100)])
def test_past_the_tile_edges(shape, ksize):
    _check("plain", shape[0], shape[1], 7, ksize)


@pytest.mark.parametrize("ksize", [3, 7])
def test_word_input(ksize):
    _check("word", 72, 136, 9, ksize)           # the 8-byte loads
    _check("word", 71, 97, 11, ksize, 0.3)      # one sample per access


def test_four_dimensional_frames():
    from siril_amd import filters as FL
    x = np.stack([MR.scene(40, 52, seed=20 + s) for s in range(6)]).reshape(2, 3, 40, 52)
    got = FL.fmedian(_dev(x), 5, 0.3, 2)
    assert tuple(got.shape) == (2, 3, 40, 52)
    _same(got.cpu().numpy(), MR.fmedian(x, 5, 0.3, 2))


@pytest.mark.parametrize("w,pad,offset", [(97, 3, 1), (136, 3, 1), (136, 8, 0)])
@pytest.mark.parametrize("ksize", [3, 9])
def test_strides_and_offsets(w, pad, offset, ksize):
    """P = 3 with both strides W*H + pad and both bases `offset` samples into
    their buffers: pad 3 / offset 1 takes the one-sample route at either width,
    pad 8 / offset 0 the 16-byte route.  Two iterations pass through the
    workspace.  The padding stays as it was."""
    import torch
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    h, P = 71, 3
    ps = w * h + pad
    x = np.stack([MR.scene(h, w, seed=30 + p) for p in range(P)])
    want = MR.fmedian(x, ksize, 0.3, 2)
    buf = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    for p in range(P):
        buf[offset + p * ps: offset + p * ps + w * h] = _dev(x[p]).reshape(-1)
    before = buf.cpu().numpy()
    out = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    FL.fmedian_device(ctx, buf.data_ptr() + 4 * offset, 4, P, w, h, ps, ksize, 0.3, 2, out.data_ptr() + 4 * offset, ps)
    got = out.cpu().numpy()
    seen = np.zeros(got.shape, bool)
    for p in range(P):
        a = offset + p * ps
        _same(got[a:a + w * h].reshape(h, w), want[p])
        seen[a:a + w * h] = True
    assert np.all(got[~seen] == -7.0)               # the padding is not written
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))    # nor the input
    ctx.close()


@pytest.mark.parametrize("ksize", [3, 5, 7, 15])
def test_ties(ksize):
    _check("levels", 71, 97, 40, ksize)
    _check("levels", 71, 97, 40, ksize, route=2)
    _check("three", 40, 70, 0, ksize)
    _check("three", 40, 70, 0, ksize, route=2)


@pytest.mark.parametrize("ksize", [3, 5, 7, 11])
def test_special_values(ksize):
    _check("special", 71, 97, 50, ksize)            # all bits, NaN payloads included
    _check("special", 71, 97, 50, ksize, 0.3)       # NaN at the same places


@pytest.mark.parametrize("it", [1, 2, 3])
def test_iterations(it):
    _check("plain", 71, 97, 5, 3, 0.3, it)
    _check("plain", 71, 97, 5, 9, 1.0, it)


@pytest.mark.parametrize("ksize", NETWORK_KSIZES)
def test_routes_agree(ksize):
    for scene in (("plain", 71, 97, 5), ("plain", 65, 129, 7), ("special", 71, 97, 50)):
        a = _check(*scene, ksize, route=1)
        b = _check(*scene, ksize, route=2)
        c = _check(*scene, ksize, route=0)
        d = _check(*scene, ksize, route=3)          # the selection over all 32 bits
        for other in (b, c, d):
            assert np.array_equal(a.view(np.uint32), other.view(np.uint32))


def test_route_refusals():
    from siril_amd import SgpuError
    from siril_amd import filters as FL
    d = _dev(_scene("plain", 71, 97, 5))
    for ksize, route in ((9, 1), (15, 1), (3, 4), (3, -1)):
        with pytest.raises(SgpuError):
            FL.fmedian(d, ksize, route=route)


def test_repeat_runs_are_bit_equal():
    from siril_amd import filters as FL
    d = _dev(_scene("special", 71, 97, 50))
    for ksize in (5, 9):
        a = FL.fmedian(d, ksize, 0.3, 2).cpu().numpy()
        b = FL.fmedian(d, ksize, 0.3, 2).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_and_the_empty_call():
    import torch
    from siril_amd import SgpuError
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    x = _dev(_scene("plain", 71, 97, 5))
    with pytest.raises(SgpuError):
        FL.fmedian(x, 3, out=x)
    for bad in ((4, 1.0, 1), (17, 1.0, 1), (3, 1.001, 1), (3, float("nan"), 1), (3, 1.0, 0), (3, 1.0, 9)):
        with pytest.raises(SgpuError):
            FL.fmedian(x, *bad)
    with pytest.raises(SgpuError):
        FL.fmedian(_dev(_scene("plain", 4, 5, 3)), 9)       # r = 4 > 3
    with pytest.raises(ValueError):
        FL.fmedian(x, 3, out=torch.empty((2, 71, 96), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        FL.fmedian(x.double(), 3)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h, w = 71, 97
    buf = torch.zeros(3 * h * w, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    n = 4 * h * w
    for args in ((p, 4, 2, w, h, h * w, 3, 1.0, 1, p + n - 4, h * w),           # the ranges share one sample
                 (p + n, 4, 2, w, h, h * w, 3, 1.0, 1, p, h * w),               # ... the other way round
                 (p, 4, 1, w, h, h * w - 1, 3, 1.0, 1, p + 2 * n, h * w),       # strides below the plane
                 (p, 4, 1, w, h, h * w, 3, 1.0, 1, p + 2 * n, h * w - 1),
                 (p, 8, 1, w, h, h * w, 3, 1.0, 1, p + 2 * n, h * w),           # element sizes
                 (p, 1, 1, w, h, h * w, 3, 1.0, 1, p + 2 * n, h * w),
                 (0, 4, 1, w, h, h * w, 3, 1.0, 1, p + 2 * n, h * w),           # null planes
                 (p, 4, 1, w, h, h * w, 3, 1.0, 1, 0, h * w)):
        with pytest.raises(SgpuError):
            FL.fmedian_device(ctx, *args)
    FL.fmedian_device(ctx, p, 4, 1, w, h, h * w, 3, 1.0, 1, p + n, h * w)        # adjacent ranges are fine
    FL.fmedian_device(ctx, 0, 4, 0, w, h, h * w, 3, 1.0, 1, 0, h * w)            # the empty call
    assert FL.last_kernel_ms(ctx) == []
    empty = torch.empty((0, h, w), dtype=torch.float32, device="cuda")
    assert tuple(FL.fmedian(empty, 3).shape) == (0, h, w)
    torch.cuda.synchronize()
    ctx.close()


def test_last_kernel_ms():
    import torch
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    ctx = Context(0)
    d = _dev(_scene("plain", 71, 97, 5))
    FL.fmedian(d, 5, 0.3, 3, ctx=ctx)
    ms = FL.last_kernel_ms(ctx)
    assert [(r, k) for r, k, _ in ms] == [("network", 5)] * 3 and all(t > 0.0 for _, _, t in ms)
    FL.fmedian(d, 9, 1.0, 1, ctx=ctx)
    ms = FL.last_kernel_ms(ctx)
    assert [(r, k) for r, k, _ in ms] == [("select", 9)] and ms[0][2] > 0.0
    FL.fmedian(d, 3, 1.0, 2, ctx=ctx, route=3)
    assert [(r, k) for r, k, _ in FL.last_kernel_ms(ctx)] == [("select-wide", 3)] * 2
    torch.cuda.synchronize()
    ctx.close()

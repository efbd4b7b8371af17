"""The guided filter's kernels (siril_amd/csrc/epf.hip) against the restatement
(tests/epf_ref.py) on all 32 bits of every sample: NaN at the same places and
every other sample equal as uint32; no tolerance anywhere.

The kernels' tile is 64 wide and 32 high (64 x 16 above d = 17), so the shapes
are 13 x 13 at d = 25, 8 x 8 at d = 15 and 4 x 5 at d = 7 (every tap reflects),
71 x 97 at every odd d, and 65 x 129, 129 x 65, 130 x 200, 9 x 1100 one pixel or
more past a tile edge each way, at d on both sides of the change of tile.
References are computed once per (scene, parameters) and shared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epf_ref as ER  # noqa: E402
import median_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DS = tuple(range(3, 26, 2))


def _dev(a):
    import torch
    a = np.array(a)         # a copy: the shared scenes are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _scene(kind, h, w, seed):
    if kind == "plain":
        return _readonly(MR.scene(h, w, seed=seed)[None])
    if kind == "word":
        return _readonly(MR.scene(h, w, seed=seed, word=True)[None])
    assert kind == "special"    # NaN of both signs, +-inf, -0 against +0, negative samples, about 2 % in all
    rng = np.random.RandomState(3000 + seed)
    x = MR.scene(h, w, seed=seed).copy()
    x[rng.rand(h, w) < 0.3] = 0.0
    bits = x.view(np.uint32)
    special = np.array([0x7FC00000, 0xFFC00000, 0x7FC01234, 0xFFC04321, 0x7F800000, 0xFF800000, 0x80000000,
                        0xBE800000, 0xBF000000, 0x80000001], np.uint32)
    hit = rng.rand(h, w) < 0.02
    bits[hit] = rng.choice(special, size=int(hit.sum()))
    x[0, 0] = np.array([0xFFC00001], np.uint32).view(F)[0]
    return _readonly(x[None])


@functools.lru_cache(maxsize=None)
def _want(scene, guide, d, si, ss, mod):
    return _readonly(ER.epf(_scene(*scene), d, si, ss, mod, guide=None if guide is None else _scene(*guide)))


def _check(scene, d, si=0.1, ss=3.0, mod=1.0, guide=None):
    from siril_amd import filters as FL
    got = FL.epf(_dev(_scene(*scene)), d, si, ss, mod, guided=True,
                 guide=None if guide is None else _dev(_scene(*guide))).cpu().numpy()
    _same(got, _want(scene, guide, d, si, ss, mod))
    return got


def test_every_tap_reflects():
    _check(("plain", 13, 13, 1), 25)
    _check(("plain", 13, 13, 1), 25, mod=0.3)
    _check(("plain", 8, 8, 2), 15)
    _check(("plain", 4, 5, 3), 7)
    _check(("plain", 2, 2, 3), 3)
    _check(("plain", 13, 13, 1), 25, guide=("plain", 13, 13, 4))


@pytest.mark.parametrize("d", DS)
def test_every_d(d):
    _check(("plain", 71, 97, 5), d)
    _check(("plain", 71, 97, 5), d, guide=("plain", 71, 97, 6))


@pytest.mark.parametrize("d", [3, 9, 17, 19, 25])
@pytest.mark.parametrize("shape", [(65, 129), (129, 65), (130, 200), (9, 1100)])
def test_past_the_tile_edges(shape, d):
    d = min(d, 2 * min(shape) - 1)          # 9 rows carry a radius of 8
    _check(("plain", shape[0], shape[1], 7), d)
    _check(("plain", shape[0], shape[1], 7), d, guide=("plain", shape[0], shape[1], 8))


def test_the_window_of_d_zero():
    for ss, d in ((0.3, 3), (1.0, 5), (3.0, 11), (9.0, 25)):
        got = _check(("plain", 71, 97, 5), 0, ss=ss)
        assert np.array_equal(got.view(np.uint32), _want(("plain", 71, 97, 5), None, d, 0.1, ss, 1.0).view(np.uint32))


@pytest.mark.parametrize("d", [5, 21])
def test_word_input(d):
    _check(("word", 72, 136, 9), d)               # the 8-byte loads
    _check(("word", 71, 97, 11), d, mod=0.3)      # one sample per access


@pytest.mark.parametrize("d", [3, 9, 23])
def test_guides_of_either_type(d):
    _check(("plain", 72, 136, 12), d, guide=("word", 72, 136, 9))
    _check(("word", 72, 136, 9), d, guide=("plain", 72, 136, 12), mod=0.3)
    _check(("word", 71, 97, 11), d, guide=("word", 71, 97, 13))
    _check(("plain", 71, 97, 5), d, guide=("plain", 71, 97, 6), mod=0.3)


@pytest.mark.parametrize("d", [3, 9, 23])
def test_self_guide_equals_a_guide_equal_to_the_input(d):
    for scene in (("plain", 71, 97, 5), ("plain", 72, 136, 12), ("word", 72, 136, 9), ("special", 71, 97, 50)):
        a = _check(scene, d)
        b = _check(scene, d, guide=scene)
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("si", [0.02, 1e-6, 1.0, 0.3])
def test_sigmas(si):
    _check(("plain", 71, 97, 5), 7, si=si)
    _check(("plain", 71, 97, 5), 7, si=si, mod=0.3, guide=("plain", 71, 97, 6))


def test_four_dimensional_frames():
    from siril_amd import filters as FL
    x = np.stack([MR.scene(40, 52, seed=20 + s) for s in range(6)]).reshape(2, 3, 40, 52)
    g = np.stack([MR.scene(40, 52, seed=30 + s, word=True) for s in range(6)]).reshape(2, 3, 40, 52)
    got = FL.epf(_dev(x), 5, 0.1, 2.0, 0.3, guided=True)
    assert tuple(got.shape) == (2, 3, 40, 52)
    _same(got.cpu().numpy(), ER.epf(x, 5, 0.1, 2.0, 0.3))
    _same(FL.epf(_dev(x), 5, 0.1, guided=True, guide=_dev(g)).cpu().numpy(), ER.epf(x, 5, 0.1, guide=g))


@pytest.mark.parametrize("w,pad,offset", [(97, 3, 1), (136, 3, 1), (136, 8, 0)])
@pytest.mark.parametrize("d,with_guide", [(5, False), (5, True), (21, True)])
def test_strides_and_offsets(w, pad, offset, d, with_guide):
    """P = 3 with every stride W*H + pad and every base `offset` samples into
    its buffer: pad 3 / offset 1 takes the one-sample route at either width,
    pad 8 / offset 0 the 16-byte route.  The guide is laid out in the same
    way.  The padding stays as it was."""
    import torch
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    h, P = 71, 3
    ps = w * h + pad
    x = np.stack([MR.scene(h, w, seed=30 + p) for p in range(P)])
    g = np.stack([MR.scene(h, w, seed=40 + p) for p in range(P)]) if with_guide else None
    want = ER.epf(x, d, 0.1, 3.0, 0.3, guide=g)

    def laid_out(planes):
        buf = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
        for p in range(P):
            buf[offset + p * ps: offset + p * ps + w * h] = _dev(planes[p]).reshape(-1)
        return buf

    buf = laid_out(x)
    gbuf = laid_out(g) if g is not None else None
    before = buf.cpu().numpy()
    out = torch.full((offset + P * ps,), -7.0, dtype=torch.float32, device="cuda")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    FL.epf_device(ctx, buf.data_ptr() + 4 * offset, 4, P, w, h, ps, gbuf.data_ptr() + 4 * offset if g is not None else 0,
                  4 if g is not None else 0, ps if g is not None else 0, ER.GUIDED, d, 0.1, 3.0, 0.3,
                  out.data_ptr() + 4 * offset, ps)
    got = out.cpu().numpy()
    seen = np.zeros(got.shape, bool)
    for p in range(P):
        a = offset + p * ps
        _same(got[a:a + w * h].reshape(h, w), want[p])
        seen[a:a + w * h] = True
    assert np.all(got[~seen] == -7.0)               # the padding is not written
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))    # nor the input
    ctx.close()


@pytest.mark.parametrize("d", [3, 7, 19])
def test_special_values(d):
    scene = ("special", 71, 97, 50)
    _check(scene, d)                                    # NaN at the same places
    _check(scene, d, mod=0.3, guide=("plain", 71, 97, 6))
    _check(("plain", 71, 97, 6), d, guide=scene)


def test_repeat_runs_are_bit_equal():
    from siril_amd import filters as FL
    d = _dev(_scene("special", 71, 97, 50))
    a = FL.epf(d, 9, 0.1, 3.0, 0.3, guided=True).cpu().numpy()
    b = FL.epf(d, 9, 0.1, 3.0, 0.3, guided=True).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_and_the_empty_call():
    import torch
    from siril_amd import SgpuError
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    x = _dev(_scene("plain", 71, 97, 5))
    with pytest.raises(SgpuError, match="bilateral filter is not built"):
        FL.epf(x, 3)
    with pytest.raises(SgpuError):
        FL.epf(x, 3, guided=True, out=x)
    with pytest.raises(SgpuError):
        g = x.clone()
        FL.epf(x, 3, guided=True, guide=g, out=g)
    for bad in ((4, 0.1, 3.0, 1.0), (27, 0.1, 3.0, 1.0), (3, 0.0, 3.0, 1.0), (3, float("nan"), 3.0, 1.0),
                (0, 0.1, 0.0, 1.0), (3, 0.1, 3.0, 1.001), (3, 0.1, 3.0, float("nan"))):
        with pytest.raises(SgpuError):
            FL.epf(x, *bad, guided=True)
    FL.epf(x, 3, 0.1, 0.0, guided=True)                     # ss is read only for d = 0
    with pytest.raises(SgpuError):
        FL.epf(_dev(_scene("plain", 4, 5, 3)), 9, guided=True)      # r = 4 > 3
    with pytest.raises(ValueError):
        FL.epf(x, 3, guide=x.clone())                       # a guide without guided=True
    with pytest.raises(ValueError):
        FL.epf(x, 3, guided=True, guide=_dev(_scene("plain", 65, 129, 7)))
    with pytest.raises(ValueError):
        FL.epf(x, 3, guided=True, out=torch.empty((1, 71, 96), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        FL.epf(x.double(), 3, guided=True)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h, w = 71, 97
    buf = torch.zeros(5 * h * w, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    n = 4 * h * w
    G = ER.GUIDED
    FL.epf_device(ctx, p, 4, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + n, h * w)        # adjacent ranges are fine
    assert len(FL.last_kernel_ms_epf(ctx)) == 2
    for args in ((p, 4, 2, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + n - 4, h * w),        # the ranges share one sample
                 (p + n, 4, 2, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p, h * w),            # ... the other way round
                 (p, 4, 1, w, h, h * w, p + 2 * n, 4, h * w, G, 3, 0.1, 3.0, 1.0, p + 3 * n - 4, h * w),   # ... with the guide
                 (p, 4, 1, w, h, h * w, p + 3 * n, 4, h * w, G, 3, 0.1, 3.0, 1.0, p + 2 * n + 4, h * w),
                 (p, 4, 1, w, h, h * w, 0, 0, 0, ER.BILATERAL, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),        # mode 0 is not built
                 (p, 4, 1, w, h, h * w, p + n, 8, h * w, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),           # the guide's element size
                 (p, 4, 1, w, h, h * w, p + n, 0, h * w, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),
                 (p, 4, 1, w, h, h * w, p + n, 4, h * w - 1, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),       # ... and stride
                 (p, 4, 1, w, h, h * w - 1, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),    # strides below the plane
                 (p, 4, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w - 1),
                 (p, 8, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),        # element sizes
                 (p, 1, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),
                 (p, 4, 1, w, h, h * w, 0, 0, 0, 2, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),        # the mode
                 (p, 4, 1, w, h, h * w, 0, 0, 0, G, 4, 0.1, 3.0, 1.0, p + 2 * n, h * w),        # d
                 (0, 4, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w),        # null planes
                 (p, 4, 1, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, 0, h * w)):
        with pytest.raises(SgpuError):
            FL.epf_device(ctx, *args)
        assert FL.last_kernel_ms_epf(ctx) == []             # the hook describes the refused call
    FL.epf_device(ctx, p, 4, 1, w, h, h * w, p + n, 4, h * w, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w)
    FL.epf_device(ctx, p, 4, 1, w, h, h * w, p, 4, h * w, G, 3, 0.1, 3.0, 1.0, p + 2 * n, h * w)   # the input as its own guide
    FL.epf_device(ctx, 0, 4, 0, w, h, h * w, 0, 0, 0, G, 3, 0.1, 3.0, 1.0, 0, h * w)            # the empty call
    assert FL.last_kernel_ms_epf(ctx) == []
    empty = torch.empty((0, h, w), dtype=torch.float32, device="cuda")
    assert tuple(FL.epf(empty, 3, guided=True).shape) == (0, h, w)
    torch.cuda.synchronize()
    ctx.close()


def test_last_kernel_ms():
    import torch
    from siril_amd import filters as FL
    from siril_amd.stacking import Context
    ctx = Context(0)
    d = _dev(_scene("plain", 71, 97, 5))
    FL.epf(d, 0, 0.1, 3.0, guided=True, ctx=ctx)
    ms = FL.last_kernel_ms_epf(ctx)
    assert [(k, w) for k, w, _ in ms] == [("guided-a", 11), ("guided-b", 11)] and all(t > 0.0 for _, _, t in ms)
    FL.epf(d, 25, 0.1, 3.0, 0.3, guided=True, guide=d.clone(), ctx=ctx)
    assert [(k, w) for k, w, _ in FL.last_kernel_ms_epf(ctx)] == [("guided-a", 25), ("guided-b", 25)]
    torch.cuda.synchronize()
    ctx.close()

"""Calibration on the GPU (siril_amd/csrc/calibrate.hip): every result is
compared with the numpy restatement of the specification (tests/calib_ref.py)
on the bit patterns of every pixel, no tolerance.

Shapes (width x height): 97x53 (odd pixel count: the vector tail runs), 64x1,
530x516 (the dark-optimisation area is the inner 512 x 512 square; several
workgroups) and 12x9 (cosmetic-correction corners and edges).  N = 3 frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(97, 53), (64, 1), (530, 516), (12, 9)]
DTYPES = [np.float32, np.uint16]
BAD_ARGUMENT = -21
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want)), f"{np.count_nonzero(_bits(got) != _bits(want))} samples differ"


_cache = {}


def _case(w, h, dtype):
    """Frames and masters of one shape (the reference inputs, built once)."""
    key = (w, h, np.dtype(dtype).name)
    if key not in _cache:
        rng = np.random.default_rng(w * 1000 + h)
        fr = (2000 + rng.random((3, h, w)) * 50000).astype(np.uint16)
        frames = fr if dtype == np.uint16 else CR.to_float(fr)
        bias = (0.02 + rng.random((h, w)) * 0.005).astype(f32)
        dark = (0.01 + rng.random((h, w)) * 0.01).astype(f32)
        flat = (0.4 + rng.random((h, w)) * 0.5).astype(f32)
        flat.ravel()[::17] = 0.0                    # "no data" samples
        _cache[key] = (frames, bias, dark, flat)
    return _cache[key]


def _masters(ctx, bias=None, level=None, dark=None, flat=None, norm=1.0, **kw):
    from siril_amd import calibration as CAL
    return CAL.prepare_masters(bias=bias if bias is not None else level, dark=dark, flat=flat, norm=norm, ctx=ctx,
                               **kw)


def _ref(frames, bias=None, level=None, dark=None, flat=None, norm=1.0, k=None):
    return np.stack([CR.s2(fr, bias, level, dark, 1.0 if k is None else k[f], flat, norm)
                     for f, fr in enumerate(frames)])


# ---------------------------------------------------------------- S1 + S2
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u16"])
@pytest.mark.parametrize("use_flat", [False, True], ids=["noflat", "flat"])
@pytest.mark.parametrize("use_dark", [False, True], ids=["nodark", "dark"])
@pytest.mark.parametrize("bias_kind", ["none", "plane", "level"])
def test_s2_every_combination(ctx, bias_kind, use_dark, use_flat, dtype):
    from siril_amd import calibration as CAL
    w, h = 97, 53
    frames, bias, dark, flat = _case(w, h, dtype)
    kw = dict(bias=bias if bias_kind == "plane" else None, level=f32(0.0123) if bias_kind == "level" else None,
              dark=dark if use_dark else None, flat=flat if use_flat else None, norm=f32(0.6172))
    out = CAL.calibrate(_gpu(frames), _masters(ctx, **kw), ctx=ctx)
    _same(out.cpu().numpy(), _ref(frames, **kw))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_s2_shapes(ctx, shape, dtype):
    from siril_amd import calibration as CAL
    w, h = shape
    frames, bias, dark, flat = _case(w, h, dtype)
    kw = dict(bias=bias, dark=dark, flat=flat, norm=f32(0.55))
    out = CAL.calibrate(_gpu(frames), _masters(ctx, **kw), ctx=ctx)
    _same(out.cpu().numpy(), _ref(frames, **kw))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u16"])
@pytest.mark.parametrize("offset", [0, 1], ids=["base0", "base1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_s2_frame_stride_and_unaligned_base(ctx, shape, offset, dtype):
    """frame_stride = W*H + 3 (for every shape but 97x53 that puts frames 1 and
    2 off 16-byte alignment), and a base pointer one sample past alignment:
    the scalar path gives the same bits, the gaps are not written."""
    import torch
    from siril_amd import calibration as CAL
    w, h = shape
    frames, bias, dark, flat = _case(w, h, dtype)
    stride = w * h + 3
    buf = np.zeros(offset + 3 * stride, frames.dtype)
    for f in range(3):
        buf[offset + f * stride: offset + f * stride + w * h] = frames[f].ravel()
    d_in = _gpu(buf)
    d_out = torch.full((offset + 3 * stride,), -7.0, dtype=torch.float32, device="cuda")
    k = np.array([0.5, 1.0, 1.25], f32)
    d_k = torch.from_numpy(k).cuda()
    m = _masters(ctx, bias=bias, dark=dark, flat=flat, norm=f32(0.55))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    CAL.calibrate_device(ctx, d_in.data_ptr() + offset * d_in.element_size(), d_out.data_ptr() + offset * 4,
                         d_in.element_size(), 3, w, h, stride, m, d_k=d_k.data_ptr())
    got = d_out.cpu().numpy()
    want = np.full(offset + 3 * stride, -7.0, f32)
    ref = _ref(frames, bias=bias, dark=dark, flat=flat, norm=f32(0.55), k=k)
    for f in range(3):
        want[offset + f * stride: offset + f * stride + w * h] = ref[f].ravel()
    _same(got, want)


def test_s2_nan_out_given_and_in_place(ctx):
    import torch
    from siril_amd import calibration as CAL
    w, h = 97, 53
    frames, bias, dark, flat = _case(w, h, np.float32)
    frames = frames.copy()
    frames[1, 7, 5] = np.nan
    frames[2, 0, 1] = -0.25
    frames[0, h - 1, w - 1] = 3.5                   # above 1: no clamp
    kw = dict(level=f32(0.01), dark=dark, flat=flat, norm=f32(1.5))
    want = _ref(frames, **kw)
    assert np.isnan(want[1, 7, 5]) and np.nanmax(want) > 1 and np.nanmin(want) < 0
    m = _masters(ctx, **kw)
    d = _gpu(frames)
    out = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    r = CAL.calibrate(d, m, out=out, ctx=ctx)
    assert r is out
    _same(out.cpu().numpy(), want)
    _same(d.cpu().numpy(), frames)                  # the input is left alone
    r = CAL.calibrate(d, m, out=d, ctx=ctx)         # float frames may be calibrated in place
    _same(d.cpu().numpy(), want)


# ---------------------------------------------------------------------- S3
_optim = {}


def _optim_case(w, h, dtype):
    key = (w, h, np.dtype(dtype).name)
    if key not in _optim:
        frames, dark = CR.synth_optim_case(w, h, dtype=dtype)
        k = np.array([CR.dark_optimize(fr, dark, level=f32(0.03)) for fr in frames], f32)
        _optim[key] = (frames, dark, k)
    return _optim[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u16"])
@pytest.mark.parametrize("shape", [(97, 53), (530, 516), (40, 600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_s3_dark_optimisation(ctx, shape, dtype):
    """Three frames with k_true 0.6, 1.0, 1.45 in one call: k and the
    calibrated frames equal the restatement's.  40 x 600: the whole frame is
    the area and has more rows than the workgroup has threads."""
    from siril_amd import calibration as CAL
    w, h = shape
    frames, dark, k_ref = _optim_case(w, h, dtype)
    assert np.all(np.abs(k_ref - np.array([0.6, 1.0, 1.45])) < 0.01)
    m = _masters(ctx, level=f32(0.03), dark=dark)
    out, k = CAL.calibrate(_gpu(frames), m, dark_optim=True, ctx=ctx)
    assert k.dtype == np.float32
    _same(k, k_ref)
    _same(out.cpu().numpy(), _ref(frames, level=f32(0.03), dark=dark, k=k_ref))
    _same(CAL.dark_optimize(_gpu(frames), m, ctx=ctx), k_ref)


def test_s3_area_is_the_inner_square(ctx):
    """530 x 516: pixels outside the central 512 x 512 square do not move k."""
    from siril_amd import calibration as CAL
    w, h = 530, 516
    frames, dark, k_ref = _optim_case(w, h, np.uint16)
    fr = frames.copy()
    inner = np.zeros((h, w), bool)
    inner[2:514, 9:521] = True
    fr[:, ~inner] = 65535
    m = _masters(ctx, level=f32(0.03), dark=dark)
    _same(CAL.dark_optimize(_gpu(fr), m, ctx=ctx), k_ref)
    fr = frames.copy()
    fr[:, 2, 9] = 65535                             # the square's first pixel does
    k2 = CAL.dark_optimize(_gpu(fr), m, ctx=ctx)
    _same(k2, np.array([CR.dark_optimize(x, dark, level=f32(0.03)) for x in fr], f32))


# ------------------------------------------------------------- S4, S5, S6
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_s4_region_stats(ctx, shape):
    from siril_amd import calibration as CAL
    w, h = shape
    rng = np.random.default_rng(5)
    p = rng.random((h, w)).astype(f32)
    p.ravel()[::7] = 0.0
    p[h // 2, w // 3] = np.nan
    d = _gpu(p)
    regions = [(0, 0, w, h, 1), (w // 3, 0, w - 1, h, 1), (0, 0, w, h, 2), (1, h // 2, w, h, 2)]
    for x0, y0, x1, y1, step in regions:
        n, mean, sigma = CAL.region_stats(d, x0, y0, x1, y1, step, ctx=ctx)
        rn, rmean, rsigma = CR.region_stats(p, x0, y0, x1, y1, step)
        assert n == rn
        _same(np.array([mean, sigma]), np.array([rmean, rsigma]))
    assert CAL.region_stats(_gpu(np.zeros((h, w), f32)), ctx=ctx) == (0, 0.0, 0.0)


@pytest.mark.parametrize("diag", [0, 1])
@pytest.mark.parametrize("shape", [(97, 53), (530, 516), (12, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_s5_equalised_flat_and_norm(ctx, shape, diag):
    from siril_amd import calibration as CAL
    w, h = shape
    rng = np.random.default_rng(9 + diag)
    flat = (0.5 + rng.random((h, w)) * 0.1).astype(f32)
    gains = [1.0, 0.7, 1.3, 1.02] if diag == 0 else [0.7, 1.0, 1.03, 1.4]
    for s in range(4):
        flat[s >> 1::2, s & 1::2] *= f32(gains[s])
    flat.ravel()[::31] = 0.0
    before = flat.copy()
    ref, rdiag, c1, c2 = CR.equalize_cfa(flat)
    assert rdiag == diag
    m = CAL.prepare_masters(flat=flat, cfa=True, equalize_cfa=True, ctx=ctx)
    assert m.equalize[0] == diag
    _same(np.array(m.equalize[1:], f32), np.array([c1, c2], f32))
    _same(m.flat.cpu().numpy(), ref)
    _same(np.array([m.norm], f32), np.array([CR.flat_norm(ref)], f32))
    assert np.array_equal(flat, before)             # the caller's master is never written
    # without the equalisation the norm is the plain flat's mean; a given norm is kept
    m = CAL.prepare_masters(flat=flat, ctx=ctx)
    _same(np.array([m.norm], f32), np.array([CR.flat_norm(flat)], f32))
    assert CAL.prepare_masters(flat=flat, norm=0.25, ctx=ctx).norm == 0.25


def _dark_plane(w, h):
    rng = np.random.default_rng(w + h)
    dark = (rng.gamma(2.0, 200.0, (h, w)) / 65535).astype(f32)
    dark.ravel()[rng.choice(w * h, max(2, w * h // 100), replace=False)] = f32(30000 / 65535)
    dark.ravel()[rng.choice(w * h, max(2, w * h // 200), replace=False)] = 0.0
    return dark


@pytest.mark.parametrize("sig", [(3.0, 3.0), (-1.0, 3.0), (3.0, -1.0), (0.2, 0.2), (-1.0, -0.5)],
                         ids=["3_3", "nocold", "nohot", "dense", "over_half"])
@pytest.mark.parametrize("shape", [(97, 53), (530, 516), (12, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_s6_deviant_list(ctx, shape, sig):
    from siril_amd import calibration as CAL
    w, h = shape
    dark = _dark_plane(w, h)
    ref, rstats = CR.find_deviant(dark, *sig)
    lst, stats = CAL.find_deviant_pixels(_gpu(dark), sig[0], sig[1], ctx=ctx)
    _same(np.array(stats), np.array(rstats))
    got = lst.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    if sig == (-1.0, -0.5):
        assert len(ref) > w * h // 2
    if sig[0] == -1.0:
        assert np.all(ref[:, 1] == CR.HOT)
    if sig == (3.0, 3.0):
        assert len(ref) > 0


# ---------------------------------------------------------------------- S7
def _cc_lists(w, h, step):
    """name -> list of (position, type) in raster order unless said otherwise."""
    C_, H_ = CR.COLD, CR.HOT
    P = lambda x, y: y * w + x
    cx, cy = w // 2, h // 2
    L = {}
    L["isolated"] = [(P(2, 0), H_), (P(w - 3, h // 3), C_), (P(cx, cy), H_)] if h > 2 else [(P(2, 0), H_)]
    L["hot_column"] = [(P(cx, y), H_) for y in range(h)]
    L["cluster"] = [(P(cx + dx * step, cy + dy * step), H_ if (dx + dy) % 2 else C_)
                    for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= cy + dy * step < h]
    L["cold_then_hot"] = [(P(3, cy), C_), (P(3 + 2 * step, cy), H_)]
    L["borders"] = sorted({(P(0, 0), C_), (P(w - 1, 0), H_), (P(0, h - 1), H_), (P(w - 1, h - 1), C_),
                           (P(cx, 0), C_), (P(cx, h - 1), C_), (P(0, cy), C_), (P(w - 1, cy), C_),
                           (P(cx + 3, 0), H_), (P(w - 1, cy + (1 if h > 2 else 0)), H_)}, key=lambda e: e[0])
    L["borders"] = list({p: t for p, t in L["borders"]}.items())
    L["empty"] = []
    # any list: not in raster order, a position listed twice with both types
    L["unordered_dup"] = L["cluster"][::-1] + [(P(cx, cy), H_), (P(cx, cy), C_)] + L["cold_then_hot"][::-1]
    every = {}
    for k in ("hot_column", "cluster", "cold_then_hot", "borders", "isolated"):
        for p, t in L[k]:
            every.setdefault(p, t)
    L["all"] = sorted(every.items())
    return L


CC_NAMES = ["isolated", "hot_column", "cluster", "cold_then_hot", "borders", "empty", "unordered_dup", "all"]


@pytest.mark.parametrize("name", CC_NAMES)
@pytest.mark.parametrize("cfa", [False, True], ids=["mono", "cfa"])
@pytest.mark.parametrize("shape", [(97, 53), (12, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_s7_cosmetic_correction(ctx, oracle, shape, cfa, name):
    from siril_amd import calibration as CAL
    w, h = shape
    lst = np.array(_cc_lists(w, h, 2 if cfa else 1)[name], np.int32).reshape(-1, 2)
    rng = np.random.default_rng(21)
    frames = rng.random((3, h, w)).astype(f32)
    if len(lst):
        frames[:, lst[:, 0] // w, lst[:, 0] % w] += f32(3.0)
        frames[1, lst[0, 0] // w, lst[0, 0] % w] = np.nan
    want = np.stack([CR.cosmetic(fr, lst, cfa) for fr in frames])
    d = _gpu(frames)
    CAL.cosmetic_correction(d, _gpu(lst) if len(lst) else None, cfa, ctx=ctx)
    _same(d.cpu().numpy(), want)


def test_s7_plan_follows_the_list(ctx, oracle):
    """The launch plan kept in the context is rebuilt when the list's content
    changes at the same address and size."""
    from siril_amd import calibration as CAL
    w, h = 97, 53
    frames = np.random.default_rng(2).random((3, h, w)).astype(f32)
    a = np.array([(5 * w + 5, CR.HOT), (5 * w + 6, CR.COLD)], np.int32)
    b = np.array([(9 * w + 40, CR.COLD), (9 * w + 41, CR.COLD)], np.int32)
    d_list = _gpu(a)
    for lst in (a, b, a):
        d_list.copy_(_gpu(lst))
        d = _gpu(frames)
        CAL.cosmetic_correction(d, d_list, False, ctx=ctx)
        _same(d.cpu().numpy(), np.stack([CR.cosmetic(fr, lst) for fr in frames]))


# -------------------------------------------------------------- whole path
def _full_case(n=3, w=97, h=53):
    frames, dark = CR.synth_optim_case(w, h, k_true=(0.6, 1.0, 1.45, 0.8, 1.2)[:n], seed=8)
    rng = np.random.default_rng(4)
    flat = (20000 + rng.random((h, w)) * 4000)
    for s, g in enumerate((1.0, 0.6, 1.5, 1.01)):
        flat[s >> 1::2, s & 1::2] *= g
    flat16 = np.rint(flat).astype(np.uint16)
    dark16 = np.rint(dark * 65535).astype(np.uint16)
    assert np.array_equal(CR.to_float(dark16), dark)
    return frames, dark16, flat16


def _full_ref(frames, dark16, flat16, level):
    dark, flat = CR.to_float(dark16), CR.to_float(flat16)
    eq = CR.equalize_cfa(flat)[0]
    lst = CR.find_deviant(dark, 3.0, 3.0)[0]
    assert len(lst) > 0
    return CR.calibrate(frames, level=level, dark=dark, flat=eq, norm=CR.flat_norm(eq), dark_optim=True,
                        deviant=lst, cfa=True)


def test_whole_path(ctx, oracle):
    from siril_amd import calibration as CAL
    frames, dark16, flat16 = _full_case()
    level = f32(1900) * CR.INV
    want, k_ref = _full_ref(frames, dark16, flat16, level)
    m = CAL.prepare_masters(bias=float(level), dark=dark16, flat=flat16, cfa=True, equalize_cfa=True,
                            cc_sigma=(3.0, 3.0), ctx=ctx)
    out, k = CAL.calibrate(_gpu(frames), m, dark_optim=True, ctx=ctx)
    _same(k, k_ref)
    _same(out.cpu().numpy(), want)


def test_calibrate_command(oracle, tmp_path):
    from siril_amd import cli
    from siril_amd.sequence import frame_name, read_fits, stack_frames, write_fits, write_seq
    frames, dark16, flat16 = _full_case(n=5)
    d = str(tmp_path)
    for i, fr in enumerate(frames):
        write_fits(os.path.join(d, frame_name("light_", i + 1)), fr)
    write_seq(os.path.join(d, "light_.seq"), "light_", 5)
    write_fits(os.path.join(d, "dark_stacked.fit"), dark16)
    write_fits(os.path.join(d, "pp_flat_stacked.fit"), flat16)
    assert cli.main(["calibrate", os.path.join(d, "light_"), '-bias="=1900"', "-dark=dark_stacked",
                     "-flat=pp_flat_stacked", "-cc=dark", "3", "3", "-cfa", "-equalize_cfa", "-opt"]) == 0
    want, _ = _full_ref(frames, dark16, flat16, f32(1900) * CR.INV)
    for i in range(5):
        got = read_fits(os.path.join(d, frame_name("pp_light_", i + 1)))
        _same(got, want[i])
    idx, ref = stack_frames(os.path.join(d, "pp_light_.seq"))
    assert idx == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------- refusals
def test_refusals(ctx):
    import ctypes as C
    import torch
    from siril_amd import SgpuError, calibration as CAL
    from siril_amd._lib import lib
    w, h = 97, 53
    frames, bias, dark, flat = _case(w, h, np.uint16)
    m = _masters(ctx, dark=dark, flat=flat)
    d = _gpu(frames)
    out = torch.empty((3, h, w), dtype=torch.float32, device="cuda")

    def refused(fn):
        with pytest.raises(SgpuError) as e:
            fn()
        assert e.value.code == BAD_ARGUMENT
        assert "failed (-21): " in str(e.value) and len(str(e.value).split(": ", 1)[1]) > 0

    for es in (1, 3, 8):
        refused(lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), es, 3, w, h, w * h, m))
    refused(lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), 2, 3, w, h, w * h - 1, m))
    # WORD input aliased by the float output
    big = torch.zeros(3 * h * w, dtype=torch.float32, device="cuda")
    refused(lambda: CAL.calibrate_device(ctx, big.data_ptr(), big.data_ptr(), 2, 3, w, h, w * h, m))
    refused(lambda: CAL.calibrate_device(ctx, big.data_ptr() + 64, big.data_ptr(), 2, 2, w, h, w * h, m))
    nodark = _masters(ctx, flat=flat)
    refused(lambda: CAL.calibrate(d, nodark, dark_optim=True, ctx=ctx))
    refused(lambda: CAL.dark_optimize(d, nodark, ctx=ctx))
    nodark.deviant = _gpu(np.array([(5, CR.HOT)], np.int32))
    refused(lambda: CAL.calibrate(d, nodark, ctx=ctx))
    refused(lambda: CAL.prepare_masters(flat=flat, cc_sigma=(3.0, 3.0), ctx=ctx))
    refused(lambda: CAL.prepare_masters(flat=flat, equalize_cfa=True, cfa_pattern_size=6, ctx=ctx))
    # a list entry outside the frame is refused, not applied
    bad = _gpu(np.array([(w * h, CR.HOT)], np.int32))
    refused(lambda: CAL.cosmetic_correction(out, bad, False, ctx=ctx))
    assert lib().sgpu_last_error()

"""The Richardson-Lucy kernels taken alone (rl_conv.hip, rl_fft.hip and their
host side in sgpu_rl.cpp) through sgpu_rl_conv_device / sgpu_rl_reg_device,
against the plain references of tests/rl_conv_ref.py and oracle/rl_ref.py.

The main inputs are small integers (image in [-8, 8], taps in [-4, 4]): every
partial sum stays below 2^24, so the true convolution is an integer that
float32 holds exactly in any summation order, and a missed, doubled or
misplaced tap moves it by at least 1.
  (a) direct kernel: bit-exact at the taps-padding, row-band, LDS-threshold
      and tile-seam sizes, and at images smaller than the tile's reach
  (b) FFT convolution: rounds to the exact integers, and errs by at most 8x
      what the single-precision scipy restatement of the same transform errs
  (c) spectrum chain: bit-identical to standalone calls, also on slices
      shorter than the PSF (H < 2 h)
  (d) the eight epilogues, the sanitising branches, the stop measure
  (e) the regulariser weights at non-square sizes
  (f) slice plumbing: an identity deconvolution over many slices
tests/test_rl_conv_ref.py checks the references themselves without a GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rl_conv_ref as RC  # noqa: E402

from oracle import rl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -21
_ref_cache = {}
_ratios = {}


@pytest.fixture(scope="module")
def D():
    from siril_amd import deconvolution
    return deconvolution


@pytest.fixture(scope="module")
def ctx():
    from siril_amd.stacking import Context
    c = Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _conv(D, ctx, x, k, path=0, wrap=1, epi=0, want_stop=False, chain=-1, **ops):
    """One call on host arrays; the output starts as NaN, so a pixel the
    kernel does not write cannot pass.  Returns out (and the stop measure)."""
    import torch
    dx = _dev(x)
    out = torch.full(dx.shape, float("nan"), dtype=torch.float32, device=dx.device)
    dev = {n: (_dev(v) if isinstance(v, np.ndarray) else v) for n, v in ops.items()}
    stop = D.rl_conv_device(dx, np.asarray(k, np.float32), out, path=path, wrap=wrap, epi=epi, want_stop=want_stop,
                            chain=chain, ctx=ctx, **dev)
    o = out.cpu().numpy()
    return (o, stop) if want_stop else o


def _exact(H, W, ks, wrap, seed=0):
    key = (H, W, ks, wrap, seed)
    if key not in _ref_cache:
        x, k = RC.int_image(H, W, seed), RC.int_taps(ks, seed)
        _ref_cache[key] = (x, k, RC.conv_exact(x, k, wrap))
    return _ref_cache[key]


def _float_case(wrap):
    key = ("float", wrap)
    if key not in _ref_cache:
        H, W, ks = RC.FLOAT_CASE
        x, k = RC.float_image(H, W), RC.moffat_taps(ks)
        _ref_cache[key] = (x, k, RC.conv_exact(x, k, wrap), RC.conv_exact(np.abs(x), np.abs(k), wrap))
    return _ref_cache[key]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def _refused(D, ctx, *a, **kw):
    from siril_amd._lib import SgpuError
    with pytest.raises(SgpuError) as e:
        _conv(D, ctx, *a, **kw)
    assert e.value.code == BAD_ARGUMENT
    return True


# ------------------------------------------------------------ (a) direct path
def _direct_shapes(ks, wrap):
    hk = ks // 2
    shapes = [(hk + 1, hk + 1), (63, 65), (64, 64), (65, 129), (130, 67)]
    if not wrap:
        shapes += [(1, 1), (5, 200)]
    return shapes


def _check_direct(D, ctx, ks, wrap):
    hk = ks // 2
    for H, W in _direct_shapes(ks, wrap):
        x, k, want = _exact(H, W, ks, wrap)
        if wrap and min(H, W) < hk + 1:
            assert _refused(D, ctx, x, k, path=0, wrap=wrap)
            continue
        got = _conv(D, ctx, x, k, path=0, wrap=wrap)
        bad = np.argwhere(got != want.astype(np.float32))
        assert bad.size == 0, f"ks={ks} wrap={wrap} {H}x{W}: {len(bad)} pixels differ, first (y, x) = {bad[0]}"


# 1, 3: one chunk of taps columns; 15 / 17 and 31 / 33, 49 / 51, 63: either side
# of the 16-column taps padding; 17 is the first size with unmasked row bands;
# the dynamic LDS passes 64 KiB between 49 and 51.  The largest size runs last
# and a small one after it (the kernel's LDS attribute only ever grows).
@pytest.mark.parametrize("ks", [1, 3, 15, 17, 31, 33, 49, 51, 63, "max"])
def test_direct_store_bit_exact(D, ctx, ks):
    if ks == "max":
        ks = D.max_conv_ks()
        assert ks == 101
    for wrap in (0, 1):
        _check_direct(D, ctx, ks, wrap)


def test_direct_small_kernel_after_the_largest(D, ctx):
    for ks in (3, 17):
        for wrap in (0, 1):
            _check_direct(D, ctx, ks, wrap)


@pytest.mark.parametrize("wrap", [0, 1])
def test_direct_float_within_summation_bound(D, ctx, wrap):
    """|got - exact| <= ks^2 * 2^-24 * (|x| * |k|) pointwise: the worst case
    of any summation order of ks^2 rounded float32 products (each of the at
    most ks^2 roundings is relative 2^-24 of a partial sum that |x| * |k|
    bounds)."""
    x, k, want, mag = _float_case(wrap)
    ks = k.shape[0]
    got = _conv(D, ctx, x, k, path=0, wrap=wrap).astype(np.float64)
    bound = ks * ks * 2.0 ** -24 * mag
    excess = np.abs(got - want) - bound
    print(f"direct float wrap={wrap}: max err {np.abs(got - want).max():.3e}, min bound {bound.min():.3e}")
    assert excess.max() <= 0


def test_direct_domain_is_checked(D, ctx):
    import torch
    from siril_amd._lib import SgpuError
    x = RC.int_image(20, 20)
    assert _refused(D, ctx, x, np.ones((4, 4)), path=0)                       # even
    assert _refused(D, ctx, x, np.ones((103, 103)), path=0, wrap=0)           # > max_conv_ks
    assert _refused(D, ctx, x, RC.int_taps(3), path=0, epi=RC.EPI_RATIO)      # f missing
    assert _refused(D, ctx, x, RC.int_taps(3), path=0, epi=RC.EPI_MULT_REG, est=x.astype(np.float32))   # w missing
    assert _refused(D, ctx, x, RC.int_taps(3), path=0, epi=RC.EPI_TAPER, wy=np.ones(20, np.float32))    # wx missing
    assert _refused(D, ctx, x, RC.int_taps(3), path=0, chain=0)               # no chain on the direct path
    assert _refused(D, ctx, x[:3], RC.int_taps(7), path=0, wrap=1)            # H < hk + 1
    assert _refused(D, ctx, x, RC.int_taps(3), path=1, wrap=0)                # the FFT path is circular
    dx = _dev(x)
    with pytest.raises(SgpuError):                                            # out aliases in
        D.rl_conv_device(dx, RC.int_taps(3).astype(np.float32), dx, ctx=ctx)
    with pytest.raises(SgpuError):                                            # overlapping views
        buf = torch.zeros(21 * 20, dtype=torch.float32, device="cuda")
        D.rl_conv_device(buf[:400].view(20, 20), RC.int_taps(3).astype(np.float32), buf[20:].view(20, 20), ctx=ctx)


# -------------------------------------------------------------- (b) FFT path
def _check_fft(got, x, k, want, label):
    """np.rint(got) == exact everywhere (a condition: a structural error is at
    least 1), and max|got - exact| <= 8 x max|conv_f32_fft - exact|, the right
    side from the reference alone.  8 is three bits of room: the kernels
    transform in float32 at the same lengths as the reference, with float
    twiddle tables and radix-8 butterflies."""
    ref = RC.conv_f32_fft(x, k)
    e_ref = float(np.abs(ref.astype(np.float64) - want).max())
    e_gpu = float(np.abs(got.astype(np.float64) - want).max())
    ratio = e_gpu / e_ref if e_ref > 0 else (0.0 if e_gpu == 0 else float("inf"))
    _ratios[label] = ratio
    print(f"RLFFT {label}: gpu {e_gpu:.3e} ref {e_ref:.3e} ratio {ratio:.2f} max|c| {np.abs(want).max():.6g}")
    if np.issubdtype(np.asarray(want).dtype, np.integer):
        bad = np.argwhere(np.rint(got).astype(np.int64) != want)
        assert bad.size == 0, f"{label}: {len(bad)} pixels round to another integer, first (y, x) = {bad[0]}"
    assert e_gpu <= 8 * e_ref, f"{label}: GPU error {e_gpu:.3e} > 8 x reference error {e_ref:.3e}"
    return e_ref


@pytest.mark.parametrize("H,W,ks", RC.FFT_CASES)
def test_fft_store(D, ctx, H, W, ks):
    x, k, want = _exact(H, W, ks, 1)
    assert D.fft_smooth_len(W + 3 * (ks // 2)) == RC.fft_smooth_len(W + 3 * (ks // 2))
    assert D.fft_smooth_len(H + 3 * (ks // 2)) == RC.fft_smooth_len(H + 3 * (ks // 2))
    got = _conv(D, ctx, x, k, path=1)
    _check_fft(got, x, k, want, f"{H}x{W} ks={ks}")


def test_fft_float_case(D, ctx):
    x, k, want, _ = _float_case(1)
    got = _conv(D, ctx, x, k, path=1)
    _check_fft(got, x, k, want, "float %dx%d ks=%d" % RC.FLOAT_CASE)


def test_fft_too_long_is_refused(D, ctx):
    """W + 3h > 8192 (or H): no FFT length, refused without a launch."""
    assert D.fft_smooth_len(8193) == 0
    assert _refused(D, ctx, np.zeros((13, 8190)), RC.int_taps(3), path=1)
    assert _refused(D, ctx, np.zeros((8190, 13)), RC.int_taps(3), path=1)


def test_fft_column_major_plane_subprocess():
    """SGPU_RL_TRANSPOSE=0 (the row kernels store and load the column-major
    plane themselves): the (65, 200) ks = 63 case under the same two rules."""
    import subprocess
    code = (
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import test_rl_conv_gpu as T\n"
        "from siril_amd import deconvolution as D\n"
        "from siril_amd.stacking import Context\n"
        "ctx = Context(0)\n"
        "x, k, want = T._exact(65, 200, 63, 1)\n"
        "T._check_fft(T._conv(D, ctx, x, k, path=1), x, k, want, '65x200 ks=63 column-major')\n"
        "x, k, want = T._exact(200, 65, 63, 1)\n"
        "T._check_fft(T._conv(D, ctx, x, k, path=1), x, k, want, '200x65 ks=63 column-major')\n"
        "print('DONE')\n")
    env = dict(os.environ, SGPU_RL_TRANSPOSE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DONE" in r.stdout


# ----------------------------------------------------------------- (c) chain
# The issue's four shapes, then four with h and H even.  H < 2h at (59, 90, 63),
# (44, 90, 61) and (20, 70, 29): rows H - h <= y < h of the periodic extension
# need a wrap copy on both sides.  (59, 90) at ks = 63 is the thin second slice
# of the 6000 x 4000 configuration, narrowed.
CHAIN_CASES = [(59, 90, 63), (31, 70, 31), (64, 64, 15), (33, 40, 15),
               (44, 90, 61), (20, 70, 29), (64, 64, 13), (34, 40, 13)]
CHAIN_SCALE = np.float32(2.0 ** -8)                  # keeps the third result's magnitude moderate


def _chain_run(D, ctx, H, W, ks):
    """Three convolutions in a row, standalone (y1s, y2s, y3s) and chained:
    call 1 leaves its output's spectrum (chain = 2) and call 2 consumes it
    (chain = 1) -> y2; then 2 -> 3 -> 1, so that the fused kernel's own output
    spectrum is consumed too -> y2b, y3."""
    key = ("chain", H, W, ks)
    if key not in _ref_cache:
        x0 = RC.int_image(H, W, 1)
        k1 = RC.int_taps(ks, 1).astype(np.float32)
        k2, k3 = RC.int_taps(ks, 2) * CHAIN_SCALE, RC.int_taps(ks, 3) * CHAIN_SCALE
        r = dict(x0=x0, k1=k1, k2=k2, k3=k3)
        r["y1s"] = _conv(D, ctx, x0, k1, path=1)
        r["y2s"] = _conv(D, ctx, r["y1s"], k2, path=1)
        r["y3s"] = _conv(D, ctx, r["y2s"], k3, path=1)
        r["y1"] = _conv(D, ctx, x0, k1, path=1, chain=2)
        r["y2"] = _conv(D, ctx, r["y1"], k2, path=1, chain=1)
        _conv(D, ctx, x0, k1, path=1, chain=2)
        r["y2b"] = _conv(D, ctx, r["y1"], k2, path=1, chain=3)
        r["y3"] = _conv(D, ctx, r["y2b"], k3, path=1, chain=1)
        _ref_cache[key] = r
    return _ref_cache[key]


@pytest.mark.parametrize("H,W,ks", CHAIN_CASES + [(20, 70, 31)])
def test_chain_within_fft_error(D, ctx, H, W, ks):
    """Every parity of h and H: the chained result and the standalone one are
    both the convolution of the same float32 image (call 1's output is
    bit-identical either way: the inverse row pass pairs the same rows), so
    each lies within 8 x (reference error) of the exact result by the rule of
    (b), and they lie within 16 x of each other.  A wrap copy that is missing
    from the periodic extension moves rows by O(max|c|)."""
    r = _chain_run(D, ctx, H, W, ks)
    assert _bits_equal(r["y1"], r["y1s"])
    assert np.array_equal(np.rint(r["y1s"]).astype(np.int64), RC.conv_exact(r["x0"], r["k1"].astype(np.int64), 1))
    for name, src, k, got, alone in (("call 2", r["y1s"], r["k2"], r["y2"], r["y2s"]),
                                     ("call 2 (chain 3)", r["y1s"], r["k2"], r["y2b"], r["y2s"]),
                                     ("call 3", r["y2b"], r["k3"], r["y3"], None)):
        exact = RC.conv_exact(src.astype(np.float64), k.astype(np.float64), 1)
        e_ref = float(np.abs(RC.conv_f32_fft(src, k).astype(np.float64) - exact).max())
        e_gpu = float(np.abs(got.astype(np.float64) - exact).max())
        d = 0.0 if alone is None else float(np.abs(got.astype(np.float64) - alone).max())
        print(f"chain {H}x{W} ks={ks} {name}: gpu {e_gpu:.3e} ref {e_ref:.3e} chained-standalone {d:.3e} "
              f"max|c| {np.abs(exact).max():.6g}")
        assert e_gpu <= 8 * e_ref
        assert d <= 16 * e_ref


@pytest.mark.parametrize("H,W,ks", CHAIN_CASES)
def test_chain_bit_identical(D, ctx, H, W, ks):
    """A call that consumes the spectrum its predecessor left computes the
    bits of the same call run standalone.  The row passes pack two real rows
    into one complex transform, and a row's separated spectrum depends in its
    last bits on its partner: the fused inverse + forward kernel
    (k_rlf_rows_inv_fwd) pairs image rows 2j, 2j + 1, the standalone forward
    pass rows 2j, 2j + 1 of the periodic extension, image rows 2j - h,
    2j + 1 - h.  fft_conv_chain therefore fuses only where h = ks/2 and H are
    even (the last four shapes, where the fused kernel's wrap copies are under
    test) and leaves the spectrum through the plain inverse and forward passes
    elsewhere (the issue's four shapes, h = 31, 15, 7, 7); with the fused
    kernel at those, 4587 of 5310, 1831 of 2170, 3541 of 4096 and 1119 of 1320
    pixels of call 2 differed from the standalone call by rounding."""
    r = _chain_run(D, ctx, H, W, ks)
    assert _bits_equal(r["y1"], r["y1s"])
    assert _bits_equal(r["y2"], r["y2s"]), f"call 2: {int((r['y2'] != r['y2s']).sum())} of {H * W} pixels differ"
    assert _bits_equal(r["y2b"], r["y2s"])
    # y3s continues from y2s, y3 from y2b: the same bits when the line above holds
    assert _bits_equal(r["y3"], r["y3s"]), f"call 3: {int((r['y3'] != r['y3s']).sum())} of {H * W} pixels differ"


def test_chain_without_a_spectrum_is_refused(D, ctx):
    x, k = RC.int_image(33, 40), RC.int_taps(15)
    _conv(D, ctx, x, k, path=1)                                   # standalone: leaves nothing
    assert _refused(D, ctx, x, k, path=1, chain=1)
    _conv(D, ctx, x, k, path=1, chain=2)
    assert _refused(D, ctx, RC.int_image(33, 42), k, path=1, chain=1)        # another geometry
    _conv(D, ctx, x, k, path=1, chain=2)
    assert _refused(D, ctx, x, RC.int_taps(13), path=1, chain=1)             # another PSF size
    _conv(D, ctx, x, k, path=1, chain=2)
    _conv(D, ctx, x, k, path=0)                                              # any call in between spends it
    assert _refused(D, ctx, x, k, path=1, chain=1)
    _conv(D, ctx, x, k, path=1, chain=2)
    _conv(D, ctx, x, k, path=1, chain=1)
    assert _refused(D, ctx, x, k, path=1, chain=1)                           # chain = 1 leaves none


# ------------------------------------------------------------- (d) epilogues
EH, EW, EKS = 37, 70, 5
DT, RLAM = 0.3, 0.37


def _epi_operands():
    key = "epi"
    if key not in _ref_cache:
        rng = np.random.default_rng(41)
        x, k, c = _exact(EH, EW, EKS, 1, seed=4)
        _ref_cache[key] = dict(
            x=x.astype(np.float32), k=k, c=c.astype(np.float32),
            f=rng.uniform(0.5, 2.0, (EH, EW)).astype(np.float32),
            est=rng.uniform(0.5, 2.0, (EH, EW)).astype(np.float32),
            w=rng.uniform(-1.0, 1.0, (EH, EW)).astype(np.float32),
            ref=rng.uniform(0.5, 2.0, (EH, EW)).astype(np.float32),
            wy=rng.uniform(0.0, 1.0, EH).astype(np.float32),        # no symmetry: an ox / oy swap shows
            wx=rng.uniform(0.0, 1.0, EW).astype(np.float32))
    return _ref_cache[key]


def _epi_kwargs(o, epi):
    if epi in (RC.EPI_RATIO, RC.EPI_RATIO_NAIVE):
        return dict(f=o["f"])
    if epi in (RC.EPI_MULT, RC.EPI_GRAD):
        return dict(est=o["est"], dt=DT)
    if epi in (RC.EPI_MULT_REG, RC.EPI_GRAD_REG):
        return dict(est=o["est"], w=o["w"], dt=DT, rlam=RLAM)
    if epi == RC.EPI_TAPER:
        return dict(wy=o["wy"], wx=o["wx"])
    return {}


# ulps allowed: the library is built without contraction, so every epilogue
# is the float32 (EPI_TAPER: double) expression as written.  The three with a
# division were allowed its last bit and measured bit-equal on an MI355X (the
# device's float division is correctly rounded), so all eight are held to 0.
EPI_ULPS = {epi: 0 for epi in range(8)}


@pytest.mark.parametrize("epi", list(range(8)))
def test_epilogue_direct(D, ctx, epi):
    o = _epi_operands()
    assert (o["c"] == 0).any() and (o["c"] < 0).any()        # the sanitising branches are taken
    kw = _epi_kwargs(o, epi)
    got = _conv(D, ctx, o["x"], o["k"], path=0, wrap=1, epi=epi, **kw)
    want = RC.epilogue(epi, o["c"], x=o["x"], **kw)
    assert not np.isnan(got).any() and np.array_equal(np.isinf(got), np.isinf(want))
    ulps = RC.ulp_diff(got, want)
    print(f"epilogue {epi}: {ulps} ulp")
    assert ulps <= EPI_ULPS[epi]


def test_epilogue_sanitising_on_zero_input(D, ctx):
    """c == 0 everywhere: EPI_RATIO gives f / 1e-9f, EPI_RATIO_NAIVE
    max(1e-9, f / 0) (inf for f > 0, 1e-9 for f <= 0: -inf and the NaN of 0 / 0
    both fail the comparison)."""
    o = _epi_operands()
    f = o["f"].copy()
    f[0, :5] = 0.0
    f[1, :5] = -1.5
    z = np.zeros((EH, EW), np.float32)
    nine = np.float32(1e-9)
    got = _conv(D, ctx, z, o["k"], path=0, wrap=1, epi=RC.EPI_RATIO, f=f)
    assert _bits_equal(got, (f / nine).astype(np.float32))
    got = _conv(D, ctx, z, o["k"], path=0, wrap=0, epi=RC.EPI_RATIO_NAIVE, f=f)
    want = np.where(f > 0, np.float32(np.inf), nine).astype(np.float32)
    assert _bits_equal(got, want)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("epi", [RC.EPI_MULT, RC.EPI_GRAD_REG])
@pytest.mark.parametrize("with_ref", [False, True])
def test_stop_measure(D, ctx, path, epi, with_ref):
    """stop_out == sum |out - ref| / |ref| with the terms formed in float32
    from the GPU's own output and summed in float64, to 1e-9 relative: the
    terms are non-negative, so another order of at most 1e5 doubles moves the
    sum by less than 1e-11."""
    o = _epi_operands()
    kw = _epi_kwargs(o, epi)
    if with_ref:
        kw["stop_ref"] = o["ref"]
    got, stop = _conv(D, ctx, o["x"], o["k"], path=path, wrap=1, epi=epi, want_stop=True, **kw)
    want = RC.stop_measure(got, o["ref"] if with_ref else o["est"])
    print(f"stop path={path} epi={epi} ref={with_ref}: {stop!r} vs {want!r}")
    assert want > 0 and abs(stop - want) <= 1e-9 * want
    # an epilogue without a stop measure reports 0
    _, none = _conv(D, ctx, o["x"], o["k"], path=path, wrap=1, epi=RC.EPI_STORE, want_stop=True)
    assert none == 0.0


def test_epilogue_fft_taper_and_ratio(D, ctx):
    """The FFT path's c carries the error d <= 8 x (reference error) of (b);
    through the formulas: EPI_TAPER moves by (1 - w) d, EPI_RATIO (where the
    exact c is a non-zero integer) by |f| d / (|c| (|c| - d)), plus one
    rounding of the result each."""
    o = _epi_operands()
    c = o["c"].astype(np.float64)
    d = 8 * float(np.abs(RC.conv_f32_fft(o["x"], o["k"]).astype(np.float64) - c).max())
    assert 0 < d < 0.01
    ulp = 2.0 ** -23
    got = _conv(D, ctx, o["x"], o["k"], path=1, epi=RC.EPI_TAPER, wy=o["wy"], wx=o["wx"]).astype(np.float64)
    want = RC.epilogue(RC.EPI_TAPER, o["c"], x=o["x"], wy=o["wy"], wx=o["wx"]).astype(np.float64)
    w = o["wy"].astype(np.float64)[:, None] * o["wx"].astype(np.float64)[None, :]
    assert (np.abs(got - want) <= (1 - w) * d + ulp * np.abs(want)).all()
    got = _conv(D, ctx, o["x"], o["k"], path=1, epi=RC.EPI_RATIO, f=o["f"]).astype(np.float64)
    nz = c != 0
    want = o["f"].astype(np.float64)[nz] / c[nz]
    tol = o["f"].astype(np.float64)[nz] * d / (np.abs(c[nz]) * (np.abs(c[nz]) - d)) + ulp * np.abs(want)
    assert (np.abs(got[nz] - want) <= tol).all()


# ----------------------------------------------------- (e) regulariser weights
def _flat_rows_image(H, W):
    """Constant rows in runs of equal rows: |grad| = 0 inside a run (the
    epsilon and the sanitize branches), a pure vertical step between runs."""
    vals = np.array([3, 3, 3, -2, -2, 5, 0, 0, 0, 0, -7, 4], np.float32)
    return np.repeat(vals[np.arange(H) % len(vals)][:, None], W, axis=1)


REG_SIZES = [(2, 2), (2, 7), (3, 64), (63, 65), (65, 3), (130, 67)]


def _reg(D, ctx, e, mode):
    import torch
    de = _dev(e)
    w = torch.full(de.shape, float("nan"), dtype=torch.float32, device=de.device)
    g = torch.full(de.shape, float("nan"), dtype=torch.float32, device=de.device)
    D.rl_reg_device(de, w, g if mode == D.REG_W_NAIVE_FH else None, mode=mode, ctx=ctx)
    return w.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("H,W", REG_SIZES)
@pytest.mark.parametrize("flat", [False, True])
def test_regulariser_weights(D, ctx, H, W, flat):
    """FH modes and gxy: every intermediate is an exact integer, so the
    weights can differ in the square root's last bit at most; measured
    bit-equal on an MI355X and held to that.  TV modes, 4e-6
    absolute: four unit-vector terms of magnitude <= 1, each off by at most
    2 ulp of 1 from a hypot that may differ in its last bit, and three
    additions at magnitude <= 4: below 1.7e-6 together, while an indexing
    error is O(0.1 - 1)."""
    e = _flat_rows_image(H, W) if flat else RC.int_image(H, W, 9).astype(np.float32)
    for mode, ref in ((D.REG_W_FFT_TV, R.reg_fft_tv), (D.REG_W_NAIVE_TV, R.reg_naive_tv)):
        got, _ = _reg(D, ctx, e, mode)
        err = np.abs(got.astype(np.float64) - ref(e)).max()
        print(f"reg mode {mode} {H}x{W} flat={flat}: max err {err:.3e}")
        assert not np.isnan(got).any() and err <= 4e-6
    got, _ = _reg(D, ctx, e, D.REG_W_FFT_FH)
    u1 = RC.ulp_diff(got, R.reg_fft_fh(e))
    got, gxy = _reg(D, ctx, e, D.REG_W_NAIVE_FH)
    want, want_gxy = R.reg_naive_fh(e)
    u3 = RC.ulp_diff(got, want)
    print(f"reg FH {H}x{W} flat={flat}: {u1} / {u3} ulp")
    assert u1 == 0 and u3 == 0
    assert _bits_equal(gxy, want_gxy)


def test_regulariser_domain_is_checked(D, ctx):
    import torch
    from siril_amd._lib import SgpuError
    e = _dev(np.zeros((1, 8), np.float32))
    with pytest.raises(SgpuError):
        D.rl_reg_device(e, torch.empty_like(e), mode=0, ctx=ctx)             # H < 2
    e = _dev(np.zeros((4, 4), np.float32))
    with pytest.raises(SgpuError):
        D.rl_reg_device(e, torch.empty_like(e), mode=4, ctx=ctx)
    with pytest.raises(SgpuError):
        D.rl_reg_device(e, e, mode=0, ctx=ctx)


# ---------------------------------------------------------- (f) slice plumbing
def _white(H, W, seed):
    img = np.random.default_rng([H, W, seed]).random((H, W), dtype=np.float32)
    img[H // 3, W // 2] = 1.0                      # max exactly 1: no scaling
    assert img.max() == 1.0
    return img


def _delta(ks):
    k = np.zeros((ks, ks), np.float32)
    k[ks // 2, ks // 2] = 1.0
    return k


@pytest.mark.parametrize("H,W", [(97, 131), (150, 61)])
@pytest.mark.parametrize("ks", [3, 15])
def test_identity_over_many_slices_fft(D, H, W, ks):
    """maxiter = 0 with a delta PSF: padding, slice extraction, three edge
    tapers of an identity convolution, slice store, unpadding.  Output ==
    input to 1e-5 of the maximum: each taper is within the ~3e-7
    single-precision FFT error (tests/test_rl_conv_ref.py), a tenfold margin
    on three of them; a misplaced or reflected pixel of white noise is O(0.3)."""
    from siril_amd.stacking import Context
    hk = ks // 2
    side = 60 if ks == 15 else 40
    mem = 10 * side * side * 4
    nsl = len(R.slices(W + 2 * hk, H + 2 * hk, mem, hk, 10))
    assert nsl >= 6
    img = _white(H, W, ks)
    c = Context(0)
    D.set_memory_budget(mem, c)
    got = img.copy()
    assert D.fft_richardson_lucy(got, _delta(ks), maxiter=0, regtype=R.REG_NONE_MULT, ctx=c) == 0
    from siril_amd._lib import lib
    assert lib().sgpu_rl_last_fft_convs(c.h) == 3 * nsl
    c.close()
    err = float(np.abs(got.astype(np.float64) - img).max())
    print(f"identity fft {H}x{W} ks={ks}: {nsl} slices, max err {err:.3e}")
    assert err <= 1e-5 * img.max()


@pytest.mark.parametrize("H,W,side", [(9, 9, None), (9, 9, 8), (40, 33, 8)])
def test_identity_over_slices_naive(D, H, W, side):
    """The same through naive_richardson_lucy at ks = 3 (padding 2 ks, the
    edge tapers on the direct kernel with wrap = 1), to 4 ulp: the direct
    identity is exact and each of the three tapers rounds once.  The 9 x 9
    image makes 21-pixel slices, smaller than the tile's reach; the small
    budget cuts slices down to 2 pixels."""
    from siril_amd.stacking import Context
    ks = 3
    mem = R.AMPLE_MEMORY if side is None else 7 * (side + 2) * (side + 2) * 4
    nsl = len(R.slices(W + 4 * ks, H + 4 * ks, mem, 1, 7))
    assert side is None or nsl >= 6
    img = _white(H, W, 3)
    c = Context(0)
    D.set_memory_budget(mem, c)
    got = img.copy()
    assert D.naive_richardson_lucy(got, _delta(ks), maxiter=0, regtype=R.REG_NONE_MULT, ctx=c) == 0
    from siril_amd._lib import lib
    assert lib().sgpu_rl_last_conv_launches(c.h) == 3 * nsl
    c.close()
    ulps = RC.ulp_diff(got, img)
    print(f"identity naive {H}x{W}: {nsl} slices, {ulps} ulp")
    assert ulps <= 4


def test_report_fft_error_ratios():
    """The largest GPU / reference error ratio of the FFT cases above."""
    if _ratios:
        worst = max(_ratios, key=_ratios.get)
        print(f"RLFFT worst ratio {_ratios[worst]:.2f} at {worst} over {len(_ratios)} cases")

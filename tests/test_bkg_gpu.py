"""The background-extraction kernels (siril_amd/csrc/background.hip) against
the restatement (tests/bkg_ref.py), stage by stage, float32 and WORD: box
medians and selection bit for bit, the fit within 100 x the restatement's own
rounding floor, the streaming pass bit for bit from the coefficients the GPU
returned, the whole within one float32 ulp; the vector tail, the scalar form,
the statuses and the empty call.  tests/test_bkg.py pins, without a GPU, that
no case here is a degenerate fit or a selection on the knife's edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402
import bkg_scenes as BS  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_IDS = list(BS.CASES)
_gpu_cache = {}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _gpu(case, word, degree, divide=False):
    """One call per (case, type, degree, mode), shared by the tests."""
    from siril_amd.background import subsky
    key = (case, word, degree, divide)
    if key not in _gpu_cache:
        R = BS.reference(case, word)
        out, info = subsky(_dev(R["frames"]), degree, R["S"], R["tol"], divide=divide)
        _gpu_cache[key] = (out.cpu().numpy(), info)
    return _gpu_cache[key]


def _ulp_distance(a, b):
    """Distance in float32 steps, by the ordered integer key."""
    def key(x):
        bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
        return np.where(bits >> 31 != 0, 0x80000000 - bits, bits)
    return np.abs(key(a) - key(b))


# ---- box medians -------------------------------------------------------------
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", CASE_IDS)
def test_box_medians_and_selection_bit_for_bit(case, word):
    R = BS.reference(case, word)
    out, info = _gpu(case, word, 1)
    assert info["grid"] == R["grid"]
    for p, pl in enumerate(R["planes"]):
        # the selection is compared only where it is not on the knife's edge
        assert np.min(np.abs(pl["med"].astype(np.float64) - pl["T"])) > 1e-6 * abs(pl["T"])
        assert np.array_equal(info["med"][p].view(np.uint32), pl["med"].view(np.uint32)), p
        assert np.array_equal(info["keep"][p], pl["keep"]), p
        assert int(info["kept"][p]) == pl["kept"]
        assert int(info["status"][p]) == 0


def test_box_medians_with_ties_word():
    """A WORD plane of four levels: every box is full of ties."""
    from siril_amd.background import subsky
    rng = np.random.RandomState(5)
    levels = np.array([1200, 1201, 1300, 9000], np.uint16)
    fr = levels[rng.randint(0, 4, (2, 77, 131))]
    g = BR.grid(131, 77, 10)
    out, info = subsky(_dev(fr), 1, 10, 1.0, strict=False)
    for p in range(2):
        want = BR.box_medians(fr[p], g)
        assert np.array_equal(info["med"][p].view(np.uint32), want.view(np.uint32))
        assert set(np.unique(want)) <= set(np.unique(BR.to_float(levels)))
        keep, kept, *_ = BR.select(want, 1.0)
        assert np.array_equal(info["keep"][p], keep) and int(info["kept"][p]) == kept


def test_box_medians_key_order_and_non_finite():
    """NaN of both signs, +-inf, negative samples and signed zeros inside the
    boxes: the order is the ordered key's, a non-finite median becomes 0."""
    from siril_amd.background import subsky
    rng = np.random.RandomState(9)
    w, h = 131, 77
    fr = rng.normal(0.0, 1.0, (1, h, w)).astype(np.float32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)
    special[1] = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    pick = rng.randint(0, 12, (h, w))
    fr[0] = np.where(pick < 6, special[np.minimum(pick, 5)], fr[0])
    # boxes whose median is +inf, -inf and NaN
    g = BR.grid(w, h, 10)
    cx, cy = BR.centres(g)
    for k, v in ((0, np.inf), (1, -np.inf), (2, np.nan)):
        fr[0, cy[0] - 12:cy[0] + 13, cx[k] - 12:cx[k] + 13] = v
    want = BR.box_medians(fr[0], g)
    assert want[0] == 0.0 and want[1] == 0.0 and want[2] == 0.0
    out, info = subsky(_dev(fr), 1, 10, 1.0, strict=False)
    assert np.array_equal(info["med"][0].view(np.uint32), want.view(np.uint32))
    assert np.isfinite(info["med"]).all()
    keep, kept, *_ = BR.select(want, 1.0)
    assert np.array_equal(info["keep"][0], keep) and int(info["kept"][0]) == kept


def test_largest_grid():
    """K = 8190 of the 8192 allowed: the fit workgroup's LDS at its largest,
    eight boxes per thread in the rank counts."""
    from siril_amd.background import subsky
    w, h, S = 115, 114, 115
    g = BR.grid(w, h, S)
    assert g["K"] == 8190
    fr = BS.plane(w, h, 1, False)[None]
    med = BR.box_medians(fr[0], g)
    keep, kept, T, m, mad = BR.select(med, 1.0)
    assert np.min(np.abs(med.astype(np.float64) - T)) > 1e-6 * abs(T)
    st, c, mean = BR.fit(med, keep, g, w, h, 1)
    assert st == 0
    out, info = subsky(_dev(fr), 1, S, 1.0)
    assert np.array_equal(info["med"][0].view(np.uint32), med.view(np.uint32))
    assert np.array_equal(info["keep"][0], keep) and int(info["kept"][0]) == kept
    b, bg = BR.background(c, w, h), BR.background(info["coef"][0], w, h)
    st2, c2, mean2 = BR.fit(med, keep, g, w, h, 1, descending=True)
    floor = max(np.max(np.abs(b - BR.background(c2, w, h))), 4 * 2.0 ** -52 * np.max(np.abs(b)))
    assert np.max(np.abs(bg - b)) <= 100 * floor
    assert np.array_equal(out.cpu().numpy()[0].view(np.uint32),
                          BR.correct(fr[0], info["coef"][0], info["mean"][0]).view(np.uint32))


# ---- fit ----------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", CASE_IDS)
def test_fit_within_the_rounding_floor(case, word, degree):
    """The background from the GPU's coefficients against the restatement's,
    within 100 x the restatement's own rounding floor: the largest difference
    over the plane between its fit and the same fit with the kept boxes summed
    in descending order, not below 4 * 2^-52 * max|b|."""
    R = BS.reference(case, word)
    out, info = _gpu(case, word, degree)
    w, h = R["w"], R["h"]
    for p, pl in enumerate(R["planes"]):
        st, c, mean = pl["fits"][degree]
        st2, c2, mean2 = pl["rev"][degree]
        assert st == 0 and st2 == 0 and int(info["status"][p]) == 0
        b = BR.background(c, w, h)
        floor = max(np.max(np.abs(b - BR.background(c2, w, h))), 4 * 2.0 ** -52 * np.max(np.abs(b)))
        dist = np.max(np.abs(BR.background(info["coef"][p], w, h) - b))
        dmean = abs(float(info["mean"][p]) - mean)
        print(f"{case} word={int(word)} degree={degree} plane={p}: floor {floor:.3e} gpu distance {dist:.3e} "
              f"mean distance {dmean:.3e}")
        assert dist <= 100 * floor
        assert dmean <= 100 * floor
        assert np.all(info["coef"][p][BR.ncoef(degree):] == 0.0)


# ---- apply ----------------------------------------------------------------------
@pytest.mark.parametrize("divide", [False, True])
@pytest.mark.parametrize("degree", [1, 4])
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", ["small_t1", "wide"])
def test_apply_bit_for_bit_from_the_gpus_coefficients(case, word, degree, divide):
    R = BS.reference(case, word)
    out, info = _gpu(case, word, degree, divide)
    for p in range(BS.NPLANES):
        want = BR.correct(R["frames"][p], info["coef"][p], info["mean"][p], 0, divide)
        assert np.array_equal(out[p].view(np.uint32), want.view(np.uint32)), p


@pytest.mark.parametrize("degree", [1, 4])
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", CASE_IDS)
def test_end_to_end_within_one_ulp(case, word, degree):
    R = BS.reference(case, word)
    out, info = _gpu(case, word, degree)
    for p, pl in enumerate(R["planes"]):
        st, c, mean = pl["fits"][degree]
        want = BR.correct(R["frames"][p], c, mean)
        assert _ulp_distance(out[p], want).max() <= 1, p


def test_nan_samples_pass_through():
    """There is no clamp: a NaN sample stays NaN in both modes, and every other
    sample is the restatement's."""
    from siril_amd.background import subsky
    fr = BS.frames("small_t1", False).copy()
    fr[0, 40, 60] = np.nan          # a single sample: no box median changes class
    for divide in (False, True):
        out, info = subsky(_dev(fr), 2, 10, 1.0, divide=divide)
        out = out.cpu().numpy()
        assert np.isnan(out[0, 40, 60]) and np.isnan(out).sum() == 1
        want = BR.correct(fr[0], info["coef"][0], info["mean"][0], 0, divide)
        assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))


# ---- paths ----------------------------------------------------------------------
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", ["small_t1", "wide"])
def test_vector_tail_and_scalar_form_give_the_same_bits(case, word):
    """200 x 150 planes lie 16-byte aligned one after the other and W*H = 30000
    is no multiple of 256 (nor of the 512 pixels of a WORD group): the plain
    call runs the vector kernel and the scalar tail.  131 x 77 = 10087 samples
    are odd, so the plain call is all scalar; padded to a stride of 10088 the
    planes go through the vector kernel, whose lanes then cross rows (131 is no
    multiple of 4).  A plane stride of W*H + 3 and a base offset by one sample
    take the scalar form for everything.  All give the same bits."""
    import torch
    from siril_amd.background import _params, subsky_device
    from siril_amd.stacking import Context
    R = BS.reference(case, word)
    w, h, P = R["w"], R["h"], BS.NPLANES
    assert (w * h) % 256 != 0 and w * h > 512
    ref_out, ref_info = _gpu(case, word, 3)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    prm = _params(3, R["S"], R["tol"], False)
    fr = R["frames"]
    tdt = torch.int16 if word else torch.float32
    padded = (w * h // 8 + 1) * 8
    for stride, offset in ((w * h + 3, 0), (w * h, 1), (padded, 0)):
        src = torch.zeros(offset + P * stride, dtype=tdt, device="cuda")
        dst = torch.full((offset + P * stride,), -7.0, dtype=torch.float32, device="cuda")
        for p in range(P):
            src[offset + p * stride: offset + p * stride + w * h] = _dev(fr[p]).reshape(-1)
        coef = torch.empty((P, 15), dtype=torch.float64, device="cuda")
        status = torch.empty(P, dtype=torch.int32, device="cuda")
        es = src.element_size()
        subsky_device(ctx, src.data_ptr() + offset * es, es, P, w, h, stride, prm, dst.data_ptr() + offset * 4,
                      d_coef=coef.data_ptr(), d_status=status.data_ptr())       # med, keep, mean, kept: the context's
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert not status.cpu().numpy().any()
        assert np.array_equal(coef.cpu().numpy().view(np.uint64), ref_info["coef"].view(np.uint64))
        for p in range(P):
            a = got[offset + p * stride: offset + p * stride + w * h].reshape(h, w)
            assert np.array_equal(a.view(np.uint32), ref_out[p].view(np.uint32)), (stride, offset, p)
            gap = got[offset + p * stride + w * h: offset + (p + 1) * stride]
            assert np.all(gap == -7.0)          # nothing written between the planes
        assert np.all(got[:offset] == -7.0)


def test_four_dimensional_input_and_in_place():
    from siril_amd.background import subsky
    R = BS.reference("wide", False)
    ref_out, ref_info = _gpu("wide", False, 2)
    t = _dev(R["frames"][None])                 # [1, 3, H, W]
    out, info = subsky(t, 2, R["S"], R["tol"], out=t)
    assert out is t and info["kept"].shape == (1, 3) and info["coef"].shape == (1, 3, 15)
    assert np.array_equal(out.cpu().numpy()[0].view(np.uint32), ref_out.view(np.uint32))
    assert np.array_equal(info["med"][0], ref_info["med"])


# ---- statuses -------------------------------------------------------------------
def test_statuses_and_strict():
    from siril_amd.background import subsky
    R = BS.reference("small_t1", False)
    ref_out, ref_info = _gpu("small_t1", False, 1)
    g = R["grid"]
    cx, cy = BR.centres(g)
    fr = R["frames"].copy()
    fr[1] = 0.0                                         # nothing kept: status 1
    # Plane 2: only the boxes of column 4 (the centre column, u = 0) are kept: status 2.  With every
    # other column at zero the median and the MAD of the box medians are zero, so T = 0 and nothing
    # is kept (status 1); the columns to the left are therefore -1 (their boxes are not > 0) and those
    # to the right 0, which leaves m = 0, MAD = a median of column 4, and T = 3 MAD above column 4.
    x0, x1 = cx[4] - 12, cx[4] + 13
    fr[2][:, :x0] = -1.0
    fr[2][:, x1:] = 0.0
    want2 = BR.subsky_plane(fr[2], 1, R["S"], 3.0)[1]
    assert want2["status"] == 2 and want2["kept"] == g["ny"] and set(np.nonzero(want2["keep"])[0] % g["nx"]) == {4}
    t = _dev(fr)
    out, info = subsky(t, 1, R["S"], 3.0, strict=False)
    out = out.cpu().numpy()
    assert list(info["status"]) == [0, 1, 2]
    assert int(info["kept"][1]) == 0 and int(info["kept"][2]) == g["ny"]
    assert np.array_equal(info["keep"][2], want2["keep"])
    assert np.array_equal(out[1].view(np.uint32), fr[1].view(np.uint32))
    assert np.array_equal(out[2].view(np.uint32), fr[2].view(np.uint32))
    assert not info["coef"][1:].any() and not info["mean"][1:].any()
    # plane 0 is what it is without the failing neighbours
    alone, ainfo = subsky(_dev(fr[:1]), 1, R["S"], 3.0)
    assert np.array_equal(out[0].view(np.uint32), alone.cpu().numpy()[0].view(np.uint32))
    assert np.array_equal(info["coef"][0].view(np.uint64), ainfo["coef"][0].view(np.uint64))
    with pytest.raises(ValueError) as e:
        subsky(t, 1, R["S"], 3.0)
    assert "plane (1,)" in str(e.value) and "status 1" in str(e.value)
    # a WORD plane with status 1 is its conversion
    wfr = np.zeros((1, 77, 131), np.uint16)
    wfr[0, 3, 5] = 40000
    out, info = subsky(_dev(wfr), 1, 10, 1.0, strict=False)
    assert int(info["status"][0]) == 1 and int(info["kept"][0]) == 0
    assert np.array_equal(out.cpu().numpy()[0].view(np.uint32), BR.to_float(wfr[0]).view(np.uint32))


def test_one_box_is_status_1():
    from siril_amd.background import subsky
    fr = np.full((2, 25, 25), 0.3, np.float32)
    out, info = subsky(_dev(fr), 1, 1, 1.0, strict=False)
    assert info["grid"]["K"] == 1 and list(info["status"]) == [1, 1] and list(info["kept"]) == [1, 1]
    assert info["med"][0, 0] == np.float32(0.3)
    assert np.array_equal(out.cpu().numpy(), fr)


def test_no_planes_and_refusals():
    import torch
    from siril_amd import SgpuError
    from siril_amd.background import subsky
    out, info = subsky(torch.empty((0, 77, 131), dtype=torch.float32, device="cuda"), 1, 10)
    assert tuple(out.shape) == (0, 77, 131) and info["med"].shape == (0, 45) and info["status"].shape == (0,)
    t = torch.zeros((1, 77, 131), dtype=torch.float32, device="cuda")
    for kw in (dict(degree=0), dict(degree=5), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(samples=0),
               dict(samples=200)):
        with pytest.raises(SgpuError):
            subsky(t, **kw)
    with pytest.raises(SgpuError):
        subsky(torch.zeros((1, 24, 131), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        subsky(t.double())

"""The thin-plate-spline background kernels (siril_amd/csrc/background_rbf.hip)
against the restatement (tests/bkg_rbf_ref.py), bit for bit: the solve seam on
hand-made and random systems, the whole call on the scenes of
tests/bkg_scenes.py (float32 and WORD, subtraction and division), the geometry
of the evaluation pass (vector tail, scalar form, lanes that cross rows), and
the edges (the cap, one sample, no sample, smooth, the empty call, in place).
tests/test_bkg_rbf.py pins, without a GPU, that every case here ends as
described."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_rbf_ref as RR  # noqa: E402
import bkg_rbf_scenes as RS  # noqa: E402
import bkg_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu

_gpu_cache = {}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64),
                          np.ascontiguousarray(b, np.float64).view(np.uint64))


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def _ref(key, smooth, lam_rel):
    """The restatement with the double lam_rel the library used (its own pow)."""
    assert abs(lam_rel / RR.lam_rel(smooth) - 1.0) < 1e-14
    return RS.plane_reference(key, smooth, None if lam_rel == RR.lam_rel(smooth) else lam_rel)


# ---- the solve seam ----------------------------------------------------------------
@pytest.mark.parametrize("name", RS.SEAM)
def test_solve_seam_bit_for_bit(name):
    from siril_amd.background import rbf_solve
    a = RS.seam_systems(name)
    want_x, want_st = RS.seam_reference(name)
    assert list(want_st) == RS.SEAM_STATUS[name]
    d = _dev(a)
    x, st = rbf_solve(d)
    assert np.array_equal(st, want_st)
    assert _same64(x, want_x)
    assert _same64(d.cpu().numpy(), a)            # the caller's systems are left alone
    x2, st2 = rbf_solve(d)                        # the same bits on a second call
    assert np.array_equal(st2, st) and _same64(x2, x)


def test_solve_seam_refusals():
    import torch
    from siril_amd._lib import SgpuError
    from siril_amd.background import rbf_solve
    with pytest.raises(SgpuError):
        rbf_solve(torch.zeros((1, 1026, 1027), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        rbf_solve(torch.zeros((1, 3, 3), dtype=torch.float64, device="cuda"))
    x, st = rbf_solve(torch.zeros((0, 3, 4), dtype=torch.float64, device="cuda"))
    assert x.shape == (0, 3) and st.shape == (0,)


# ---- the whole call ----------------------------------------------------------------
def _gpu(case, word, divide):
    from siril_amd.background import subsky_rbf
    key = (case, word, divide)
    if key not in _gpu_cache:
        w, h, S, tol = SC.CASES[case]
        out, info = subsky_rbf(_dev(SC.frames(case, word)), S, tol, 0.5, divide=divide)
        _gpu_cache[key] = (out.cpu().numpy(), info)
    return _gpu_cache[key]


@pytest.mark.parametrize("divide", [False, True])
@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", list(SC.CASES))
def test_whole_call_bit_for_bit(case, word, divide):
    from siril_amd.background import subsky
    out, info = _gpu(case, word, divide)
    w, h, S, tol = SC.CASES[case]
    # medians and mask are the polynomial path's
    _, pinfo = subsky(_dev(SC.frames(case, word)), 1, S, tol)
    assert _same32(info["med"], pinfo["med"]) and np.array_equal(info["keep"], pinfo["keep"])
    assert np.array_equal(info["kept"], pinfo["kept"])
    for p in range(SC.NPLANES):
        r = _ref(("scene", case, int(word), p), 0.5, info["lam_rel"])
        assert info["grid"] == r["grid"]
        assert _same32(info["med"][p], r["med"]) and np.array_equal(info["keep"][p], r["keep"])
        assert int(info["status"][p]) == 0 and int(info["kept"][p]) == r["fit"]["n"]
        assert _same64(info["weights"][p], r["weights"]), (case, word, p)
        assert _same64(info["mean"][p], r["mean"])
        assert _same32(out[p], r["div"] if divide else r["sub"]), (case, word, p)


# ---- the geometry of the evaluation pass ---------------------------------------------
@pytest.mark.parametrize("word", [False, True])
def test_evaluation_pass_geometry(word):
    """131 x 77 = 10087 samples per plane, an odd number.  A stride of W*H + 3 from a base one sample in is
    the scalar form throughout; a padded 16-byte stride from an aligned base is the vector form, with a
    scalar tail (W*H is no multiple of 256 or 512) and 4-pixel lanes that cross rows (131 is odd).  Both
    give the restatement's bits, as the contiguous call of test_whole_call_bit_for_bit does."""
    import torch
    from siril_amd.background import subsky_rbf_device
    from siril_amd.stacking import Context
    case = "small_t1"
    w, h, S, tol = SC.CASES[case]
    fr = SC.frames(case, word)
    P, npix = fr.shape[0], w * h
    assert npix % 2 == 1
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    want = None
    for stride, base in ((npix + 3, 1), ((npix + 63) // 64 * 64 + 64, 0)):
        host = np.zeros(P * stride + 8, fr.dtype)
        for p in range(P):
            host[base + p * stride: base + p * stride + npix] = fr[p].ravel()
        d_in = _dev(host)
        d_out = torch.full((P * stride + 8,), -7.0, dtype=torch.float32, device="cuda")
        lam = subsky_rbf_device(ctx, d_in.data_ptr() + base * d_in.element_size(), d_in.element_size(), P, w, h,
                                stride, S, tol, 0.5, False, d_out.data_ptr() + base * 4)
        got = d_out.cpu().numpy()
        if want is None:
            want = [_ref(("scene", case, int(word), p), 0.5, lam)["sub"] for p in range(P)]
        used = np.zeros(P * stride + 8, bool)
        for p in range(P):
            sl = slice(base + p * stride, base + p * stride + npix)
            used[sl] = True
            assert _same32(got[sl].reshape(h, w), want[p]), (stride, base, p)
        assert (got[~used] == -7.0).all()         # nothing written between or after the planes
    ctx.close()


# ---- the edges -----------------------------------------------------------------------
@pytest.mark.parametrize("word", [False, True])
def test_cap_1023_samples(word):
    from siril_amd.background import subsky_rbf
    w, h, S, tol = RS.CAP
    plane = RS.edge_plane(w, h, word)
    out, info = subsky_rbf(_dev(plane[None]), S, tol, 0.5)
    r = _ref(("cap", int(word)), 0.5, info["lam_rel"])
    assert info["grid"]["K"] == 1023 and int(info["kept"][0]) == 1023 and int(info["status"][0]) == 0
    assert _same64(info["weights"][0], r["weights"])
    assert _same64(info["mean"][0], r["mean"])
    assert _same32(out.cpu().numpy()[0], r["sub"])


def test_more_than_1024_boxes_refused():
    import torch
    from siril_amd._lib import SgpuError
    from siril_amd.background import rbf_check, subsky_rbf
    w, h, S = RS.CAP_REFUSED
    with pytest.raises(SgpuError):
        rbf_check(w, h, S)
    with pytest.raises(SgpuError):
        subsky_rbf(torch.ones((1, h, w), dtype=torch.float32, device="cuda"), S, 1e9)


@pytest.mark.parametrize("word", [False, True])
def test_one_sample(word):
    from siril_amd.background import subsky_rbf
    w, h, S, tol = RS.ONE
    plane = RS.edge_plane(w, h, word)
    out, info = subsky_rbf(_dev(plane[None]), S, tol)
    r = _ref(("one", int(word)), 0.5, info["lam_rel"])
    wts = info["weights"][0]
    assert int(info["kept"][0]) == 1 and int(info["status"][0]) == 0
    assert wts[0] == 0.0 and not np.signbit(wts[0]) and wts[1] == float(info["med"][0, 0]) == info["mean"][0]
    assert _same64(wts, r["weights"])
    assert _same32(out.cpu().numpy()[0], r["sub"])


@pytest.mark.parametrize("word", [False, True])
def test_zero_plane_status_1_output_is_the_converted_input(word):
    from siril_amd.background import subsky_rbf
    import bkg_ref as BR
    fr = SC.frames("small_t1", word).copy()
    fr[1] = 0
    with pytest.raises(ValueError, match="no sample box kept"):
        subsky_rbf(_dev(fr), 10, 1.0)
    out, info = subsky_rbf(_dev(fr), 10, 1.0, strict=False)
    assert info["status"].tolist() == [0, 1, 0] and int(info["kept"][1]) == 0
    assert not info["weights"][1].any() and info["mean"][1] == 0.0
    out = out.cpu().numpy()
    assert _same32(out[1], BR.to_float(fr[1]))
    for p in (0, 2):
        assert _same32(out[p], _ref(("scene", "small_t1", int(word), p), 0.5, info["lam_rel"])["sub"])


@pytest.mark.parametrize("smooth", [0.0, 0.5, 1.0])
def test_smooth(smooth):
    from siril_amd.background import subsky_rbf
    out, info = subsky_rbf(_dev(SC.frames("small_t3", False)[:1]), 10, 3.0, smooth)
    r = _ref(("scene", "small_t3", 0, 0), smooth, info["lam_rel"])
    assert _same64(info["weights"][0], r["weights"])
    assert _same32(out.cpu().numpy()[0], r["sub"])


@pytest.mark.parametrize("smooth", [-0.1, 1.5, float("nan")])
def test_smooth_refused(smooth):
    from siril_amd._lib import SgpuError
    from siril_amd.background import subsky_rbf
    with pytest.raises(SgpuError):
        subsky_rbf(_dev(SC.frames("small_t3", False)[:1]), 10, 3.0, smooth)


def test_empty_call():
    import torch
    from siril_amd.background import subsky_rbf
    out, info = subsky_rbf(torch.empty((0, 77, 131), dtype=torch.float32, device="cuda"), 10)
    assert tuple(out.shape) == (0, 77, 131) and info["status"].shape == (0,) and info["weights"].shape == (0, 1025)


def test_out_aliased_to_float_input():
    from siril_amd._lib import SgpuError
    from siril_amd.background import subsky_rbf, subsky_rbf_device
    from siril_amd.stacking import Context
    fr = _dev(SC.frames("small_t1", False))
    out, info = subsky_rbf(fr, 10, 1.0, out=fr)
    assert out.data_ptr() == fr.data_ptr()
    want, _ = _gpu("small_t1", False, False)
    assert _same32(out.cpu().numpy(), want)
    # WORD input cannot be its own output
    wd = _dev(SC.frames("small_t1", True))
    with pytest.raises(ValueError):
        subsky_rbf(wd, 10, 1.0, out=wd)
    ctx = Context(0)
    with pytest.raises(SgpuError):
        subsky_rbf_device(ctx, wd.data_ptr(), 2, 1, 131, 77, 131 * 77, 10, 1.0, 0.5, False, wd.data_ptr())
    ctx.close()


def test_kernel_times_reported():
    from siril_amd.background import rbf_last_kernel_ms, subsky_rbf
    from siril_amd.stacking import Context
    ctx = Context(0)
    subsky_rbf(_dev(SC.frames("small_t1", False)), 10, 1.0, ctx=ctx)
    ms = rbf_last_kernel_ms(ctx)
    assert len(ms) == 4 and all(v > 0.0 for v in ms) and ms[3] >= max(ms[:3])
    ctx.close()

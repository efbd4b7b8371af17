"""Drizzle, the parts that need no device: the size rule, the forward maps and
the refusals of the library's host side against tests/drizzle_ref.py, the
`seqapplyreg` parser and the .seq pieces of the command, and two properties of
the restatement itself over the maps the GPU tests use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drizzle_ref as DR  # noqa: E402
from warp_ref import rotation_H, translation_H  # noqa: E402

BAD_ARGUMENT = -21
PERSPECTIVE = np.array([[1.01, 0.02, -1.2], [-0.015, 0.99, 0.8], [2e-4, -1e-4, 1.0]])
W, H = 21, 13


def _maps():
    return {"identity": np.eye(3), "quarter": translation_H(0.25, 0.25), "shift": translation_H(-1.4, 0.7),
            "rotation": rotation_H(W, H, 1.5, 0.8, -0.6), "perspective": PERSPECTIVE,
            "mirror": np.array([[-1.0, 0, W - 1.25], [0, 1, 0.5], [0, 0, 1]])}


def test_output_size_rule():
    from siril_amd import SgpuError
    from siril_amd import registration as Rg
    for w, h, s in ((45, 23, 2.0), (45, 23, 1.5), (45, 23, 1.0), (45, 23, 0.5), (6000, 4000, 2.0), (7, 5, 0.1),
                    (33, 9, 0.3), (5, 5, 0.1), (256, 64, 0.25), (3, 3, 4.0)):
        assert Rg.drizzle_output_size(w, h, s) == DR.output_size(w, h, s)
    assert Rg.drizzle_output_size(45, 23, 1.5) == (68, 35) and Rg.drizzle_output_size(45, 23, 0.5) == (23, 12)
    for w, h, s in ((45, 23, 0.09), (45, 23, 4.01), (45, 23, float("nan")), (4, 4, 0.1), (0, 5, 1.0), (5, -1, 1.0)):
        with pytest.raises(SgpuError) as e:
            Rg.drizzle_output_size(w, h, s)
        assert e.value.code == BAD_ARGUMENT


def test_forward_maps():
    from siril_amd import registration as Rg
    # integer translations: exact, and the row flip turns dy into -dy
    Hs = np.stack([np.eye(3), translation_H(3, -2), translation_H(-7, 5)])
    A = Rg.drizzle_forward_maps(Hs, 0, 23)
    assert np.array_equal(A[1], [1, 0, 3, 0, 1, 2, 0, 0, 1]) and np.array_equal(A[2], [1, 0, -7, 0, 1, -5, 0, 0, 1])
    assert np.array_equal(A[0], np.eye(3).ravel())
    # general maps, each as the reference in turn: the restatement's bits
    Hs = np.stack(list(_maps().values()))
    for ref in range(len(Hs)):
        assert np.array_equal(Rg.drizzle_forward_maps(Hs, ref, H), DR.forward_maps(Hs, ref, H))
    # the map the frame warp inverts: M of the warp times A is the identity
    M = Rg.warp_inverse_maps(Hs, 3, H).reshape(-1, 3, 3)
    A = Rg.drizzle_forward_maps(Hs, 3, H).reshape(-1, 3, 3)
    for f in range(len(Hs)):
        assert np.allclose(M[f] @ A[f], np.eye(3), atol=1e-9)


def test_refusals():
    from siril_amd import SgpuError
    from siril_amd import registration as Rg
    ok = np.stack([np.eye(3), translation_H(0.25, 0.25)])

    def refused(fn, *a, **kw):
        with pytest.raises(SgpuError) as e:
            fn(*a, **kw)
        assert e.value.code == BAD_ARGUMENT

    singular = ok.copy()
    singular[1] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    refused(Rg.drizzle_forward_maps, singular, 0, 23)
    refused(Rg.drizzle_forward_maps, singular, 1, 23)             # as the reference too
    nonfinite = ok.copy()
    nonfinite[1, 0, 2] = np.inf
    refused(Rg.drizzle_forward_maps, nonfinite, 0, 23)
    refused(Rg.drizzle_forward_maps, ok, 2, 23)
    with pytest.raises(ValueError):
        DR.forward_maps(singular, 0, 23)
    # W = 1 - 0.05 x vanishes at x = 20: inside a 45-wide frame, outside a 10-wide one
    pole = ok.copy()
    pole[1] = [[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]]
    A = Rg.drizzle_forward_maps(pole, 0, 23)                      # the maps themselves are regular
    refused(Rg.drizzle_forward_maps, pole, 0, 23, width=45, scale=2.0)
    with pytest.raises(ValueError):
        DR.check_map(A[1], 45, 23, 2.0, 1.0, DR.SQUARE)
    Rg.drizzle_forward_maps(pole, 0, 23, width=10, scale=2.0)
    DR.check_map(A[1], 10, 23, 2.0, 1.0, DR.SQUARE)
    # the inverse map's denominator changes sign over the output although A's does not over the input:
    # a pole of M inside the output frame
    Ainv = np.array([[1, 0, 0], [0, 1, 0], [-0.05, 0, 1.0]])
    back = ok.copy()
    back[1] = np.linalg.inv(Ainv)
    Ab = DR.forward_maps(back, 0, 23)
    assert DR._w_regular(list(Ab[1]), -1.0, 45.0, -1.0, 23.0)
    refused(Rg.drizzle_forward_maps, back, 0, 23, width=45, scale=1.0)
    with pytest.raises(ValueError):
        DR.check_map(Ab[1], 45, 23, 1.0, 1.0, DR.SQUARE)
    # scale, pixfrac and kernel out of range
    for kw in (dict(scale=0.05), dict(scale=4.5), dict(pixfrac=0.0), dict(pixfrac=-0.5), dict(pixfrac=1.01),
               dict(kernel=3), dict(kernel=-1)):
        refused(Rg.drizzle_forward_maps, ok, 0, 23, width=45, **kw)
    with pytest.raises(ValueError):
        Rg.drizzle_forward_maps(ok, 0, 23, width=45, kernel="lanczos3")


def test_parse_seqapplyreg_command():
    from siril_amd import registration as Rg
    c = Rg.parse_seqapplyreg_command(["seqapplyreg", "light_"])
    assert (c.seq, c.layer, c.drizzle, c.scale, c.pixfrac, c.kernel, c.flat, c.interp, c.clamp, c.prefix) == \
        ("light_", 0, False, 1.0, 1.0, "square", None, Rg.OPENCV_LANCZOS4, True, "r_")
    c = Rg.parse_seqapplyreg_command("seqapplyreg pp_light -drizzle -scale=2 -pixfrac=0.5 -kernel=turbo "
                                     "-flat=master_flat -layer=1 -prefix=dz_".split())
    assert (c.seq, c.layer, c.drizzle, c.scale, c.pixfrac, c.kernel, c.flat, c.prefix) == \
        ("pp_light", 1, True, 2.0, 0.5, "turbo", "master_flat", "dz_")
    c = Rg.parse_seqapplyreg_command("pp_light -interp=cu -noclamp".split())
    assert (c.drizzle, c.interp, c.clamp) == (False, Rg.OPENCV_CUBIC, False)
    for k in ("point", "turbo", "square"):
        assert Rg.parse_seqapplyreg_command(["s", "-drizzle", f"-kernel={k}"]).kernel == k
    for bad in (["seqapplyreg"], ["seqapplyreg", "-drizzle"], ["s", "-scale=2"], ["s", "-pixfrac=0.5"],
                ["s", "-kernel=square"], ["s", "-flat=f"], ["s", "-drizzle", "-scale=0.05"],
                ["s", "-drizzle", "-scale=5"], ["s", "-drizzle", "-pixfrac=0"], ["s", "-drizzle", "-pixfrac=1.5"],
                ["s", "-drizzle", "-kernel=gaussian"], ["s", "-drizzle", "-kernel=lanczos3"],
                ["s", "-drizzle", "-flat="], ["s", "-drizzle", "-interp=cu"], ["s", "-drizzle", "-noclamp"],
                ["s", "-interp=spline"], ["s", "-prefix="], ["s", "-layer=-1"], ["s", "-noout"], ["s", "-framing=max"]):
        with pytest.raises(ValueError):
            Rg.parse_seqapplyreg_command(bad)


def test_register_parser_is_unchanged():
    """`register` keeps refusing -drizzle and takes none of the new options."""
    from siril_amd import registration as Rg
    for bad in (["s", "-drizzle"], ["s", "-scale=2"], ["s", "-pixfrac=0.5"], ["s", "-kernel=square"]):
        with pytest.raises(ValueError):
            Rg.parse_register_command(bad)
    c = Rg.parse_register_command(["register", "light_", "-noout"])
    assert c.noout and not hasattr(c, "drizzle")


def test_cli_knows_seqapplyreg():
    from siril_amd import cli
    assert "seqapplyreg <seq>" in cli.__doc__ and "-drizzle" in cli.__doc__


def test_write_seq_drizzle_flag_and_registration_reader(tmp_path):
    from siril_amd import registration as Rg
    from siril_amd.sequence import write_seq
    rng = np.random.default_rng(5)
    Hs = np.tile(np.eye(3), (4, 1, 1)) + rng.normal(0, 1e-3, (4, 3, 3))
    Hs[2] = 0.0
    vals = dict(fwhm=[3.5, 3.25, 0, 3.75], wfwhm=[3.5, 4.0, 0, 4.5], roundness=[0.9, 0.8, 0, 0.7],
                quality=[0.5, 0.25, 0, 0.125], bkg=[0.05, 0.06, 0.07, 0.08], nstars=[100, 90, 3, 80])
    a, b = tmp_path / "a.seq", tmp_path / "b.seq"
    write_seq(str(a), "a_", 4, reference=1, included=[True, True, False, True], homographies=Hs, reg_layer=1, **vals)
    write_seq(str(b), "a_", 4, reference=1, included=[True, True, False, True], homographies=Hs, reg_layer=1,
              drizzle=True, **vals)
    la, lb = a.read_text().splitlines(), b.read_text().splitlines()
    assert la[2] == "S 'a_' 1 4 3 5 1 4 0 0 0" and lb[2] == "S 'a_' 1 4 3 5 1 4 0 0 1"
    assert la[:2] + la[3:] == lb[:2] + lb[3:]
    write_seq(str(b), "a_", 4, reference=1, included=[True, True, False, True], homographies=Hs, reg_layer=1,
              drizzle=False, **vals)
    assert b.read_text() == a.read_text()
    inc, H2, v = Rg.read_seq_registration(str(a), 1)
    assert list(inc) == [True, True, False, True] and np.array_equal(H2, Hs)
    assert list(v["nstars"]) == vals["nstars"] and np.array_equal(v["quality"], vals["quality"])
    assert np.allclose(v["fwhm"], vals["fwhm"]) and np.allclose(v["bkg"], vals["bkg"])
    with pytest.raises(ValueError):
        Rg.read_seq_registration(str(a), 0)                   # no R0 lines
    write_seq(str(b), "a_", 4)
    with pytest.raises(ValueError):
        Rg.read_seq_registration(str(b))


def test_flat_weights():
    from siril_amd import registration as Rg
    flat = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 7.0]], np.float32)     # mean 2
    w = Rg.drizzle_flat_weights(flat)
    assert w.dtype == np.float32 and np.array_equal(w, np.array([[0.5, 1, 1.5], [0, 0, 3.5]], np.float32))
    w16 = Rg.drizzle_flat_weights(np.array([[100, 300]], np.uint16))
    assert np.array_equal(w16, np.array([[0.5, 1.5]], np.float32))
    with pytest.raises(ValueError):
        Rg.drizzle_flat_weights(np.zeros((2, 2), np.float32))


# ---- properties of the restatement ------------------------------------------
@pytest.mark.parametrize("scale", [2.0, 1.5, 1.0, 0.5])
@pytest.mark.parametrize("pixfrac", [1.0, 0.7, 0.5])
def test_reference_conserves_each_drop(scale, pixfrac):
    """SQUARE: for every input pixel whose drop lies inside the output, the
    double sum of a / jaco over the output pixels it touches is within 1e-12
    of 1 (the quad's area is split exactly; only the rounding of sgarea's
    double arithmetic remains)."""
    seen = 0
    fr = np.ones((H, W), np.float32)
    for name, Hm in _maps().items():
        A = DR.forward_maps(np.stack([np.eye(3), Hm]), 0, H)[1]
        _, _, tot = DR.drizzle_frame(fr, A, scale, pixfrac, DR.SQUARE, totals=True)
        inside = np.isfinite(tot)
        seen += int(inside.sum())
        if inside.any():
            dev = np.abs(tot[inside] - 1.0).max()
            print(f"{name} scale {scale} pixfrac {pixfrac}: {int(inside.sum())} drops inside, max |sum - 1| {dev:.3g}")
            assert dev <= 1e-12, (name, dev)
    assert seen > 3 * (W - 4) * (H - 4)


@pytest.mark.parametrize("kernel", ["square", "turbo", "point"])
@pytest.mark.parametrize("scale", [2.0, 1.5, 1.0, 0.5])
@pytest.mark.parametrize("pixfrac", [1.0, 0.7, 0.5])
def test_reference_keeps_a_constant(scale, pixfrac, kernel):
    """A constant frame drizzles to that constant within 4 float ulp wherever
    the weight is positive (the running mean of equal samples), and to exactly
    0 with weight 0 elsewhere."""
    c = np.float32(1234.5)
    fr = np.full((H, W), c, np.float32)
    ulp = float(np.spacing(c))
    covered = 0
    for name, Hm in _maps().items():
        A = DR.forward_maps(np.stack([np.eye(3), Hm]), 0, H)[1]
        out, cnt = DR.drizzle_frame(fr, A, scale, pixfrac, DR.KERNELS[kernel])
        pos = cnt > 0
        covered += int(pos.sum())
        assert not out[~pos].any() and (cnt >= 0).all()
        dev = np.abs(out[pos].astype(np.float64) - float(c)).max() / ulp
        print(f"{name} scale {scale} pixfrac {pixfrac} {kernel}: max deviation {dev:.2f} ulp")
        assert dev <= 4.0, (name, dev)
    assert covered > 0

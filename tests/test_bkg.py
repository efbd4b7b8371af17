"""The restatement of the polynomial background extraction (tests/bkg_ref.py,
DESIGN.md 6i) pinned without a GPU: the sample grid and its refusals, a planted
polynomial of every degree recovered, the closed-form mean of the model, the
conditions the GPU cases (tests/test_bkg_gpu.py) rely on, and the `seqsubsky`
command's parsing and refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_ref as BR  # noqa: E402
import bkg_scenes as BS  # noqa: E402


GRIDS = [((131, 77, 10), dict(dist=13, nx=9, ny=5, K=45, startx=1, starty=0)),
         ((200, 150, 20), dict(dist=10, nx=18, ny=13, K=234, startx=2, starty=2)),
         ((25, 25, 1), dict(dist=25, nx=1, ny=1, K=1, startx=0, starty=0)),
         ((6000, 4000, 20), dict(dist=300, nx=20, ny=14, K=280, startx=137, starty=37))]
REFUSED = [(24, 100, 1), (100, 24, 1), (100, 100, 0), (100, 100, 101), (116, 115, 116)]


@pytest.mark.parametrize("shape,want", GRIDS)
def test_grid_values(shape, want):
    assert BR.grid(*shape) == want
    # every box inside the plane
    cx, cy = BR.centres(want)
    assert cx[0] - BR.R >= 0 and cx[-1] + BR.R <= shape[0] - 1
    assert cy[0] - BR.R >= 0 and cy[-1] + BR.R <= shape[1] - 1


@pytest.mark.parametrize("shape", REFUSED)
def test_grid_refusals(shape):
    with pytest.raises(ValueError):
        BR.grid(*shape)


def test_grid_of_the_library_is_the_restatement():
    """sgpu_bkg_grid is host only: it runs without a device."""
    from siril_amd import SgpuError
    from siril_amd.background import sample_grid
    for shape, want in GRIDS + [((115, 114, 115), BR.grid(115, 114, 115))]:
        assert sample_grid(*shape) == want
    assert BR.grid(115, 114, 115)["K"] == 8190
    for shape in REFUSED:
        with pytest.raises(SgpuError) as e:
            sample_grid(*shape)
        assert e.value.code != 0 and "subsky" in str(e.value)


def test_parameter_refusals():
    BR.check_params(1, 0.0)
    for d, t in ((0, 1.0), (5, 1.0), (1, -0.1), (1, float("nan")), (1, float("inf"))):
        with pytest.raises(ValueError):
            BR.check_params(d, t)


def test_term_order():
    assert BR.TERMS == [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3),
                        (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
    assert [BR.ncoef(d) for d in (1, 2, 3, 4)] == [3, 6, 10, 15]


def _planted(degree, seed):
    rng = np.random.RandomState(seed)
    c = np.zeros(15)
    c[:BR.ncoef(degree)] = rng.uniform(-0.05, 0.05, BR.ncoef(degree))
    c[0] = 0.2
    return c


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_planted_polynomial_comes_back(degree):
    """A noiseless float64 polynomial plane sampled at the box centres (the
    median of a box of a curved surface is not its centre value, and B2's
    medians are float32: both are left out here) is fitted back to 1e-9
    relative in the background."""
    w, h = 131, 77
    g = BR.grid(w, h, 10)
    c = _planted(degree, 7 + degree)
    plane = BR.background(c, w, h)
    cx, cy = BR.centres(g)
    med = np.array([plane[y, x] for y in cy for x in cx], np.float64)
    st, got, mean = BR.fit(med, np.ones(g["K"], np.uint8), g, w, h, degree)
    assert st == 0
    b = BR.background(got, w, h)
    assert np.max(np.abs(b - plane)) <= 1e-9 * np.max(np.abs(plane))
    assert np.all(got[BR.ncoef(degree):] == 0.0)


@pytest.mark.parametrize("shape", [(131, 77), (200, 150), (25, 25)])
def test_closed_form_mean_is_the_mean_of_the_plane(shape):
    w, h = shape
    for degree in (1, 2, 3, 4):
        c = _planted(degree, 40 + degree)
        want = float(np.mean(BR.background(c, w, h)))
        assert abs(BR.model_mean(c, w, h) - want) <= 1e-13 * abs(want)


def test_box_median_key_order_and_non_finite_rule():
    g = BR.grid(25, 25, 1)
    pl = np.zeros((25, 25), np.float32)
    flat = pl.ravel()
    flat[:312] = -1.0
    flat[312] = np.float32(-0.0)
    flat[313:] = 2.0
    assert BR.box_medians(pl, g).view(np.uint32)[0] == 0x80000000       # -0 sorts below +0 and is kept as it is
    flat[:313] = np.nan
    flat[313:] = 1.0
    assert BR.box_medians(pl, g)[0] == 0.0                              # +NaN sorts last: the median is NaN -> 0
    flat[:313] = -np.inf
    assert BR.box_medians(pl, g)[0] == 0.0 and BR.box_medians(pl, g).view(np.uint32)[0] == 0
    flat[:] = 1.0
    flat[:312] = np.float32(np.nan) * np.float32(-1.0)                  # some NaNs on either side: order by the bits
    assert BR.box_medians(pl, g)[0] == 1.0


def test_constant_level_keeps_every_box_and_zero_none():
    g = BR.grid(60, 50, 4)
    med = np.full(g["K"], 0.25, np.float32)
    keep, kept, T, m, mad = BR.select(med, 1.0)
    assert kept == g["K"] and mad == 0.0 and T == 0.25
    keep, kept, *_ = BR.select(np.zeros(g["K"], np.float32), 1.0)
    assert kept == 0
    st, c, mean = BR.fit(np.zeros(g["K"], np.float32), keep, g, 60, 50, 1)
    assert st == 1 and not c.any() and mean == 0.0


def test_single_column_is_status_2():
    g = BR.grid(131, 77, 10)
    med = np.zeros(g["K"], np.float32)
    keep = np.zeros(g["K"], np.uint8)
    for j in range(g["ny"]):
        med[j * g["nx"] + 4] = 0.1 + 0.01 * j
        keep[j * g["nx"] + 4] = 1
    assert BR.fit(med, keep, g, 131, 77, 1)[0] == 2


@pytest.mark.parametrize("word", [False, True])
@pytest.mark.parametrize("case", list(BS.CASES))
def test_conditions_the_gpu_cases_rely_on(case, word):
    """Every plane of every GPU case, at every degree: at least as many boxes
    kept as coefficients (and at least 15), status 0, no box median within 1e-6
    relative of the threshold, and a normal matrix conditioned below 1e5 (the
    Cholesky solve then loses at most about 1e5 * 2^-52 = 2e-11 relative, far
    below a float32 ulp): a tolerance of the GPU tests never hides a degenerate
    fit or a selection on the knife's edge."""
    R = BS.reference(case, word)
    for pl in R["planes"]:
        assert pl["kept"] >= 15
        assert np.min(np.abs(pl["med"].astype(np.float64) - pl["T"])) > 1e-6 * abs(pl["T"])
        # the raised patch is above the threshold: its boxes are dropped
        assert pl["kept"] < R["grid"]["K"]
        for d in (1, 2, 3, 4):
            st, c, mean = pl["fits"][d]
            assert st == 0 and pl["kept"] >= BR.ncoef(d)
            A, _ = BR.normal_equations(pl["med"], pl["keep"], R["grid"], R["w"], R["h"], d)
            assert np.linalg.cond(np.array(A)) < 1e5


def test_restatement_removes_a_planted_gradient():
    w, h = 200, 150
    x = np.arange(w, dtype=np.float64)[None, :] / (w - 1)
    pl = (0.2 + 0.05 * x + np.zeros((h, 1))).astype(np.float32)
    out, info = BR.subsky_plane(pl, 1)
    assert info["status"] == 0
    slope = np.polyfit(np.arange(w), out.astype(np.float64).mean(axis=0), 1)[0] * (w - 1)
    assert abs(slope) < 0.01 * 0.05
    assert abs(float(out.mean()) - float(pl.mean())) < 1e-6


def test_division_by_a_zero_background_is_zero():
    pl = np.full((30, 40), 0.5, np.float32)
    assert not BR.correct(pl, np.zeros(15), 1.0, divide=True).any()
    c = np.zeros(15)
    c[1] = 1.0                              # b = u: zero only where u is, at the centre column of an odd width
    out = BR.correct(np.full((25, 41), 0.5, np.float32), c, 2.0, divide=True)
    assert np.all(out[:, 20] == 0.0) and np.all(out[:, :20] < 0.0) and np.all(out[:, 21:] > 0.0)


def test_parse_seqsubsky():
    from siril_amd.background import parse_seqsubsky_command as parse
    c = parse("seqsubsky pp_light 1".split())
    assert (c.seq, c.degree, c.samples, c.tolerance, c.prefix) == ("pp_light", 1, 20, 1.0, "bkg_")
    c = parse("pp_light 4 -samples=10 -tolerance=2.5 -nodither -prefix=b_".split())
    assert (c.degree, c.samples, c.tolerance, c.prefix) == (4, 10, 2.5, "b_")
    for bad, word in (("seqsubsky", "sequence"), ("seqsubsky seq", "degree"), ("seqsubsky seq 0", "1 .. 4"),
                      ("seqsubsky seq 5", "1 .. 4"), ("seqsubsky seq x", "degree"), ("seqsubsky seq 1 -rbf", "-rbf"),
                      ("seqsubsky seq -rbf", "-rbf"), ("seqsubsky seq 1 -smooth=0.5", "-smooth"),
                      ("seqsubsky seq 1 -samples=0", "-samples"), ("seqsubsky seq 1 -tolerance=-1", "-tolerance"),
                      ("seqsubsky seq 1 -tolerance=nan", "-tolerance"), ("seqsubsky seq 1 -dither", "-dither")):
        with pytest.raises(ValueError) as e:
            parse(bad.split())
        assert word in str(e.value), bad


def test_seqsubsky_refuses_ser_sequences(tmp_path):
    from siril_amd.background import run_seqsubsky
    seq = tmp_path / "s.seq"
    seq.write_text("#Siril sequence file. Contains general information about the sequence and per-image data\n"
                   "S 's' 1 2 2 5 0 4 0 0\nTS\nL 1\nI 1 1\nI 2 1\n")
    with pytest.raises(ValueError) as e:
        run_seqsubsky(["seqsubsky", str(seq), "1"])
    assert "SER" in str(e.value) and "seqsubsky" in str(e.value)

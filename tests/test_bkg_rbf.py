"""The restatement of the thin-plate-spline background extraction
(tests/bkg_rbf_ref.py) pinned without a GPU: its logarithm
against the long-double one, its LU against numpy.linalg.solve on the systems
the GPU tests use, the tie rule, singular systems and order 1 on hand-made
matrices, that every GPU case ends as described (so no bit comparison passes
vacuously), and the `subsky` command's parser."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_rbf_ref as RR  # noqa: E402
import bkg_rbf_scenes as RS  # noqa: E402
import bkg_scenes as SC  # noqa: E402

EPS = 2.0 ** -52


# ---- R2 ----
def test_rbf_log_within_three_ulp_of_the_long_double_log():
    """2e6 log-uniform points of [1e-8, 8]; measured 2.67 ulp (ten terms), bound 3."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.fail("this platform's long double is no wider than double: the measurement needs it")
    rng = np.random.RandomState(20240)
    s = np.exp(rng.uniform(np.log(1e-8), np.log(8.0), 2000000))
    ref = np.log(s.astype(np.longdouble))
    got = RR.rbf_log(s)
    ulp = np.spacing(np.abs(ref.astype(np.float64)))
    err = float((np.abs(got.astype(np.longdouble) - ref) / ulp).max())
    print("rbf_log: max error %.3f ulp" % err)
    assert err <= 3.0


def test_phi_is_r2_log_r_and_plus_zero_at_zero():
    s = np.array([0.0, 1.0, 0.25, 4.0, 1e-8])
    p = RR.phi(s)
    assert p[0] == 0.0 and not np.signbit(p[0]) and p[1] == 0.0
    r = np.sqrt(s[2:])
    assert np.allclose(p[2:], r * r * np.log(r), rtol=1e-14, atol=0)


def test_axes_one_scale():
    x0, y0, a = RR.axes(131, 77)
    assert (x0, y0, a) == (65.0, 38.0, 1.0 / 65.0)
    x0, y0, a = RR.axes(77, 131)
    assert a == 1.0 / 65.0


def test_lam_rel():
    assert abs(RR.lam_rel(0.5) / 1e-4 - 1.0) < 1e-15
    assert abs(RR.lam_rel(0.0) / (1e-4 * 10 ** -1.5) - 1.0) < 1e-14
    assert abs(RR.lam_rel(1.0) / (1e-4 * 10 ** 1.5) - 1.0) < 1e-14


# ---- R4 ----
def _against_numpy(aug, cond_range=None):
    A, b = aug[:, :-1], aug[:, -1]
    st, x = RR.lu_solve(aug)
    assert st == 0
    ref = np.linalg.solve(A, b)
    cond = float(np.linalg.cond(A))
    margin = 100.0 * cond * EPS * float(np.abs(ref).max())
    err = float(np.abs(x - ref).max())
    print("order %d: condition %.3g, |x - numpy| %.3g, margin %.3g" % (len(b), cond, err, margin))
    assert err <= margin
    if cond_range:
        assert cond_range[0] <= cond <= cond_range[1], cond
    return cond


@pytest.mark.parametrize("case,cond", [("small_t1", 6.2e2), ("wide", 9.7e3)])
def test_lu_against_numpy_on_the_scene_systems(case, cond):
    r = RS.plane_reference(("scene", case, 0, 0))
    _against_numpy(r["fit"]["aug"], (0.95 * cond, 1.05 * cond))
    for word in (0, 1):
        for p in range(SC.NPLANES):
            _against_numpy(RS.plane_reference(("scene", case, word, p))["fit"]["aug"])


def test_lu_against_numpy_on_the_cap_case():
    r = RS.plane_reference(("cap", 0))
    assert r["fit"]["n"] == 1023
    _against_numpy(r["fit"]["aug"], (0.95 * 3.2e5, 1.05 * 3.2e5))


def test_lu_against_numpy_on_the_6000x4000_grid():
    """S = 20: 280 boxes.  The condition depends on which boxes are kept: 3.9e4 with all of them, 8.7e3
    with the 191 that tolerance 1.0 keeps of the benchmark's sky (the issue's 2.5e4, whose selection is
    not stated, lies between the two)."""
    full = RS.grid_system(6000, 4000, 20)
    assert full.shape == (281, 282)
    c_full = _against_numpy(full, (0.95 * 3.86e4, 1.05 * 3.86e4))
    bench = RS.grid_system(6000, 4000, 20, "bench")
    assert bench.shape == (192, 193)
    c_bench = _against_numpy(bench, (0.95 * 8.7e3, 1.05 * 8.7e3))
    assert c_bench < 2.5e4 < c_full


@pytest.mark.parametrize("name", ["order2", "tie", "dense70", "dense1025", "eight"])
def test_lu_against_numpy_on_the_seam_systems(name):
    a = RS.seam_systems(name)
    x, st = RS.seam_reference(name)
    assert list(st) == RS.SEAM_STATUS[name]
    for s in range(len(a)):
        if st[s] == 0:
            _against_numpy(a[s])


def test_lu_tie_rule_lowest_row_among_equals():
    a = RS.TIE
    assert abs(a[1, 0]) == abs(a[2, 0]) > abs(a[0, 0])         # equal maxima in the first pivot column
    st, x = RR.lu_solve(a)
    st2, x2 = RR.lu_solve(a, tie_last=True)
    assert st == 0 and st2 == 0
    assert np.allclose(x, x2, rtol=1e-13)
    assert not np.array_equal(x.view(np.uint64), x2.view(np.uint64))       # the system tells the two rules apart
    # the right rule by hand: row 1 is the pivot row of step 0
    b = a.copy()
    b[[0, 1]] = b[[1, 0]]
    l1, l2 = b[1, 0] / b[0, 0], b[2, 0] / b[0, 0]
    b[1, 1:] = b[1, 1:] - l1 * b[0, 1:]
    b[2, 1:] = b[2, 1:] - l2 * b[0, 1:]
    if abs(b[2, 1]) > abs(b[1, 1]):
        b[[1, 2]] = b[[2, 1]]
    l = b[2, 1] / b[1, 1]
    b[2, 2:] = b[2, 2:] - l * b[1, 2:]
    x3 = np.zeros(3)
    x3[2] = b[2, 3] / b[2, 2]
    b[:2, 3] = b[:2, 3] - b[:2, 2] * x3[2]
    x3[1] = b[1, 3] / b[1, 1]
    b[:1, 3] = b[:1, 3] - b[:1, 1] * x3[1]
    x3[0] = b[0, 3] / b[0, 0]
    assert np.array_equal(x.view(np.uint64), x3.view(np.uint64))


def test_lu_singular_nan_and_order_one():
    for name in ("singular", "nan"):
        x, st = RS.seam_reference(name)
        assert list(st) == [2] and not x.any() and not np.signbit(x).any()
    x, st = RS.seam_reference("order1")
    assert list(st) == [0] and x[0, 0] == 1.5
    assert RR.lu_solve(np.array([[0.0, 1.0]]))[0] == 2
    assert RR.lu_solve(np.array([[np.inf, 1.0]]))[0] == 2
    # a NaN counts as the largest: it is picked at once
    assert RR.lu_solve(np.array([[1.0, 2.0, 1.0], [np.nan, 1.0, 1.0]]))[0] == 2
    x, st = RS.seam_reference("eight")
    assert not x[5].any()


# ---- the GPU cases end as described ----
@pytest.mark.parametrize("case", list(SC.CASES))
def test_scene_cases_end_as_described(case):
    for word in (0, 1):
        for p in range(SC.NPLANES):
            r = RS.plane_reference(("scene", case, word, p))
            f = r["fit"]
            assert r["status"] == 0 and f["n"] == r["kept"] >= 30
            if (word, p) == (0, 0):
                assert f["n"] == RS.SCENE_N[case]
            # every kept centre is a pixel whose s is exactly 0 for its own sample
            x0, y0, a = RR.axes(r["w"], r["h"])
            du = (f["px"].astype(np.float64) - x0) * a - f["u"]
            dv = (f["py"].astype(np.float64) - y0) * a - f["v"]
            assert np.count_nonzero((du * du + dv * dv) == 0.0) == f["n"]
            assert ((f["px"] >= 0) & (f["px"] < r["w"]) & (f["py"] >= 0) & (f["py"] < r["h"])).all()
            assert np.isfinite(r["bkg"]).all() and np.isfinite(r["sub"]).all() and np.isfinite(r["div"]).all()
            assert r["weights"][f["n"] + 1:].tolist() == [0.0] * (RR.MAX_SAMPLES - f["n"])
            # the spline follows the sky: after the subtraction the kept medians sit at the mean
            resid = r["bkg"][f["py"], f["px"]] - np.array([float(r["med"][k]) for k in range(len(r["keep"])) if r["keep"][k]])
            assert np.abs(resid).max() < 2e-3


def test_edge_cases_end_as_described():
    with pytest.raises(ValueError):
        RR.check(*RS.CAP_REFUSED, 1e9, 0.5)
    for word in (0, 1):
        r = RS.plane_reference(("cap", word))
        assert r["grid"]["K"] == 1023 and r["fit"]["n"] == 1023 and r["status"] == 0
        assert np.isfinite(r["sub"]).all()
        r = RS.plane_reference(("one", word))
        assert r["grid"]["K"] == 1 and r["fit"]["n"] == 1 and r["status"] == 0
        assert r["weights"][0] == 0.0 and not np.signbit(r["weights"][0])
        assert r["weights"][1] == float(r["med"][0]) == r["mean"]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            RR.check(131, 77, 10, 1.0, bad)
    out, info = RR.subsky_rbf_plane(np.zeros((30, 40), np.float32), 1, 1.0)
    assert info["status"] == 1 and info["fit"]["n"] == 0 and not out.any() and not info["weights"].any()


def test_descending_floor_of_the_solve():
    """The same system with the samples in the opposite order: the restatement's own rounding floor on b."""
    r = RS.plane_reference(("scene", "wide", 0, 0))
    f = r["fit"]
    g = RR.fit(r["med"], r["keep"], r["grid"], r["w"], r["h"], r["lam_rel"], descending=True)
    b2 = RR.background(g["x"], f["u"], f["v"], r["w"], r["h"])
    d = float(np.abs(b2 - r["bkg"]).max())
    print("descending floor on b: %.3g" % d)
    assert 0.0 < d < 1e-13


# ---- the parser ----
def test_parse_subsky_command():
    from siril_amd.background import parse_subsky_command as P
    c = P("subsky stack -rbf".split())
    assert (c.image, c.rbf, c.samples, c.tolerance, c.smooth, c.divide, c.out) == ("stack", True, 20, 1.0, 0.5, False, "")
    c = P("stack.fit -rbf -samples=30 -tolerance=2.5 -smooth=0.25 -nodither -divide -out=flat.fit".split())
    assert (c.image, c.rbf, c.samples, c.tolerance, c.smooth, c.divide, c.out) == \
        ("stack.fit", True, 30, 2.5, 0.25, True, "flat.fit")
    c = P("subsky stack 3 -samples=12".split())
    assert (c.rbf, c.degree, c.samples) == (False, 3, 12)
    for bad in ("subsky", "subsky -rbf", "subsky stack", "subsky stack 0", "subsky stack 5", "subsky stack two",
                "subsky stack 2 -smooth=0.5", "subsky stack -rbf -dither", "subsky stack -rbf -smooth=1.5",
                "subsky stack -rbf -smooth=-0.1", "subsky stack -rbf -smooth=nan", "subsky stack -rbf -smooth=x",
                "subsky stack -rbf -samples=0", "subsky stack -rbf -samples=1.5", "subsky stack -rbf -tolerance=-1",
                "subsky stack -rbf -tolerance=inf", "subsky stack -rbf -out=", "subsky stack -rbf -prefix=a_",
                "subsky stack -rbf 2", "subsky stack 2 -rbf", "subsky stack -rbf extra"):
        with pytest.raises(ValueError):
            P(bad.split())


def test_seqsubsky_still_refuses_rbf():
    from siril_amd.background import parse_seqsubsky_command
    with pytest.raises(ValueError):
        parse_seqsubsky_command("seqsubsky seq -rbf".split())
    with pytest.raises(ValueError):
        parse_seqsubsky_command("seqsubsky seq 1 -smooth=0.5".split())

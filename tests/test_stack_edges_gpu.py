"""GPU parity of the stack kernels at every capacity, real-slot bucket and
route boundary the dispatch has (sgpu_capi.cpp sorted_capacity / launch_exact,
stack_sorted_impl.h rs_pick, stack_sorted_gw.h), against the oracle.

Bar: the project's own -- result bit-equal, both rejection maps equal, the
totals equal, every pixel compared.  No tolerances.

  A  the bucket table itself, on the CPU (the one test here without a GPU)
  B  float SIGMA / PERCENTILE / median at both edges of every real-slot bucket
  C  the WINSORIZED moment path's prep kernel at NP = 256 and 512, every bound
  D  NP = 1024: every sorted type, float and 16-bit
  E  float kernels with G > 1 lanes per pixel on shifted / normalized frames
     and weight planes (XF = 1)
  F  the exact kernels with their scratch in global memory (N > 682)
  G  the means past N = 1024 (16-bit: u32 sums up to N = 65536)

The blocks are a few hundred pixels: more than one wave per lane-group shape
and a ragged last wave.  N is looped inside the tests.

Pixels answered by the exact kernel, as the tests print them (measured on an
MI355X; reported, the assertions are the routing conditions only): 0 in every
case of B, C and D (N = 65..1024, plain and XF = 1, float and 16-bit; D's
4 096-pixel WINSORIZED blocks included).  F, of 240 pixels at N = 700 / 1000:
float MAD 1 / 1 at sigma 3/3, 7 / 6 at 1/1, 36 / 38 at 0.5/2; 16-bit MAD 1, 2,
1 at both N; SIGMEDIAN 1/1 float 11 / 13, 16-bit 1 / 1 (the 1 is the column of
nulls only).
"""
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu          # (section A runs without one, so no module-wide mark)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN = 16                    # the tests' code for the median stack (method 1)


# --------------------------------------------------------------------------- A
# {NP: (G of the straight kernels, G of the loop types and the prep kernel)},
# the defaults of stack_sorted_gw.h
GW = {128: (1, 2), 256: (2, 4), 512: (4, 8), 1024: (8, 16)}


def rs_pick(E, G, N):
    """stack_sorted_impl.h rs_pick: the real-slot bound of a launch."""
    if E not in (64, 128):
        return E
    step = 4 if E == 64 else 8
    need = (N + G - 1) // G
    rs = (need + step - 1) // step * step
    return rs if rs < E else E


def bounds(E):
    """The compiled bounds (stack_sorted_rs*.hip), then E: the full network."""
    return list(range(36, 64, 4)) + [64] if E == 64 else list(range(72, 128, 8)) + [128]


def edge_ns(NP, G):
    """Per bucket of the kernels with G lanes per pixel at capacity NP: its
    lowest N (odd), the even one above, and the two highest (odd, even)."""
    E = NP // G
    step = 4 if E == 64 else 8
    out = []
    for rs in bounds(E):
        lo, hi = G * (rs - step) + 1, G * rs
        out += [lo, lo + 1, hi - 1, hi]
    return out


STRAIGHT_NS = {np_: edge_ns(np_, GW[np_][0]) for np_ in (128, 256, 512)}   # section B (E = 128)
PREP_NS = {np_: edge_ns(np_, GW[np_][1]) for np_ in (256, 512)}            # section C (E = 64)
NS_1024 = (513, 600, 1000, 1023, 1024)                                     # section D


def test_bucket_table(hostsim):
    """GW equals the defaults of stack_sorted_gw.h, the mirror of rs_pick
    equals the library's, and the N lists of sections B-D are, bucket by
    bucket, where a scan of rs_pick over the whole capacity changes its
    answer: a retune moves the edges and fails here."""
    import ctypes as C
    text = open(os.path.join(ROOT, "siril_amd", "csrc", "stack_sorted_gw.h")).read()
    parsed = {}
    for name, g in re.findall(r"#define SGPU_GW(\d+(?:_LOOP)?)\s+(\d+)\s*,\s*\d+", text):
        parsed[name] = int(g)
    assert {np_: (parsed[str(np_)], parsed[f"{np_}_LOOP"]) for np_ in GW} == GW
    hostsim.sim_rs_pick.restype = C.c_int
    hostsim.sim_rs_pick.argtypes = [C.c_int, C.c_int, C.c_int]
    for lists, col, E in ((STRAIGHT_NS, 0, 128), (PREP_NS, 1, 64)):
        for np_, ns in lists.items():
            G = GW[np_][col]
            assert np_ // G == E
            # scan: N in (NP / 2, NP] grouped by the bound the library picks
            groups = {}
            for n in range(np_ // 2 + 1, np_ + 1):
                rs = hostsim.sim_rs_pick(E, G, n)
                assert rs == rs_pick(E, G, n)
                groups.setdefault(rs, []).append(n)
            assert sorted(groups) == bounds(E)
            want = []
            for rs in bounds(E):
                g = groups[rs]
                assert g == list(range(g[0], g[-1] + 1)) and len(g) >= 4
                want += [g[0], g[1], g[-2], g[-1]]
                assert g[0] % 2 == 1 and g[-1] % 2 == 0          # odd lowest, even highest N
            assert ns == want, (np_, G)
            assert ns[0] == np_ // 2 + 1 and ns[-1] == np_
    # the median's selection network (G == 1 only) reads ranks N/2 - 1 and N/2
    assert GW[128][0] == 1
    assert STRAIGHT_NS[128][:4] == [65, 66, 71, 72] and STRAIGHT_NS[128][-8:-4] == [113, 114, 119, 120]
    assert PREP_NS[256][:4] == [129, 130, 143, 144] and PREP_NS[512][-4:] == [481, 482, 511, 512]
    # NP = 1024 (no pruned networks): the first N of the capacity and its last two
    assert NS_1024[0] == 512 + 1 and NS_1024[-2:] == (1023, 1024)


# ------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def ctx():
    from siril_amd import stacking
    c = stacking.Context(0)
    yield c
    c.close()


def _sig(rt):
    return (0.2, 0.1) if rt == 1 else ((0.32, 0.05) if rt == 7 else (3.0, 3.0))


def _args(rt, sig=None, **kw):
    from siril_amd import stacking as S
    if rt == MEDIAN:
        kw.pop("weights", None)
        return S.StackingArgs(S.Rejection(0), (3.0, 3.0), **kw)
    return S.StackingArgs(S.Rejection(rt), sig or _sig(rt), **kw)


def _frames(rng, n, h, w, zeros=0.02, outliers=0.03, wild=0.0):
    """test_stack_gpu.py's generator."""
    fr = (0.05 + 0.005 * rng.standard_normal((n, h, w))).astype(np.float32)
    m = rng.random(fr.shape) < outliers
    fr[m] += rng.uniform(0.2, 0.6, int(m.sum())).astype(np.float32)
    if wild:
        m = rng.random(fr.shape) < wild
        fr[m] = rng.uniform(0, 1, int(m.sum())).astype(np.float32)
    fr = np.clip(fr, 1e-6, 1).astype(np.float32)
    fr[rng.random(fr.shape) < zeros] = 0
    return fr


def _frames16(rng, n, h, w, zeros=0.02):
    """test_stack_gpu.py's 16-bit generator."""
    fr = (1500 + 40 * rng.standard_normal((n, h, w)))
    m = rng.random(fr.shape) < 0.03
    fr[m] += rng.uniform(3000, 20000, int(m.sum()))
    fr = np.clip(np.round(fr), 1, 65535).astype(np.uint16)
    fr[rng.random(fr.shape) < zeros] = 0
    return fr


def _planes(rng, shape, dzero=0.1, mzero=0.05):
    """test_stack_gpu.py's drizzle weights and feather-mask values."""
    d = rng.uniform(0.05, 1.0, shape).astype(np.float32)
    d[rng.random(shape) < dzero] = 0.0
    m = np.clip(rng.uniform(-0.2, 1.3, shape), 0, 1).astype(np.float32)
    m[rng.random(shape) < mzero] = 0.0
    return d, m


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _check(res, ref, rt, what):
    """Result bits, both rejection maps and the totals (the median stack has
    no rejection)."""
    out, rl, rh, counts = ref
    assert res.result.dtype == out.dtype, what
    bad = int((_bits(res.result) != _bits(out)).sum())
    assert bad == 0, f"{what}: {bad} of {out.size} pixels differ"
    if rt != MEDIAN:
        assert np.array_equal(res.rejmap_low, rl) and np.array_equal(res.rejmap_high, rh), what
        assert tuple(res.irej) == (int(counts[0]), int(counts[1])), what


def _stack(ctx, oracle, fr, rt, sig=None, what=None, out32=True, dx=None, norm=0, scale=None, offset=None,
           mul=None, weights=None, drizz=None, mask=None, output_norm=False):
    """One stack on the GPU and in the oracle, compared; returns the number of
    pixels the exact kernel answered."""
    from siril_amd import stacking as S
    sig = sig or _sig(rt)
    med = rt == MEDIAN
    kw = {}
    if dx is not None:
        kw["shiftx"] = S.shifts_from_registration(dx)
    if norm:
        kw.update(normalize=S.Normalization(norm), scale=scale, offset=offset, mul=mul)
    args = _args(rt, sig, weights=weights, output_norm=output_norm, **kw)
    okw = dict(method=1 if med else 0, output_norm=output_norm, norm=norm, scale=scale if norm else None,
               offset=offset if norm else None, mul=mul if norm else None, shift_dx=dx,
               weights=None if med else weights, nthreads=8)
    ort = 0 if med else rt
    if fr.dtype == np.uint16:
        res = ctx.stack(fr, args, 1 if med else 0, use_32bit_output=out32)
        exact = ctx.last_exact_pixels()
        ref = oracle.stack_rows_u16(fr, ort, sig, use_32bit_output=out32, **okw)
    else:
        res = ctx.stack(fr, args, 1 if med else 0, drizzle=drizz, mask=mask)
        exact = ctx.last_exact_pixels()
        ref = oracle.stack_rows(fr, ort, sig, drizz=drizz, mask=mask, **okw)
    _check(res, ref, rt, what)
    return exact


def _tables(rng, n, offset=0.01):
    """Per-frame normalization coefficients, registration shifts and weights."""
    return dict(scale=1.0 + 0.05 * rng.standard_normal(n), offset=offset * rng.standard_normal(n),
                mul=1.0 + 0.03 * rng.standard_normal(n)), rng.uniform(-5, 5, n), rng.uniform(0.5, 2.0, n)


# --------------------------------------------------------------------------- B
def _median_rows(rng, fr):
    """Two rows of columns that land on the ends of the median's rank window:
    row 1 strictly increasing in frame order, row 2 with the N/2 smallest
    values equal and the others distinct, so that ranks N/2 - 1 and N/2 differ
    (whole rows: a registration shift moves them onto themselves).  The other
    rows stay random: a network leaves sorted input alone, so a comparator
    pruned by mistake shows on those."""
    n = fr.shape[0]
    fr[:, 1, :] = (np.float32(0.1) + np.float32(0.5) * np.arange(n, dtype=np.float32) / np.float32(n))[:, None]
    col = np.full(n, 0.2, np.float32)
    col[n // 2:] = np.float32(0.3) + np.float32(0.4) * np.arange(1, n - n // 2 + 1, dtype=np.float32) / np.float32(n)
    assert len(np.unique(col)) == n - n // 2 + 1
    fr[:, 2, :] = rng.permutation(col)[:, None]


@gpu
@pytest.mark.parametrize("rt", [2, 1, MEDIAN], ids=["sigma", "percentile", "median"])
@pytest.mark.parametrize("np_", [128, 256, 512])
def test_straight_real_slot_edges(ctx, oracle, np_, rt):
    """Float SIGMA, PERCENTILE and the median on the pruned sort networks
    (stack_sorted_rs*.hip) and the full one, at the lowest two and highest
    two N of every bucket: the gather's FMIN, the networks' RS and the
    median's rank window [LO, HI) are right only if both edges are.  Plain and
    with integer registration shifts (the XF = 1 variants)."""
    npix = 5 * 72
    line = []
    for n in STRAIGHT_NS[np_]:
        rng = np.random.default_rng(10000 * rt + n)
        fr = _frames(rng, n, 5, 72)
        if rt == MEDIAN:
            _median_rows(rng, fr)
        dx = rng.uniform(-5, 5, n)
        for shift in (None, dx):
            exact = _stack(ctx, oracle, fr, rt, dx=shift, what=f"NP={np_} rt={rt} N={n} shift={shift is not None}")
            if rt != MEDIAN:
                assert exact < npix // 2, (n, exact)
            line.append(f"{n}:{exact}")
    print(f"B NP={np_} rt={rt} exact pixels of {npix} (plain, shifted): " + " ".join(line))


# --------------------------------------------------------------------------- C
@gpu
@pytest.mark.parametrize("np_", [256, 512])
def test_winsorized_prep_bounds(ctx, oracle, np_):
    """The moment path's prep kernel with 4 (NP = 256) and 8 (NP = 512) lanes
    per pixel at every real-slot bound 36..60 and the full network, both edges
    of each: plain, and the shifted variant with -norm=addscale and weights."""
    npix = 6 * 64
    line = []
    for n in PREP_NS[np_]:
        rng = np.random.default_rng(20000 + n)
        fr = _frames(rng, n, 6, 64)
        t, dx, weights = _tables(rng, n)
        a = _stack(ctx, oracle, fr, 5, what=f"N={n} plain")
        assert a < npix // 2, (n, a)
        b = _stack(ctx, oracle, fr, 5, dx=dx, norm=3, weights=weights, what=f"N={n} shifts addscale weights", **t)
        assert b < npix // 2, (n, b)
        line.append(f"{n}:{a},{b}")
    print(f"C NP={np_} exact pixels of {npix} (plain, shifted + normalized + weighted): " + " ".join(line))


# --------------------------------------------------------------------------- D
@gpu
@pytest.mark.parametrize("rt", [1, 2, 3, 4, 5, MEDIAN])
def test_np1024_float(ctx, oracle, rt):
    """stack_sorted_np1024.hip, float: G = 8 straight kernels (PERCENTILE,
    SIGMA, median) and G = 16 loop kernels (MAD, SIGMEDIAN, WINSORIZED with
    its moment path) from the first N of the capacity to the last; plain, and
    with shifts, -norm=addscale and frame weights."""
    npix = 4 * 80
    line = []
    for n in NS_1024:
        rng = np.random.default_rng(30000 + 10 * rt + n)
        fr = _frames(rng, n, 4, 80)
        t, dx, weights = _tables(rng, n)
        a = _stack(ctx, oracle, fr, rt, what=f"rt={rt} N={n} plain")
        b = _stack(ctx, oracle, fr, rt, dx=dx, norm=3, weights=weights, what=f"rt={rt} N={n} XF", **t)
        assert a < npix // 2 and b < npix // 2, (rt, n, a, b)
        line.append(f"{n}:{a},{b}")
    print(f"D float rt={rt} exact pixels of {npix} (plain, shifted + normalized + weighted): " + " ".join(line))


@gpu
@pytest.mark.parametrize("rt", [1, 2, 3, 4, 5, MEDIAN])
def test_np1024_u16(ctx, oracle, rt):
    """stack_sorted_np1024.hip, 16-bit: the six kernels, float and 16-bit
    output; plain, and with -norm=add and frame weights."""
    npix = 4 * 80
    line = []
    for n in NS_1024:
        rng = np.random.default_rng(31000 + 10 * rt + n)
        fr = _frames16(rng, n, 4, 80)
        t, _, _ = _tables(rng, n, offset=60)
        weights = rng.uniform(0.5, 1.5, n)
        for out32 in (True, False):
            a = _stack(ctx, oracle, fr, rt, out32=out32, what=f"rt={rt} N={n} out32={out32} plain")
            b = _stack(ctx, oracle, fr, rt, out32=out32, norm=1, weights=weights,
                       what=f"rt={rt} N={n} out32={out32} norm weights", **t)
            assert a < npix // 2 and b < npix // 2, (rt, n, out32, a, b)
        line.append(f"{n}:{a},{b}")
    print(f"D u16 rt={rt} exact pixels of {npix} (plain, normalized + weighted; 16-bit output): " + " ".join(line))


@gpu
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_np1024_winsorized_chunk(ctx, oracle, u16):
    """WINSORIZED at N = 1000 over 4 096 pixels: the moment path's records of
    R = NP / 2 + 16 slots and its chunking over several waves."""
    rng = np.random.default_rng(32000 + u16)
    fr = (_frames16 if u16 else _frames)(rng, 1000, 16, 256)
    exact = _stack(ctx, oracle, fr, 5, what=f"winsorized N=1000 u16={u16}")
    print(f"D winsorized N=1000 u16={u16}: exact pixels {exact} of {16 * 256}")
    assert exact < 16 * 256 // 2


# --------------------------------------------------------------------------- E
@gpu
@pytest.mark.parametrize("rt", [1, 2, 3, 4, 5, MEDIAN])
def test_float_xf_lane_groups(ctx, oracle, rt):
    """Float kernels with G = 2..8 lanes per pixel (NP = 256, 512) on shifted
    and normalized frames: the gather's per-lane table index fe = min(e * G +
    g, N - 1) and `outside` test; every -norm= form with scale, offset and
    mul, and frame weights alone and on shifted frames."""
    for n in (129, 200, 300):
        rng = np.random.default_rng(40000 + 10 * rt + n)
        fr = _frames(rng, n, 6, 72)
        t, dx, weights = _tables(rng, n)
        for norm in (1, 2, 3, 4):
            _stack(ctx, oracle, fr, rt, dx=dx, norm=norm, what=f"rt={rt} N={n} norm={norm} shifts", **t)
        if rt != MEDIAN:
            _stack(ctx, oracle, fr, rt, weights=weights, what=f"rt={rt} N={n} weights")
            _stack(ctx, oracle, fr, rt, weights=weights, dx=dx, what=f"rt={rt} N={n} weights shifts")


@gpu
@pytest.mark.parametrize("rt", [2, 5])
def test_float_planes_lane_groups(ctx, oracle, rt):
    """Drizzle and feather-mask planes on the G > 1 float kernels (the
    gather's drizzle null per lane, the weighted mean from the cross-lane
    result): each plane alone, both, and both with weights and -norm=addscale."""
    for n in (129, 200, 300):
        rng = np.random.default_rng(41000 + 10 * rt + n)
        fr = _frames(rng, n, 6, 72)
        d, m = _planes(rng, fr.shape)
        t, dx, weights = _tables(rng, n)
        _stack(ctx, oracle, fr, rt, dx=dx, drizz=d, what=f"rt={rt} N={n} drizzle")
        _stack(ctx, oracle, fr, rt, dx=dx, mask=m, what=f"rt={rt} N={n} mask")
        _stack(ctx, oracle, fr, rt, dx=dx, drizz=d, mask=m, what=f"rt={rt} N={n} both planes")
        _stack(ctx, oracle, fr, rt, dx=dx, drizz=d, mask=m, weights=weights, norm=3,
               what=f"rt={rt} N={n} both planes weights addscale", **t)


# --------------------------------------------------------------------------- F
@gpu
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("rt", [6, 7], ids=["linearfit", "gesdt"])
def test_exact_global_scratch_every_pixel(ctx, oracle, rt, u16):
    """LINEARFIT and GESDT above N = 128 run on the exact kernel alone; above
    N = 682 its scratch (6 N words a thread) is in global memory
    (k_stack_exact / k_stack_exact16, sized by exact_threads)."""
    for n in (700, 1024):
        rng = np.random.default_rng(50000 + 10 * rt + n)
        fr = (_frames16 if u16 else _frames)(rng, n, 2, 64)
        exact = _stack(ctx, oracle, fr, rt, what=f"rt={rt} N={n} u16={u16}")
        assert exact == 2 * 64, (n, exact)


def _stress_cols(rng, n, cols):
    """test_stack_gpu.py's _stress_frames: columns whose f64 sums are not
    exact (negative values, samples within a few ulp of the mean, 1e-20
    levels, 1e6 outliers), which the sorted kernels' sum-order guard defers."""
    kind = rng.integers(0, 4, cols)
    lvl = np.where(kind == 0, 1e-3, np.where(kind == 1, 0.05, np.where(kind == 2, 1e-20, 3.0)))
    spread = np.where(kind == 3, 1e-6, 0.1) * lvl
    x = lvl[None, :] + spread[None, :] * rng.standard_normal((n, cols))
    x -= np.where(kind == 0, 1.1e-3, 0.0)[None, :]
    m = rng.random(x.shape) < 0.04
    x[m] += (rng.uniform(2, 8, int(m.sum())) * np.broadcast_to(np.abs(lvl)[None, :], x.shape)[m])
    big = rng.random(x.shape) < 0.002
    x[big] *= 1e6
    x = x.astype(np.float32)
    x[rng.random(x.shape) < 0.01] = 0
    return x


def _tie_frames(rng, n, u16):
    """test_mad_quantized_ties' data: quantized samples, constant columns and
    columns of two levels; a column of nulls only (kept == 0: deferred in
    every case), and in float a row of columns with inexact sums."""
    if u16:
        fr = _frames16(rng, n, 6, 40)
        fr = np.where(fr == 0, 0, np.maximum(fr // 32 * 32, 32)).astype(np.uint16)
        fr[:, 0, :8] = 16000
        fr[:, 1, :8] = np.where(np.arange(n)[:, None] % 2 == 0, 16000, 32000)
    else:
        fr = _frames(rng, n, 6, 40, wild=0.1)
        fr = (np.round(fr * 64) / 64).astype(np.float32)
        fr[:, 0, :8] = np.float32(0.25)
        fr[:, 1, :8] = np.where(np.arange(n)[:, None] % 2 == 0, 0.25, 0.5).astype(np.float32)
        fr[:, 3, :] = _stress_cols(rng, n, 40)
    fr[:, 2, 5] = 0
    return fr


@gpu
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_exact_global_scratch_mad_deferred(ctx, oracle, u16):
    """MAD columns the sorted kernels (NP = 1024) defer, at N > 682: the
    global-scratch exact kernel over a deferred list."""
    for n in (700, 1000):
        fr = _tie_frames(np.random.default_rng(51000 + n), n, u16)
        for sig in ((3.0, 3.0), (1.0, 1.0), (0.5, 2.0)):
            exact = _stack(ctx, oracle, fr, 3, sig=sig, output_norm=not u16, what=f"MAD N={n} sig={sig} u16={u16}")
            print(f"F MAD N={n} sig={sig} u16={u16}: exact pixels {exact} of {fr[0].size}")
            assert 0 < exact


@gpu
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_exact_global_scratch_sigmedian_deferred(ctx, oracle, u16):
    """SIGMEDIAN at sigma 1 / 1 on columns with 20 % wild samples, N > 682.
    (Measured: at these N the sorted kernel defers none of the wild columns,
    its iteration cap and sum-order guard never fire on them.  What it defers
    is a column of nulls only and, in float, columns with inexact sums.)"""
    for n in (700, 1000):
        rng = np.random.default_rng(52000 + n)
        fr = _frames(rng, n, 6, 40, wild=0.2)
        if u16:
            fr = np.round(fr * 65535).astype(np.uint16)
        else:
            fr[:, 3, :] = _stress_cols(rng, n, 40)
        fr[:, 2, 5] = 0
        exact = _stack(ctx, oracle, fr, 4, sig=(1.0, 1.0), output_norm=not u16, what=f"SIGMEDIAN N={n} u16={u16}")
        print(f"F SIGMEDIAN N={n} u16={u16}: exact pixels {exact} of {fr[0].size}")
        assert 0 < exact


@gpu
@pytest.mark.parametrize("rt,u16", [(2, False), (5, False), (MEDIAN, False), (2, True), (MEDIAN, True)],
                         ids=["sigma-f32", "winsorized-f32", "median-f32", "sigma-u16", "median-u16"])
def test_exact_past_sorted_capacity(ctx, oracle, rt, u16):
    """N > 1024: no sorted kernel, every pixel on the global-scratch exact
    kernel.  Columns of one repeated sample (nulls only, a saturated level,
    -0.0) take quickmedian_value's answer where only the median's value is
    used (kept == 0, the median stack)."""
    for n in (1025, 1500):
        rng = np.random.default_rng(53000 + 10 * rt + n)
        fr = (_frames16 if u16 else _frames)(rng, n, 2, 64)
        fr[:, 0, 0] = 0
        fr[:, 0, 1] = 65535 if u16 else 0.25
        if not u16:
            fr[:, 0, 2] = -0.0
            fr[:, 0, 3] = -0.0
            fr[0, 0, 3] = 0.0                       # +0 then -0: not one bit pattern
        exact = _stack(ctx, oracle, fr, rt, what=f"rt={rt} N={n} u16={u16}")
        assert exact == 2 * 64, (n, exact)


# --------------------------------------------------------------------------- G
@gpu
@pytest.mark.parametrize("n", [1025, 4000])
def test_mean_u16_past_1024(ctx, oracle, n):
    """16-bit mean on the streaming kernel past the sorted capacity: plain,
    -norm=addscale and frame weights, float and 16-bit output."""
    rng = np.random.default_rng(60000 + n)
    fr = _frames16(rng, n, 5, 27)
    fr[:, 2, 3] = 0
    t, _, _ = _tables(rng, n, offset=60)
    weights = rng.uniform(0.5, 1.5, n)
    for out32 in (True, False):
        exact = _stack(ctx, oracle, fr, 0, out32=out32, what=f"N={n} out32={out32} plain")
        assert exact <= 1, exact                       # the all-null column alone
        _stack(ctx, oracle, fr, 0, out32=out32, norm=3, what=f"N={n} out32={out32} addscale", **t)
        _stack(ctx, oracle, fr, 0, out32=out32, weights=weights, what=f"N={n} out32={out32} weights")


@gpu
def test_mean_u16_sum_limit(ctx, oracle):
    """N = 65536, the streaming kernel's last N: a column of 65535 in every
    frame (u32 sum 65536 * 65535 = 2^32 - 65536) and one of nulls only.
    N = 65537 is the first on the sequential kernel.  The column of nulls
    goes to the exact kernel at both N (kept == 0: the median of the stack);
    before quickmedian_value (stack_exact.hip) its Lomuto partition took
    N^2 / 2 steps there and this test 412 s instead of 1.4 s."""
    rng = np.random.default_rng(61000)
    fr = _frames16(rng, 65537, 1, 64)
    fr[:, 0, 7] = 65535
    fr[:, 0, 9] = 0
    for out32 in (True, False):
        exact = _stack(ctx, oracle, fr[:65536], 0, out32=out32, what=f"N=65536 out32={out32}")
        assert exact <= 1, exact
    exact = _stack(ctx, oracle, fr, 0, what="N=65537")
    assert exact == 64, exact


@gpu
@pytest.mark.parametrize("shape", [(24, 40), (7, 33)], ids=["vec", "ragged"])
@pytest.mark.parametrize("n", [1025, 4000])
def test_mean_float_past_1024(ctx, oracle, n, shape):
    """Float mean past N = 257 (16-byte and per-pixel paths): plain, and with
    shifts and -norm=addscale."""
    rng = np.random.default_rng(62000 + n + shape[0])
    fr = _frames(rng, n, *shape)
    fr[:, 1, 3] = 0.0
    t, dx, _ = _tables(rng, n)
    _stack(ctx, oracle, fr, 0, what=f"N={n} {shape} plain")
    _stack(ctx, oracle, fr, 0, dx=dx, norm=3, what=f"N={n} {shape} shifts addscale", **t)

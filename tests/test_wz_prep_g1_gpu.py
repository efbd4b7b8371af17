"""One lane per pixel in the float WINSORIZED prep kernel at N <= 128
(k_stack_wz_prep1, stack_wz.h; stack_sorted_gw.h SGPU_WZ_PREP_W128_G1): every
GPU case bit for bit against the oracle on result bits, both rejection maps
and the totals.

The kernel has two paths per wave.  A wave whose 64 pixels all hold at least
rs - 7 samples (rs: the real-slot bound of the launch, rs_pick_prep1) stores
its ranks from compile-time slot ranges; a wave with a pixel below that takes
run-time slot loops.  `_frames` (4 % nulls) puts a pixel below the bound into
nearly every wave, `_full_frames` (no null at all) keeps every wave on the
compile-time ranges.  N covers the ends of the capacity (65, 128), the
benchmark's 100 and both sides of every bound (72, 80, .. 120).  Frames are
N x 5 x 203: 1 015 pixels, no multiple of the 64 pixels of a wave, so the last
wave is partial.

The one test without a GPU checks the picker's table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu          # (test_picker runs without one, so no module-wide mark)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [65, 72, 73, 80, 81, 88, 89, 96, 97, 100, 104, 105, 112, 113, 120, 121, 128]
SIGMAS = ((3.0, 3.0), (1.0, 1.0))


def rs_pick_prep1(n):
    """stack_sorted_rs128.hip rs_pick_prep1: N rounded up to the step of 8,
    from 72 (the first compiled bound) to 128 (the full network)."""
    return min(128, max(72, (n + 7) // 8 * 8))


def test_picker(hostsim):
    """The mirror above against the library's rs_pick at E = 128, G = 1 (what
    rs_pick_prep1 returns for N = 65..128), the bounds against the ones
    stack_sorted_rs128.hip compiles, and what the kernel's compile-time slot
    ranges rest on: N in [rs - 7, rs]."""
    import ctypes as C
    import re
    hostsim.sim_rs_pick.restype = C.c_int
    hostsim.sim_rs_pick.argtypes = [C.c_int, C.c_int, C.c_int]
    text = open(os.path.join(ROOT, "siril_amd", "csrc", "stack_sorted_rs128.hip")).read()
    first = int(re.search(r"prep1<SGPU_WZ_PREP_W128_G1, (\d+)>", text).group(1))
    step = int(re.search(r"return prep1<W, RS \+ (\d+)>", text).group(1))
    compiled = list(range(first, 128, step)) + [128]
    seen = set()
    for n in range(65, 129):
        rs = rs_pick_prep1(n)
        assert rs == hostsim.sim_rs_pick(128, 1, n)
        assert rs in compiled and rs - 7 <= n <= rs
        seen.add(rs)
    assert sorted(seen) == compiled
    # the N list of the GPU cases: the lowest and the highest N of every bucket
    assert {n for rs in compiled for n in (rs - 7, rs)} <= set(NS)


@pytest.fixture(scope="module")
def ctx():
    from siril_amd import stacking
    c = stacking.Context(0)
    yield c
    c.close()


def _args(sig, **kw):
    from siril_amd import stacking as S
    return S.StackingArgs(S.Rejection.WINSORIZED, sig, **kw)


def _check(res, ref):
    out, rl, rh, counts = ref
    assert np.array_equal(res.result.view(np.uint32), out.view(np.uint32)), \
        f"{int((res.result.view(np.uint32) != out.view(np.uint32)).sum())} pixels differ"
    assert np.array_equal(res.rejmap_low, rl) and np.array_equal(res.rejmap_high, rh)
    assert tuple(res.irej) == (int(counts[0]), int(counts[1]))


def _full_frames(n, rows, w, seed):
    """synth frames, every sample present (no null: kept == N in every lane),
    with eight columns of five levels."""
    from siril_amd import synth
    fr = synth.frames_numpy(n, rows, w, seed=seed)
    rng = np.random.default_rng(seed)
    fr[fr == 0.0] = np.float32(0.25)
    levels = np.float32(0.1) + np.float32(0.01) * rng.integers(0, 5, (n, 8)).astype(np.float32)
    fr[:, 2, 40:48] = levels                 # heavy ties
    return fr


def _frames(n, rows, w, seed):
    """the same with 4 % null samples (kept differs inside a wave, kmin < N),
    a column of nulls only and one with a NaN."""
    fr = _full_frames(n, rows, w, seed)
    rng = np.random.default_rng(seed + 1)
    fr[rng.random(fr.shape) < 0.04] = 0.0
    fr[:, 1, 7] = 0.0                        # kept == 0: the exact kernel's
    fr[n // 2, 3, 9] = np.nan
    return fr


@gpu
@pytest.mark.parametrize("n", NS)
def test_columns(ctx, oracle, n):
    fr = _frames(n, 5, 203, seed=400 + n)
    for sig in SIGMAS:
        res = ctx.stack(fr, _args(sig))
        exact = ctx.last_exact_pixels()
        print(f"N={n} sig={sig} exact={exact} deferred={ctx.last_wz_deferred()}")
        _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8))
        assert exact >= 1, "the all-null column goes to the exact kernel"


@gpu
@pytest.mark.parametrize("n", NS)
def test_full_sample_waves(ctx, oracle, n):
    """No null anywhere: every wave stores from the compile-time slot ranges."""
    fr = _full_frames(n, 5, 203, seed=500 + n)
    assert np.count_nonzero(fr == 0.0) == 0 and np.isfinite(fr).all()
    for sig in SIGMAS:
        res = ctx.stack(fr, _args(sig))
        print(f"N={n} sig={sig} exact={ctx.last_exact_pixels()} deferred={ctx.last_wz_deferred()}")
        _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8))


@pytest.fixture(scope="module")
def frames100():
    fr = _frames(100, 8, 1000, seed=9)
    fr.setflags(write=False)
    return fr


@gpu
def test_moment_path_ran(ctx, oracle, frames100):
    """100 x 8 x 1000 at sigma 3/3: deferrals to the tail passes show that the
    rounds ran on the prep's records."""
    res = ctx.stack(frames100, _args((3.0, 3.0)))
    d = ctx.last_wz_deferred()
    print("deferred", d, "exact", ctx.last_exact_pixels())
    _check(res, oracle.stack_rows(frames100, oracle.WINSORIZED, (3.0, 3.0), nthreads=8))
    assert d[0] > 0


@gpu
@pytest.mark.parametrize("n", [81, 100, 128])
def test_weights(ctx, oracle, n):
    """Weighted means on the one-lane prep's records."""
    rng = np.random.default_rng(n)
    weights = rng.uniform(0.5, 2.0, n)
    for fr in (_frames(n, 5, 203, seed=700 + n), _full_frames(n, 5, 203, seed=800 + n)):
        for sig in SIGMAS:
            _check(ctx.stack(fr, _args(sig, weights=weights)),
                   oracle.stack_rows(fr, oracle.WINSORIZED, sig, weights=weights, nthreads=8))


@gpu
@pytest.mark.parametrize("n", [81, 100, 128])
def test_shifts_addscale(ctx, oracle, n):
    """The shifted prep variant (XF = 1 runs one lane per pixel too: integer
    x-shifts, -norm=addscale coefficients), alone and with weights; the
    shifts null the samples of a frame's border, so `kept` differs inside
    the waves at the left and right edges of the full-sample frames as well."""
    from siril_amd import stacking as S
    rng = np.random.default_rng(n)
    scale = 1.0 + 0.05 * rng.standard_normal(n)
    offset = 0.01 * rng.standard_normal(n)
    mul = 1.0 + 0.03 * rng.standard_normal(n)
    dx = rng.uniform(-6, 6, n)
    weights = rng.uniform(0.5, 2.0, n)
    for fr in (_frames(n, 5, 203, seed=900 + n), _full_frames(n, 5, 203, seed=950 + n)):
        for sig in SIGMAS:
            args = _args(sig, normalize=S.Normalization.ADDITIVE_SCALING, scale=scale, offset=offset, mul=mul,
                         shiftx=S.shifts_from_registration(dx))
            _check(ctx.stack(fr, args),
                   oracle.stack_rows(fr, oracle.WINSORIZED, sig, norm=3, scale=scale, offset=offset, mul=mul,
                                     shift_dx=dx, nthreads=8))
            _check(ctx.stack(fr, _args(sig, weights=weights, shiftx=S.shifts_from_registration(dx))),
                   oracle.stack_rows(fr, oracle.WINSORIZED, sig, weights=weights, shift_dx=dx, nthreads=8))


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from siril_amd import stacking as S
fr = np.load(sys.argv[2])
ctx = S.Context(0)
res = ctx.stack(fr, S.StackingArgs(S.Rejection.WINSORIZED, (3.0, 3.0)))
d = ctx.last_wz_deferred()
np.savez(sys.argv[3], result=res.result, rl=res.rejmap_low, rh=res.rejmap_high, irej=np.array(res.irej, np.int64))
ctx.close()
print(json.dumps({"deferred": list(d)}))
"""


@gpu
def test_many_small_chunks(oracle, frames100, tmp_path):
    """SGPU_WZ_CHUNK=1024 on 8 000 pixels: eight chunks, so both workspace
    buffers are refilled by the prep three times (the knob is read once per
    process: a fresh child)."""
    fin, fout = str(tmp_path / "in.npy"), str(tmp_path / "out.npz")
    np.save(fin, frames100)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], env=dict(os.environ, SGPU_WZ_CHUNK="1024"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["deferred"][0] > 0
    a = np.load(fout)
    out, rl, rh, counts = oracle.stack_rows(frames100, oracle.WINSORIZED, (3.0, 3.0), nthreads=8)
    assert np.array_equal(a["result"].view(np.uint32), out.view(np.uint32))
    assert np.array_equal(a["rl"], rl) and np.array_equal(a["rh"], rh)
    assert tuple(a["irej"]) == (int(counts[0]), int(counts[1]))

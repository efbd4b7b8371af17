"""Oracle parity of the float WINSORIZED moment path's default launch at N =
65..128: every case bit for bit against the oracle on result bits, both
rejection maps and the totals.  (Written for a prep kernel with four lanes per
pixel, since removed; the file keeps its name and its cases, which the
one-lane prep and the fused kernel now answer.)

N covers the ends of the capacity (65, 128), the benchmark's 100 and both
sides of every multiple of 16 and of 8 between them that a prep kernel has had
a real-slot bound at (N = 4b and 4b + 1 for b = 20, 24, 26, 28; 65, 81, 97,
105 and 113 are the lowest N of those buckets).  Frames are N x 5 x 203: 1 015
pixels, no multiple of the 64 pixels of a wave, so the last wave has dead
lanes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [65, 80, 81, 96, 97, 100, 104, 105, 112, 113, 128]


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


def _frames(n, rows, w, seed):
    """synth frames with 4 % null samples (kept differs inside a wave, kmin <
    N), a column of nulls only, one with a NaN and eight columns of five levels."""
    from siril_amd import synth
    fr = synth.frames_numpy(n, rows, w, seed=seed)
    rng = np.random.default_rng(seed)
    fr[rng.random(fr.shape) < 0.04] = 0.0
    levels = np.float32(0.1) + np.float32(0.01) * rng.integers(0, 5, (n, 8)).astype(np.float32)
    fr[:, 2, 40:48] = levels                 # heavy ties
    fr[:, 1, 7] = 0.0                        # kept == 0: the exact kernel's
    fr[n // 2, 3, 9] = np.nan
    return fr


@pytest.mark.parametrize("n", NS)
def test_columns(ctx, oracle, n):
    fr = _frames(n, 5, 203, seed=400 + n)
    for sig in ((3.0, 3.0), (1.0, 1.0)):
        res = ctx.stack(fr, _args(sig))
        exact = ctx.last_exact_pixels()
        print(f"N={n} sig={sig} exact={exact} deferred={ctx.last_wz_deferred()}")
        _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8))
        assert exact >= 1, "the all-null column goes to the exact kernel"


@pytest.fixture(scope="module")
def frames100():
    fr = _frames(100, 8, 1000, seed=9)
    fr.setflags(write=False)
    return fr


def test_moment_path_ran(ctx, oracle, frames100):
    """100 x 8 x 1000: at sigma 3/3 deferrals to the tail passes show that
    the rounds ran on the prep's records (at 1/1 the rounds end or fall back
    before the head's cap: nothing is deferred there)."""
    for sig in ((3.0, 3.0), (1.0, 1.0)):
        res = ctx.stack(frames100, _args(sig))
        d = ctx.last_wz_deferred()
        print("sig", sig, "deferred", d, "exact", ctx.last_exact_pixels())
        _check(res, oracle.stack_rows(frames100, oracle.WINSORIZED, sig, nthreads=8))
        assert d[0] > 0 or sig != (3.0, 3.0)


@pytest.mark.parametrize("n", [81, 100, 128])
def test_shifts_addscale_weights(ctx, oracle, n):
    """The shifted prep variant (integer x-shifts, -norm=addscale
    coefficients) and weighted means."""
    from siril_amd import stacking as S
    fr = _frames(n, 5, 203, seed=700 + n)
    rng = np.random.default_rng(n)
    scale = 1.0 + 0.05 * rng.standard_normal(n)
    offset = 0.01 * rng.standard_normal(n)
    mul = 1.0 + 0.03 * rng.standard_normal(n)
    dx = rng.uniform(-6, 6, n)
    weights = rng.uniform(0.5, 2.0, n)
    for sig in ((3.0, 3.0), (1.0, 1.0)):
        args = _args(sig, normalize=S.Normalization.ADDITIVE_SCALING, scale=scale, offset=offset, mul=mul,
                     shiftx=S.shifts_from_registration(dx))
        _check(ctx.stack(fr, args),
               oracle.stack_rows(fr, oracle.WINSORIZED, sig, norm=3, scale=scale, offset=offset, mul=mul, shift_dx=dx,
                                 nthreads=8))
        _check(ctx.stack(fr, _args(sig, weights=weights)),
               oracle.stack_rows(fr, oracle.WINSORIZED, sig, weights=weights, nthreads=8))
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

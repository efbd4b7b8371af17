"""Split rounds of the float WINSORIZED moment path at N <= 128 (stack_wz.h:
k_stack_wz_rounds_lds with a rounds cap, k_stack_wz_tail over the striped
deferral lists): every case bit for bit against the oracle on result bits,
both rejection maps and the totals, with the deferral counters showing that
the tail passes really ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def frames100():
    """100 x 8 x 1000: 8 000 pixels = 125 waves, a row width that is no
    multiple of 64.  Shared, never modified."""
    from siril_amd import synth
    fr = synth.frames_numpy(100, 8, 1000)
    fr.setflags(write=False)
    return fr


def test_small_frames_sigma3(ctx, oracle, frames100):
    """Case A: the bench recipe at sigma 3/3; some pixels need a third round."""
    res = ctx.stack(frames100, _args((3.0, 3.0)))
    d = ctx.last_wz_deferred()
    print("deferred", d)
    _check(res, oracle.stack_rows(frames100, oracle.WINSORIZED, (3.0, 3.0), nthreads=8))
    assert d[0] > 0


def test_partial_last_wave(ctx, oracle, frames100):
    """Case A, a partial last wave: 7 990 pixels (124 waves and 54 lanes)."""
    fr = np.ascontiguousarray(frames100.reshape(100, -1)[:, :7990].reshape(100, 10, 799))
    res = ctx.stack(fr, _args((3.0, 3.0)))
    d = ctx.last_wz_deferred()
    _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, (3.0, 3.0), nthreads=8))
    assert d[0] > 0


def test_two_deferrals(ctx, oracle, frames100):
    """Case B: N = 70 at sigma 2/2 -- many pixels are still going after four
    rounds, so the second tail pass runs."""
    fr = np.ascontiguousarray(frames100[:70])
    res = ctx.stack(fr, _args((2.0, 2.0)))
    d = ctx.last_wz_deferred()
    print("deferred", d)
    _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, (2.0, 2.0), nthreads=8))
    assert d[0] > 0 and d[1] > 0
    assert d[1] <= d[0] <= fr.shape[1] * fr.shape[2]


@pytest.mark.parametrize("n", [65, 128])
def test_edge_columns(ctx, oracle, n):
    """Case C: the ends of the capacity (N = 65, 128) on a 4 x 300 frame with
    20 % zeros and constant / single-sample columns next to deferred ones."""
    from siril_amd import synth
    fr = synth.frames_numpy(n, 4, 300, seed=77 + n)
    rng = np.random.default_rng(n)
    fr[rng.random(fr.shape) < 0.2] = 0.0
    fr[:, 0, :6] = np.float32(0.25)          # constant columns
    fr[:n - 1, 1, 3] = 0.0                   # kept == 1
    fr[:, 1, 4] = 0.0                        # kept == 0
    for sig in ((3.0, 3.0), (2.0, 2.0)):
        res = ctx.stack(fr, _args(sig))
        d = ctx.last_wz_deferred()
        _check(res, oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8))
        assert d[0] > 0, (n, sig)


def test_weights_and_shifts(ctx, oracle, frames100):
    """Case D: the tail writes through weighted_mean; the prep runs its shifted variant."""
    from siril_amd import stacking as S
    rng = np.random.default_rng(12)
    n = frames100.shape[0]
    weights = rng.uniform(0.5, 2.0, n)
    res = ctx.stack(frames100, _args((3.0, 3.0), weights=weights))
    assert ctx.last_wz_deferred()[0] > 0
    _check(res, oracle.stack_rows(frames100, oracle.WINSORIZED, (3.0, 3.0), weights=weights, nthreads=8))
    dx = rng.uniform(-6, 6, n)
    res = ctx.stack(frames100, _args((3.0, 3.0), shiftx=S.shifts_from_registration(dx)))
    assert ctx.last_wz_deferred()[0] > 0
    _check(res, oracle.stack_rows(frames100, oracle.WINSORIZED, (3.0, 3.0), shift_dx=dx, nthreads=8))


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from siril_amd import stacking as S, synth
fr = synth.frames_numpy(100, 48, 512, seed=31)
ctx = S.Context(0)
res = ctx.stack(fr, S.StackingArgs(S.Rejection.WINSORIZED, (3.0, 3.0)))
d = ctx.last_wz_deferred()
np.savez(sys.argv[2], result=res.result, rl=res.rejmap_low, rh=res.rejmap_high, irej=np.array(res.irej, np.int64))
ctx.close()
print(json.dumps({"deferred": list(d)}))
"""


def test_many_small_chunks(oracle, tmp_path):
    """Case E: SGPU_WZ_CHUNK=4096 on 100 x 48 x 512 gives 6 chunks: both
    workspace buffers are reused twice and every chunk's fallback tails follow
    its split's appends.  The knobs are read once per process, so the split
    and SGPU_WZ_SPLIT=0 each run in a fresh child on the same frames; the two
    outputs are compared with each other and with the oracle."""
    from siril_amd import synth
    outs = {}
    for split in ("2", "0"):
        env = dict(os.environ, SGPU_WZ_CHUNK="4096", SGPU_WZ_SPLIT=split)
        f = str(tmp_path / f"split{split}.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, f], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])["deferred"]
        print("split", split, "deferred", d)
        assert (d[0] > 0) == (split != "0")
        outs[split] = np.load(f)
    a, b = outs["2"], outs["0"]
    for key in ("result", "rl", "rh", "irej"):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    fr = synth.frames_numpy(100, 48, 512, seed=31)
    out, rl, rh, counts = oracle.stack_rows(fr, oracle.WINSORIZED, (3.0, 3.0), nthreads=8)
    assert np.array_equal(a["result"].view(np.uint32), out.view(np.uint32))
    assert np.array_equal(a["rl"], rl) and np.array_equal(a["rh"], rh)
    assert tuple(a["irej"]) == (int(counts[0]), int(counts[1]))

"""Straight-line clamp walks of the WINSORIZED moment path (stack_wz.h:
wz_walk, RankStore::fetch_lo / fetch_hi, the one-exit iteration loop of
wz_round) on the GPU: every case bit for bit against the oracle on result
bits, both rejection maps and the totals.

Frames of 70 x 96 (105 full tiles of the rounds kernels) and 3 x 129 (387
pixels: a chunk that is no multiple of 64, a partial last tile) at N = 65, 100
and 128, float and 16-bit, plain, weighted and with integer shifts.  Planted
at known pixels of rows 0-2: columns whose first clamp iteration takes 1, 2,
3, 4, 5 or 9 samples at one end,
columns with 16, 17 and 20 outliers at one end (the walk leaves the 16 stored
ranks), kept of 1, 2, 3, 39, 40 and 41, constant columns.  SGPU_WZ_SPLIT is
read once per process, so the stacks run in one fresh child per value: 2 (the
head's capped rounds and the tail kernel) and 0 (every round in the head)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (65, 100, 128)
SHAPES = ((70, 96), (3, 129))
SIG = (3.0, 3.0)
PLANTED = (1, 2, 3, 4, 5, 9, 16, 17, 20)
KEPT = (1, 2, 3, 39, 40, 41)


def _frames(n, h, w, seed):
    from siril_amd import synth
    fr = synth.frames_numpy(n, h, w, seed=seed)
    rng = np.random.default_rng(seed)
    fr[rng.random(fr.shape) < 0.04] = 0.0
    wd = 0.005
    for i, m in enumerate(PLANTED):
        for row, sgn in ((0, -1.0), (1, 1.0)):       # row 0: low end, row 1: high end
            col = 0.06 + wd * rng.uniform(-1.0, 1.0, n)
            col[:m] = 0.06 + sgn * wd * rng.uniform(8.0, 8.5, m)
            fr[:, row, 3 + 5 * i] = rng.permutation(col).astype(np.float32)
    for i, k in enumerate(KEPT):
        col = np.zeros(n, np.float32)
        col[:k] = (0.06 + wd * rng.standard_normal(k)).astype(np.float32)
        fr[:, 2, 4 + 7 * i] = rng.permutation(col)
    fr[:, 2, 60:64] = np.float32(0.0625)             # constant columns
    fr[0, 2, 63] = np.float32(0.3)                   # ... one with an outlier
    return fr


def _to16(fr):
    return np.where(fr == 0.0, 0, np.clip(np.round(fr.astype(np.float64) * 20000.0), 1, 65535)).astype(np.uint16)


def _variants(n):
    rng = np.random.default_rng(1000 + n)
    return {"plain": {}, "weights": {"weights": rng.uniform(0.5, 2.0, n)}, "shift": {"dx": np.round(rng.uniform(-6, 6, n))}}


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from siril_amd import stacking as S
inp = np.load(sys.argv[2])
cases = json.loads(inp["cases"].tobytes().decode())
ctx = S.Context(0)
out, info = {}, {}
for name, c in cases.items():
    kw = {}
    if c["weights"]:
        kw["weights"] = inp[c["weights"]]
    if c["dx"]:
        kw["shiftx"] = S.shifts_from_registration(inp[c["dx"]])
    res = ctx.stack(inp[c["frames"]], S.StackingArgs(S.Rejection.WINSORIZED, (3.0, 3.0), **kw))
    info[name] = {"deferred": list(ctx.last_wz_deferred()), "exact": ctx.last_exact_pixels()}
    out[name + ".result"] = res.result
    out[name + ".rl"] = res.rejmap_low
    out[name + ".rh"] = res.rejmap_high
    out[name + ".irej"] = np.array(res.irej, np.int64)
ctx.close()
np.savez(sys.argv[3], **out)
print(json.dumps(info))
"""


@pytest.fixture(scope="module")
def cases():
    """name -> (frames, variant kwargs, is16); shared, never modified"""
    cs = {}
    for n in NS:
        for (h, w) in SHAPES:
            fr = _frames(n, h, w, seed=5000 + n + h)
            fr16 = _to16(fr)
            fr.setflags(write=False)
            fr16.setflags(write=False)
            for vname, v in _variants(n).items():
                cs[f"f32_n{n}_{h}x{w}_{vname}"] = (fr, v, False)
                cs[f"u16_n{n}_{h}x{w}_{vname}"] = (fr16, v, True)
    return cs


@pytest.fixture(scope="module")
def runs(cases, tmp_path_factory):
    """the children's outputs: split -> (arrays, info)"""
    d = tmp_path_factory.mktemp("wz_walk")
    arrays, meta = {}, {}
    for name, (fr, v, is16) in cases.items():
        fkey = name.rsplit("_", 1)[0]
        arrays[fkey] = fr
        meta[name] = {"frames": fkey, "weights": None, "dx": None}
        for k in ("weights", "dx"):
            if k in v:
                arrays[name + "." + k] = v[k]
                meta[name][k] = name + "." + k
    arrays["cases"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    fin = str(d / "in.npz")
    np.savez(fin, **arrays)
    got = {}
    for split in ("2", "0"):
        fout = str(d / f"out{split}.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], env=dict(os.environ, SGPU_WZ_SPLIT=split),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[split] = (np.load(fout), json.loads(r.stdout.strip().splitlines()[-1]))
    return got


@pytest.fixture(scope="module")
def refs(cases, oracle):
    """the oracle's answer per case, computed once"""
    out = {}
    for name, (fr, v, is16) in cases.items():
        f = oracle.stack_rows_u16 if is16 else oracle.stack_rows
        out[name] = f(fr, oracle.WINSORIZED, SIG, weights=v.get("weights"), shift_dx=v.get("dx"), nthreads=8)
    return out


@pytest.mark.parametrize("split", ["2", "0"])
@pytest.mark.parametrize("kind", ["f32", "u16"])
@pytest.mark.parametrize("n", NS)
def test_against_oracle(cases, runs, refs, n, kind, split):
    arr, info = runs[split]
    names = [c for c in cases if c.startswith(f"{kind}_n{n}_")]
    assert len(names) == 6
    for name in names:
        out, rl, rh, counts = refs[name]
        res = arr[name + ".result"]
        print(name, "split", split, info[name])
        assert res.dtype == out.dtype and res.shape == out.shape
        assert np.array_equal(res.view(np.uint32), out.view(np.uint32)), \
            f"{name}: {int((res.view(np.uint32) != out.view(np.uint32)).sum())} pixels differ"
        assert np.array_equal(arr[name + ".rl"], rl) and np.array_equal(arr[name + ".rh"], rh), name
        assert tuple(arr[name + ".irej"]) == (int(counts[0]), int(counts[1])), name


def test_head_and_tail_ran(cases, runs):
    """The float split defers pixels to the tail kernel at SGPU_WZ_SPLIT=2 and
    none at 0, and both children give the same bytes."""
    a, ia = runs["2"]
    b, ib = runs["0"]
    for name in cases:
        if name.startswith("f32") and "70x96" in name:
            assert ia[name]["deferred"][0] > 0, name
        assert ib[name]["deferred"][0] == 0, name
        for key in ("result", "rl", "rh", "irej"):
            assert np.array_equal(a[f"{name}.{key}"].view(np.uint8), b[f"{name}.{key}"].view(np.uint8)), (name, key)

"""The fused prep + rounds kernel of the float WINSORIZED moment path at N =
65..128 (stack_wz.h: k_stack_wz_fused1, SGPU_WZ=7): every case bit for bit
against the oracle on result bits, both rejection maps and the totals, under
the fused mode and under SGPU_WZ=2 (the two-kernel path); a subset under the
two diagnostic modes SGPU_WZ=4 (one stream, tails after the last chunk) and
SGPU_WZ=0 (the register-resident kernel only).

SGPU_WZ and SGPU_WZ_CHUNK are read once per process, so each mode runs every
case in one fresh child (this file run as a program) and leaves its outputs in
an .npz; a second pair of children runs the many-chunk case with
SGPU_WZ_CHUNK=256.  The oracle's references are computed once per module.

Cases.  `cols<N>`: N x 3 x 333 (999 pixels: no multiple of 64 or of 4, so the
last wave is partial and the compact copies go word by word) at the ends of
every real-slot bucket the N list touches; row 0 has every sample (its waves
take the straight-line rank store), rows 1-2 have 4 % nulls (run-time slot
loops), row 2 carries planted columns: kept 0, 1, 2, 3, 39, 40, 41, a NaN, and
17 / 20 outliers at either end (walks past the 16 stored ranks: the sorted
kernel's pixels).  Each at sigma 3/3 and at 1/1 (nearly every pixel a
fallback).  `recipe`: 4 096 pixels of the bench recipe, nothing planted, at
3/3 and 1/1, and its first 70 frames at 2/2 (both tail passes).  `shift`,
`weights`, `nomaps`: the variants of the gather and of the result write.
`chunks`: 1 998 pixels in chunks of 256."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [65, 72, 73, 100, 104, 105, 120, 121, 128]
MODES = ("7", "2")


def _cols(n, seed):
    from siril_amd import synth
    fr = synth.frames_numpy(n, 3, 333, seed=seed)
    fr[fr == 0.0] = np.float32(0.25)             # row 0: kept == N in every lane
    rng = np.random.default_rng(seed)
    nulls = rng.random(fr.shape) < 0.04
    nulls[:, 0, :] = False
    nulls[:, 2, 20:24] = False
    fr[nulls] = 0.0
    fr[:, 2, 5] = 0.0                            # kept == 0
    for col, kept in ((6, 1), (7, 2), (8, 3), (9, 39), (10, 40), (11, 41)):
        fr[:, 2, col] = fr[:, 0, col]
        fr[kept:, 2, col] = 0.0
    fr[:, 2, 20:24] = fr[:, 0, 20:24]            # more than 16 outliers at one end
    fr[:20, 2, 20] += np.float32(0.5)
    fr[:17, 2, 21] += np.float32(0.5)
    fr[:20, 2, 22] *= np.float32(0.01)
    fr[:17, 2, 23] *= np.float32(0.01)
    fr[n // 2, 2, 30] = np.nan
    return fr


def build_cases(chunked):
    """name -> (frames, sigmas, variant); the same arrays in the children and here"""
    from siril_amd import synth
    cases = {}
    if chunked:
        cases["chunks"] = (synth.frames_numpy(100, 6, 333, seed=61), (3.0, 3.0), {})
        return cases
    for n in NS:
        fr = _cols(n, 700 + n)
        cases[f"cols{n}_s3"] = (fr, (3.0, 3.0), {})
        cases[f"cols{n}_s1"] = (fr, (1.0, 1.0), {})
    recipe = synth.frames_numpy(100, 8, 512, seed=62)
    cases["recipe_s3"] = (recipe, (3.0, 3.0), {})
    cases["recipe_s1"] = (recipe, (1.0, 1.0), {})
    cases["recipe70_s2"] = (np.ascontiguousarray(recipe[:70]), (2.0, 2.0), {})
    small = synth.frames_numpy(100, 3, 333, seed=63)
    rng = np.random.default_rng(64)
    cases["shift"] = (small, (3.0, 3.0), {"dx": rng.uniform(-6, 6, 100)})
    cases["weights"] = (small, (3.0, 3.0), {"weights": rng.uniform(0.5, 2.0, 100)})
    cases["nomaps"] = (small, (3.0, 3.0), {"maps": False})
    return cases


def _child(out, chunked):
    sys.path.insert(0, ROOT)
    from siril_amd import stacking as S
    ctx = S.Context(0)
    data, info = {}, {}
    for name, (fr, sig, var) in build_cases(chunked).items():
        kw = {}
        if "dx" in var:
            kw["shiftx"] = S.shifts_from_registration(var["dx"])
        if "weights" in var:
            kw["weights"] = var["weights"]
        if var.get("maps") is False:
            kw["create_rejmaps"] = False
        res = ctx.stack(fr, S.StackingArgs(S.Rejection.WINSORIZED, sig, **kw))
        info[name] = {"deferred": list(ctx.last_wz_deferred()), "fallback": ctx.last_wz_fallback(),
                      "exact": ctx.last_exact_pixels()}
        data[name + ".result"] = res.result
        data[name + ".irej"] = np.array(res.irej, np.int64)
        if res.rejmap_low is not None:
            data[name + ".rl"] = res.rejmap_low
            data[name + ".rh"] = res.rejmap_high
    ctx.close()
    np.savez(out, **data)
    print(json.dumps(info))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2] == "chunked")
    sys.exit(0)


def _run(tmp, mode, chunked):
    env = dict(os.environ, SGPU_WZ=mode)
    env.pop("SGPU_WZ_CHUNK", None)
    if chunked:
        env["SGPU_WZ_CHUNK"] = "256"
    f = str(tmp / f"wz{mode}{'c' if chunked else ''}.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), f, "chunked" if chunked else "plain"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(f), json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(mode, chunked) -> (outputs, counters): one child each, started on first use"""
    tmp = tmp_path_factory.mktemp("wzfused")
    done = {}

    def get(mode, chunked=False):
        if (mode, chunked) not in done:
            done[(mode, chunked)] = _run(tmp, mode, chunked)
        return done[(mode, chunked)]
    return get


@pytest.fixture(scope="module")
def refs(oracle):
    """case -> the oracle's (result, rl, rh, counts), computed on first use, never modified"""
    built = {False: None, True: None}
    done = {}

    def get(name, chunked=False):
        if name not in done:
            if built[chunked] is None:
                built[chunked] = build_cases(chunked)
            fr, sig, var = built[chunked][name]
            done[name] = oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8, weights=var.get("weights"),
                                           shift_dx=var.get("dx"))
        return done[name]
    return get


def _check(out, name, ref, maps=True):
    res, rl, rh, counts = ref
    got = out[name + ".result"]
    assert np.array_equal(got.view(np.uint32), res.view(np.uint32)), \
        f"{int((got.view(np.uint32) != res.view(np.uint32)).sum())} pixels differ"
    if maps:
        assert np.array_equal(out[name + ".rl"], rl) and np.array_equal(out[name + ".rh"], rh)
    else:
        assert name + ".rl" not in out.files
    assert tuple(out[name + ".irej"]) == (int(counts[0]), int(counts[1]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sig", ["s3", "s1"])
@pytest.mark.parametrize("n", NS)
def test_columns(runs, refs, n, sig, mode):
    """Planted columns at both ends of each real-slot bucket; kept == 0 and the
    NaN are the exact kernel's, the 17 / 20 outliers the sorted kernel's, and
    at sigma 3/3 pixels outlast the head's two rounds."""
    out, info = runs(mode)
    name = f"cols{n}_{sig}"
    print(name, "mode", mode, info[name])
    _check(out, name, refs(name))
    assert sig != "s3" or info[name]["deferred"][0] > 0
    assert info[name]["fallback"] >= 4           # the four outlier columns at the least
    assert info[name]["exact"] >= 2              # kept == 0 and the NaN at the least


@pytest.mark.parametrize("mode", MODES)
def test_recipe(runs, refs, mode):
    """4 096 pixels of the bench recipe, nothing planted: at sigma 3/3 about
    6 % of them go past round 2 and 0.7 % take the sorted fallback
    (scripts/wzstat).  At sigma 1/1 the clip takes more than the 16 stored
    ranks of an end from nearly every pixel, so that data is fallback-heavy
    (a handful of pixels deferred, none twice) and cannot show the
    second tail pass; the first 70 frames at sigma 2/2 (test_wz_split_gpu's
    two-deferral data) do, and carry that assertion."""
    out, info = runs(mode)
    print("mode", mode, info["recipe_s3"], info["recipe_s1"], info["recipe70_s2"])
    _check(out, "recipe_s3", refs("recipe_s3"))
    assert info["recipe_s3"]["deferred"][0] > 0
    assert info["recipe_s3"]["fallback"] > 0
    _check(out, "recipe_s1", refs("recipe_s1"))
    assert info["recipe_s1"]["fallback"] > 2048
    _check(out, "recipe70_s2", refs("recipe70_s2"))
    d = info["recipe70_s2"]["deferred"]
    assert d[0] > 0 and d[1] > 0 and d[1] <= d[0] <= 4096


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["shift", "weights", "nomaps"])
def test_variants(runs, refs, name, mode):
    """Shifted frames (the XF kernels), per-frame weights (weighted_mean in
    the fused kernel and in the tail), and a stack without rejection maps."""
    out, info = runs(mode)
    _check(out, name, refs(name), maps=name != "nomaps")
    assert info[name]["deferred"][0] > 0


@pytest.mark.parametrize("mode", MODES)
def test_many_chunks(runs, refs, mode):
    """1 998 pixels in chunks of 256 (seven full chunks and one of 206: a
    partial tile whose copies go word by word): the one workspace buffer is
    reused by every chunk, each chunk's fallbacks follow its appends."""
    out, info = runs(mode, True)
    print("mode", mode, info["chunks"])
    _check(out, "chunks", refs("chunks", True))
    assert info["chunks"]["deferred"][0] > 0


DIAG_CASES = ["cols100_s3", "cols65_s1", "cols128_s3", "recipe70_s2", "shift", "weights"]


@pytest.mark.parametrize("mode", ["4", "0"])
def test_diagnostic_modes(runs, refs, mode):
    """SGPU_WZ=4 (the two kernels on one stream, no per-chunk tails: the
    per-kernel times of a profile) and SGPU_WZ=0 (no moment path).  Both give
    the oracle's bits; mode 4 runs mode 2's kernels with the same rounds cap
    and only the streams differ, so it defers the same pixels."""
    out, info = runs(mode)
    outc, infoc = runs(mode, True)
    for name in DIAG_CASES:
        print(name, "mode", mode, info[name])
        _check(out, name, refs(name))
    print("chunks mode", mode, infoc["chunks"])
    _check(outc, "chunks", refs("chunks", True))
    if mode == "4":
        _, info2 = runs("2")
        _, info2c = runs("2", True)
        for name in DIAG_CASES:
            assert info[name]["deferred"] == info2[name]["deferred"], name
        assert infoc["chunks"]["deferred"] == info2c["chunks"]["deferred"]

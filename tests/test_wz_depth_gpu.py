"""The float WINSORIZED moment path at N = 65..128 with the fused form's deeper
rank record (stack_wz.h: RankStore<128, 1, wz_fused_kt(RSL)>, 20 ranks per end
in the LDS tile of k_stack_wz_fused1 and in the k_stack_wz_tail that follows
it from the real-slot bucket 96 up; the buckets below and the two-kernel form
keep 16) and with the tail passes chosen by the
launch's sigmas (stack_wz_launch.h: wz_tail_passes -- one pass to the end when
both are >= 3, else two).  Every case bit for bit against the oracle on result
bits, both rejection maps and the totals, under the fused form (SGPU_WZ=7) and
the two-kernel form (SGPU_WZ=2).

SGPU_WZ is read once per process, so each mode runs every case in one fresh
child (this file run as a program) and leaves its outputs in an .npz.  The
oracle's references are computed once per module.

Cases.
`depth`: 100 x 3 x 333 (999 pixels: 15 full tiles and one of 39; 999 is no
multiple of 4, so every tile's compact copies go word by word -- the wide
copies at R = 48 run in the `ends` cases from N = 89 up, 772 pixels, and in
`pass3`); rows 0-1 the bench recipe, row 2 carries columns with
d = 15 .. 22 outliers at the high end and d = 15 .. 22 at the low end, on
recipe columns, and columns with 6 .. 13 outliers at both ends (the median
stays inside the stored middle ranks and the walks end inside 16 stored ranks,
between 16 and 20, or past 20).  The
fallback counts (pixels handed to the register-resident kernel) of the two
forms are compared with the host's count at each form's depth
(tests/hostsim/wz_depth_count.hip), and so is their difference.
`ends<N>`: N = 65, 72, 97, 104, 121, 128 (both ends of three real-slot buckets
RS = 72, 104, 128) and N = 88, 89, 113 (the last bucket at 16 ranks per end,
the first at 20 -- RS = 96, where the fused kernel's tiles and the tail kernel
change -- and RS = 120), 4 x 193 pixels; waves with 0, 1, 7 and 8 nulls per column
mixed, so that the straight-line store (every lane's kept >= RS - 7) and the
run-time slot loops meet at kept = RS - 7; a NaN column, constant columns and
a kept == 1 column.
`pass3`: the 100 x 8 x 1000 recipe at sigma 3/3 (one tail pass); `pass70_s2`:
its first 70 frames at 2/2 (two); `pass3_shift`: shifted frames at 3/3 -- the
two-kernel form with one pass under SGPU_WZ=2 (what an unset SGPU_WZ runs on
shifted frames), the shifted fused kernel with one pass under SGPU_WZ=7."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END_NS = [65, 72, 88, 89, 97, 104, 113, 121, 128]
DS = list(range(15, 23))
BOTH_DS = list(range(6, 14))
MODES = ("7", "2")


def _depth_frames():
    from siril_amd import synth
    fr = synth.frames_numpy(100, 3, 333, seed=81)
    fr[:, 2, :] = fr[:, 0, :]
    row = fr[:, 2, :]
    row[row == 0.0] = np.float32(0.25)           # every sample present in the planted row
    for i, d in enumerate(DS):
        row[:d, 40 + 2 * i] += np.float32(0.5)   # d outliers at the high end
        row[:d, 140 + 2 * i] *= np.float32(0.01)  # d at the low end
    # One-sided clips of that many samples also move the median out of the
    # stored middle ranks, so those columns leave the moment path at any depth.
    # Outliers at both ends keep the median where it is: d = 6 .. 13 a side,
    # where the later rounds' walks end inside 16 ranks, between 16 and 20, or
    # past 20 of an end
    for i, d in enumerate(BOTH_DS):
        row[:d, 240 + 2 * i] += np.float32(0.5)
        row[d:2 * d, 240 + 2 * i] *= np.float32(0.01)
    return fr


def _planted(base):
    """pixel indices of the columns base + 2 i of row 2, i over DS"""
    return 2 * 333 + np.array([base + 2 * i for i in range(len(DS))])


def _ends_frames(n):
    from siril_amd import synth
    h, w = 4, 193
    fr = synth.frames_numpy(n, h, w, seed=900 + n)
    fr[fr == 0.0] = np.float32(0.25)
    flat = fr.reshape(n, h * w)
    rng = np.random.default_rng(1000 + n)
    npx = h * w
    nulls = np.zeros(npx, np.int64)
    cyc3, cyc4 = np.array([0, 1, 7]), np.array([0, 1, 7, 8])
    for wv in range((npx + 63) // 64):
        lanes = np.arange(wv * 64, min(npx, wv * 64 + 64))
        k = wv % 8
        if k == 0:
            nulls[lanes] = 0                     # straight-line store at every N
        elif k == 1:
            nulls[lanes] = cyc3[lanes % 3]       # straight line at N = RS, slot loops at N = RS - 7
        elif k == 2:
            nulls[lanes] = cyc4[lanes % 4]       # one lane in four below RS - 7
        elif k == 3:
            nulls[lanes] = 0
            nulls[lanes[37 % len(lanes)]] = 8    # a single lane sends the wave to the slot loops
        elif k == 4:
            nulls[lanes] = 7
        elif k == 5:
            nulls[lanes] = 8
        else:
            nulls[lanes] = cyc4[rng.integers(0, 4, len(lanes))]
    for j in range(npx):
        if nulls[j]:
            flat[rng.choice(n, int(nulls[j]), replace=False), j] = 0.0
    flat[:, 6] = flat[3, 6]                      # constant column in a straight-line wave
    flat[:, 64 * 2 + 9] = np.where(flat[:, 64 * 2 + 9] != 0, np.float32(0.125), 0)   # constant, with nulls
    flat[n // 2, 64 * 2 + 20] = np.nan           # NaN: the exact kernel's
    flat[n // 3, 11] = np.nan                    # ... and in a straight-line wave
    flat[1:, 64 * 6 + 5] = 0.0                   # kept == 1
    return fr


def build_cases():
    """name -> (frames, sigmas, variant); the same arrays in the children and here"""
    from siril_amd import synth
    cases = {"depth": (_depth_frames(), (3.0, 3.0), {})}
    for n in END_NS:
        cases[f"ends{n}"] = (_ends_frames(n), (3.0, 3.0), {})
    recipe = synth.frames_numpy(100, 8, 1000, seed=82)
    cases["pass3"] = (recipe, (3.0, 3.0), {})
    cases["pass70_s2"] = (np.ascontiguousarray(recipe[:70]), (2.0, 2.0), {})
    rng = np.random.default_rng(83)
    cases["pass3_shift"] = (np.ascontiguousarray(recipe[:, :2, :]), (3.0, 3.0), {"dx": rng.uniform(-6, 6, 100)})
    return cases


def _child(out):
    sys.path.insert(0, ROOT)
    from siril_amd import stacking as S
    ctx = S.Context(0)
    data, info = {}, {}
    for name, (fr, sig, var) in build_cases().items():
        kw = {}
        if "dx" in var:
            kw["shiftx"] = S.shifts_from_registration(var["dx"])
        res = ctx.stack(fr, S.StackingArgs(S.Rejection.WINSORIZED, sig, **kw))
        info[name] = {"deferred": list(ctx.last_wz_deferred()), "fallback": ctx.last_wz_fallback(),
                      "exact": ctx.last_exact_pixels()}
        data[name + ".result"] = res.result
        data[name + ".irej"] = np.array(res.irej, np.int64)
        data[name + ".rl"] = res.rejmap_low
        data[name + ".rh"] = res.rejmap_high
    ctx.close()
    np.savez(out, **data)
    print(json.dumps(info))


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> (outputs, counters): one child each, started on first use"""
    tmp = tmp_path_factory.mktemp("wzdepth")
    done = {}

    def get(mode):
        if mode not in done:
            env = dict(os.environ, SGPU_WZ=mode)
            env.pop("SGPU_WZ_CHUNK", None)
            f = str(tmp / f"wz{mode}.npz")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), f], env=env, capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            done[mode] = (np.load(f), json.loads(r.stdout.strip().splitlines()[-1]))
        return done[mode]
    return get


@pytest.fixture(scope="module")
def refs(oracle, cases):
    """case -> the oracle's (result, rl, rh, counts), computed on first use, never modified"""
    done = {}

    def get(name):
        if name not in done:
            fr, sig, var = cases[name]
            done[name] = oracle.stack_rows(fr, oracle.WINSORIZED, sig, nthreads=8, shift_dx=var.get("dx"))
        return done[name]
    return get


@pytest.fixture(scope="module")
def depth_lib():
    """Host build of the moment path's routes at a given record depth, tests only."""
    csrc = os.path.join(ROOT, "siril_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostsim", "wz_depth_count.hip")
    lib = os.path.join(ROOT, "tests", "hostsim", "libwzdepth.so")
    deps = [src] + [os.path.join(csrc, h) for h in ("stack_sorted_impl.h", "stack_wz.h", "sgpu_kparams.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(map(os.path.getmtime, deps)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC",
                        "-shared", "-ffp-contract=off", "-I" + csrc, src, "-o", lib], check=True)
    L = C.CDLL(lib)
    L.wz_depth_of.restype = C.c_int
    L.wz_depth_of.argtypes = [C.c_int, C.c_int]
    L.wz_depth_routes.restype = C.c_int
    L.wz_depth_routes.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_longlong, C.c_float, C.c_float, C.c_int,
                                  C.POINTER(C.c_int)]
    return L


def _host_routes(L, fr, sig, kt):
    n = fr.shape[0]
    flat = np.ascontiguousarray(fr.reshape(n, -1), np.float32)
    route = np.zeros(flat.shape[1], np.int32)
    rc = L.wz_depth_routes(flat.ctypes.data_as(C.POINTER(C.c_float)), n, flat.shape[1], sig[0], sig[1], kt,
                           route.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return route


def _check(out, name, ref):
    res, rl, rh, counts = ref
    got = out[name + ".result"]
    assert np.array_equal(got.view(np.uint32), res.view(np.uint32)), \
        f"{int((got.view(np.uint32) != res.view(np.uint32)).sum())} pixels differ"
    assert np.array_equal(out[name + ".rl"], rl) and np.array_equal(out[name + ".rh"], rh)
    assert tuple(out[name + ".irej"]) == (int(counts[0]), int(counts[1]))


@pytest.mark.parametrize("mode", MODES)
def test_depth_parity(runs, refs, mode):
    out, info = runs(mode)
    print("mode", mode, info["depth"])
    _check(out, "depth", refs("depth"))
    assert info["depth"]["deferred"][0] > 0


def test_depth_fallback_counts(runs, cases, depth_lib):
    """The pixels each form hands to the register-resident kernel are the ones
    the host finds at that form's depth; the planted columns between the two
    depths are in the difference."""
    fr, sig, _ = cases["depth"]
    kt_fused, kt_two = depth_lib.wz_depth_of(1, fr.shape[0]), depth_lib.wz_depth_of(0, fr.shape[0])
    r_fused = _host_routes(depth_lib, fr, sig, kt_fused)
    r_two = _host_routes(depth_lib, fr, sig, kt_two)
    want_fused, want_two = int((r_fused == 1).sum()), int((r_two == 1).sum())
    got_fused, got_two = runs("7")[1]["depth"]["fallback"], runs("2")[1]["depth"]["fallback"]
    print("depths", kt_fused, kt_two, "host", want_fused, want_two, "gpu", got_fused, got_two)
    # (only the difference is asserted: a count itself can differ between host
    # and device by a pixel whose sigma interval rests on the square root
    # instruction -- sqrt_lo / sqrt_hi bracket either one -- at both depths alike)
    assert got_two - got_fused == want_two - want_fused
    # the data does what it is there for: a walk over d outliers reads the rank
    # d from the end, so it leaves a record of depth <= d; and the two depths
    # part on some of the both-ends columns
    d = np.array(DS)
    for base in (40, 140):
        assert (r_two[_planted(base)[d >= kt_two]] == 1).all()
        assert (r_fused[_planted(base)[d >= kt_fused]] == 1).all()
    both = _planted(240)
    assert kt_fused == kt_two or ((r_two[both] == 1) & (r_fused[both] == 0)).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", END_NS)
def test_bucket_ends(runs, refs, n, mode):
    out, info = runs(mode)
    name = f"ends{n}"
    print(name, "mode", mode, info[name])
    _check(out, name, refs(name))
    assert info[name]["exact"] >= 2               # the two NaN columns at the least
    assert info[name]["deferred"][0] > 0


@pytest.mark.parametrize("mode", MODES)
def test_one_tail_pass_at_sigma_3(runs, refs, mode):
    """Sigma 3/3: one tail pass runs to the end, nothing enters a second; the
    first 70 frames at 2/2 keep two passes.  Shifted frames: the two-kernel
    form under mode 2, the shifted fused kernel under mode 7, one pass each."""
    out, info = runs(mode)
    print("mode", mode, info["pass3"], info["pass70_s2"], info["pass3_shift"])
    for name in ("pass3", "pass70_s2", "pass3_shift"):
        _check(out, name, refs(name))
    assert info["pass3"]["deferred"][0] > 0 and info["pass3"]["deferred"][1] == 0
    assert info["pass3_shift"]["deferred"][0] > 0 and info["pass3_shift"]["deferred"][1] == 0
    d = info["pass70_s2"]["deferred"]
    assert d[0] > 0 and d[1] > 0 and d[1] <= d[0]

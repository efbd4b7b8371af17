"""Time the calibration kernels on 6000x4000 frames, N = 16 per call (HIP
events after warm-up): `python scripts/calibrate_bench.py [out.json]`
(profiles/calibrate_6000x4000.json).

Per input type (WORD, float32) four configurations: dark + flat; the same
with -opt; the same with a 3-sigma hot list (-cc=dark -1 3); the cosmetic step
alone.  Bytes are the traffic model's: N * W*H * (elem + 4) + the masters
once; the fraction is of 8 TB/s, as the rest of profiles/ reports it."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import calibration as CAL  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H, N = 6000, 4000, 16
WARM, STEPS = 5, 30
HBM = 8e12
ctx = Context(0)
rng = np.random.default_rng(1)

# a gamma(2, 200) ADU dark with 0.1 % of its pixels hot, a vignetted flat
dark = rng.gamma(2.0, 200.0, (H, W)).astype(np.float32)
dark.ravel()[rng.choice(W * H, W * H // 1000, replace=False)] = 30000.0
yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
flat = (30000.0 * (1.0 - 0.3 * (((xx - W / 2) / W) ** 2 + ((yy - H / 2) / H) ** 2))).astype(np.float32)
del yy, xx
dark16 = np.rint(dark).astype(np.uint16)
flat16 = np.rint(flat).astype(np.uint16)
light = (2000.0 + dark + rng.normal(0.0, 30.0, (H, W)).astype(np.float32))
frames16 = np.stack([np.clip(np.rint(light + 3.0 * f), 0, 65535).astype(np.uint16) for f in range(N)])
del light, dark, flat

res = {"width": W, "height": H, "frames_per_call": N, "warmup": WARM, "steps": STEPS, "hbm_peak_bytes_per_s": HBM,
       "cases": {}}


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
            "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(9 * len(ts)) // 10], 4)}


plain = CAL.prepare_masters(dark=dark16, flat=flat16, ctx=ctx)
hot = CAL.prepare_masters(dark=dark16, flat=flat16, cc_sigma=(-1.0, 3.0), ctx=ctx)
res["hot_list_entries"] = int(hot.deviant.shape[0])
res["hot_list_stats"] = hot.cc_stats
print("hot list:", res["hot_list_entries"], "entries", flush=True)

for name in ("word", "float32"):
    if name == "word":
        d = torch.from_numpy(frames16.view(np.int16)).cuda()
        elem = 2
    else:
        d = torch.from_numpy(frames16.astype(np.float32) * CAL.INV_USHRT_MAX).cuda()
        elem = 4
    out = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    model_bytes = N * W * H * (elem + 4) + 2 * W * H * 4

    def case(label, fn, bytes_=None, base=None):
        t = timed(fn)
        t["per_frame_ms"] = round(t["median_ms"] / N, 5)
        if bytes_:
            t["model_bytes"] = bytes_
            t["model_gb_per_s"] = round(bytes_ / (t["median_ms"] * 1e-3) / 1e9, 1)
            t["fraction_of_hbm_peak"] = round(bytes_ / (t["median_ms"] * 1e-3) / HBM, 4)
        if base is not None:
            t["added_per_frame_ms"] = round((t["median_ms"] - base["median_ms"]) / N, 5)
        res["cases"][f"{name}_{label}"] = t
        print(name, label, json.dumps(t), flush=True)
        return t

    base = case("dark_flat", lambda: CAL.calibrate(d, plain, out=out, ctx=ctx), model_bytes)
    t = case("dark_flat_opt", lambda: CAL.calibrate(d, plain, dark_optim=True, out=out, ctx=ctx), base=base)
    t["k"] = [round(float(v), 5) for v in CAL.calibrate(d, plain, dark_optim=True, out=out, ctx=ctx)[1]]
    case("dark_flat_hot3", lambda: CAL.calibrate(d, hot, out=out, ctx=ctx), base=base)
    case("cosmetic_only", lambda: CAL.cosmetic_correction(out, hot.deviant, False, ctx=ctx))
    del d, out

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "calibrate_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

"""Time the background extraction on 6000x4000 planes, 16 per call (HIP events
after warm-up): `python scripts/subsky_bench.py [out.json]`
(profiles/subsky_6000x4000.json).

Per input type (WORD, float32) and degree (1, 4): the whole call (box medians,
fit, streaming pass: three launches) and each kernel on its own, from the
events the entry records between the launches.  Bytes are the traffic model's:
P * W*H * (elem + 4) for the streaming pass (the boxes add K * 625 * elem per
plane, under 1 %); the fraction is of 8 TB/s, as the rest of profiles/ reports
it.  The yardstick is k_calibrate_vec (dark + flat) on the same frames in the
same process: its model adds the two masters once."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import background as BKG  # noqa: E402
from siril_amd import calibration as CAL  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H, P = 6000, 4000, 16
WARM, STEPS = 5, 30
HBM = 8e12
ctx = Context(0)

# a sky gradient of its own per plane, noise, and a raised patch (built on the device)
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.arange(W, device="cuda", dtype=torch.float32)[None, :] / W
y = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] / H
f32 = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
for p in range(P):
    f32[p] = 0.1 + 0.002 * p + 0.04 * x + 0.03 * y + 0.02 * x * y + 0.015 * (x - 0.5) ** 2
    f32[p] += 0.002 * torch.randn((H, W), generator=g, device="cuda")
    f32[p, : H // 2, int(0.7 * W):] += 0.2
u16 = torch.round(f32 * 65535.0).clamp(0, 65535).to(torch.int32).to(torch.int16)      # WORD bits in int16 storage
grid = BKG.sample_grid(W, H, 20)

res = {"width": W, "height": H, "planes_per_call": P, "warmup": WARM, "steps": STEPS, "hbm_peak_bytes_per_s": HBM,
       "grid": grid, "cases": {}}


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def timed(fn, kernels=False):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts, ks = [], []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
        if kernels:
            ks.append(BKG.last_kernel_ms(ctx))
    t = stats(ts)
    if kernels:
        for j, name in enumerate(("box_median", "fit", "apply")):
            t[name] = stats([k[j] for k in ks])
    return t


def rate(t, bytes_):
    t["model_bytes"] = bytes_
    t["model_gb_per_s"] = round(bytes_ / (t["median_ms"] * 1e-3) / 1e9, 1)
    t["fraction_of_hbm_peak"] = round(bytes_ / (t["median_ms"] * 1e-3) / HBM, 4)


dark = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
flat = torch.full((H, W), 0.5, dtype=torch.float32, device="cuda")
masters = CAL.Masters(dark=dark, flat=flat, norm=0.5, ctx=ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

for name, d, elem in (("word", u16, 2), ("float32", f32, 4)):
    out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
    t = timed(lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), elem, P, W, H, W * H, masters))
    rate(t, P * W * H * (elem + 4) + 2 * W * H * 4)
    res["cases"][f"{name}_calibrate_yardstick"] = t
    print(name, "calibrate yardstick", json.dumps(t), flush=True)
    for degree in (1, 4):
        prm = BKG._params(degree, 20, 1.0, False)
        status = torch.empty(P, dtype=torch.int32, device="cuda")
        kept = torch.empty(P, dtype=torch.int32, device="cuda")
        t = timed(lambda: BKG.subsky_device(ctx, d.data_ptr(), elem, P, W, H, W * H, prm, out.data_ptr(),
                                            d_kept=kept.data_ptr(), d_status=status.data_ptr()), kernels=True)
        assert not status.cpu().numpy().any()
        t["kept"] = [int(v) for v in kept.cpu().numpy()]
        bytes_ = P * W * H * (elem + 4)
        rate(t["apply"], bytes_)
        t["box_bytes"] = P * grid["K"] * 625 * elem
        t["apply_rate_over_calibrate_rate"] = round(
            t["apply"]["model_gb_per_s"] / res["cases"][f"{name}_calibrate_yardstick"]["model_gb_per_s"], 4)
        res["cases"][f"{name}_degree{degree}"] = t
        print(name, "degree", degree, json.dumps(t), flush=True)
    del out

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "subsky_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

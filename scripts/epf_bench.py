"""Time the guided filter (`epf -guided`) on 6000x4000 float32 planes, 4 per
call (HIP events after warm-up): `python scripts/epf_bench.py OUT.json PART
[PART ...]` (profiles/epf_6000x4000.json).  Every invocation is one process
that runs the yardstick and the parts named, and merges its results into
OUT.json, so that the parts can run one after the other, each under a time
limit of its own:

    guided     d = 3, 9, 25, guided by the input itself and by a second image
    median     fmedian (the selection route) at ksize 9 and 15 against the
               guided filter at the same d, their calls alternating: a windowed
               filter may not take longer than the bisection median

A call's time is taken both around the call (torch events) and per launch from
the events the entry records (`last_kernel_ms_epf`).

The filter is held against memory: its model is 28 bytes per pixel guided by
itself (pass A reads p and writes a, b; pass B reads a, b, I and writes the
result) and 32 with a guide; the halo a tile reads again,
(64 + 2r)(th + 2r) / (64 th) with th = 32 up to d = 17 and 16 above, is not in
the model: the bar (for d = 3) is 0.9 of the yardstick's rate divided by that
amplification.  The yardstick is k_calibrate_vec (dark + flat) on the same
frames in the same process."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import calibration as CAL  # noqa: E402
from siril_amd import filters as FL  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H, P = 6000, 4000, 4
WARM, STEPS = 3, 15
PARTS = ("guided", "median")
SI, SS = 0.02, 3.0

if len(sys.argv) < 3 or any(p not in PARTS for p in sys.argv[2:]):
    sys.exit(__doc__)
path, parts = sys.argv[1], sys.argv[2:]
assert torch.cuda.is_available(), "epf_bench needs a HIP device"
ctx = Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

g = torch.Generator(device="cuda").manual_seed(1)
f32 = 0.2 + 0.05 * torch.rand((P, H, W), generator=g, device="cuda")
npx = P * W * H
out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")

res = json.load(open(path)) if os.path.exists(path) else {}
res.update(width=W, height=H, planes_per_call=P, warmup=WARM, steps=STEPS, si=SI, ss=SS)
res.setdefault("cases", {})


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def timed(fns):
    """fns: {name: (call, launches)}; the calls alternate inside every step.  {name: whole-call stats, + per launch}."""
    for _ in range(WARM):
        for fn, _ in fns.values():
            fn()
    torch.cuda.synchronize()
    ts, ks = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(STEPS):
        for n, (fn, launches) in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[n].append(a.elapsed_time(b))
            ks[n].append(launches(ctx))
    r = {}
    for n in fns:
        r[n] = stats(ts[n])
        r[n]["launches"] = {}
        for k in range(len(ks[n][0])):
            r[n]["launches"][f"{ks[n][0][k][0]} {ks[n][0][k][1]}"] = stats([s[k][2] for s in ks[n]])
    return r


def yardstick(d, elem):
    dark = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
    flat = torch.full((H, W), 0.5, dtype=torch.float32, device="cuda")
    masters = CAL.Masters(dark=dark, flat=flat, norm=0.5, ctx=ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    t = timed({"cal": (lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), elem, P, W, H, W * H, masters),
                       lambda c: [])})["cal"]
    t["model_bytes"] = npx * (elem + 4) + 2 * W * H * 4
    t["model_gb_per_s"] = round(t["model_bytes"] / (t["median_ms"] * 1e-3) / 1e9, 1)
    return t


def epf_call(d, guide=None):
    gp = guide.data_ptr() if guide is not None else 0
    return (lambda: FL.epf_device(ctx, f32.data_ptr(), 4, P, W, H, W * H, gp, 4 if gp else 0, W * H if gp else 0,
                                  FL.EPF_GUIDED, d, SI, SS, 1.0, out.data_ptr(), W * H), FL.last_kernel_ms_epf)


def med_call(ksize):
    return (lambda: FL.fmedian_device(ctx, f32.data_ptr(), 4, P, W, H, W * H, ksize, 1.0, 1, out.data_ptr(), W * H,
                                      FL.ROUTE_SELECT), FL.last_kernel_ms)


def describe_guided(t, d, with_guide, cal):
    r, th = (d - 1) // 2, 32 if d <= 17 else 16
    bpp = 32 if with_guide else 28
    t["d"] = d
    t["ns_per_pixel"] = round(t["median_ms"] * 1e6 / npx, 4)
    t["bytes_per_pixel"] = bpp
    t["model_gb_per_s"] = round(bpp * npx / (t["median_ms"] * 1e-3) / 1e9, 1)
    t["tile"] = f"64x{th}"
    t["halo_amplification"] = round((64 + 2 * r) * (th + 2 * r) / (64.0 * th), 4)
    t["rate_over_calibrate_rate"] = round(t["model_gb_per_s"] / cal, 4)
    t["amplified_rate_over_calibrate_rate"] = round(t["rate_over_calibrate_rate"] * t["halo_amplification"], 4)
    if d == 3:
        t["bar"] = round(0.9 / t["halo_amplification"], 4)
        t["meets_bar"] = t["rate_over_calibrate_rate"] >= t["bar"]
    return t


def save():
    json.dump(res, open(path, "w"), indent=1)


for part in parts:
    y = yardstick(f32, 4)
    res["cases"][f"{part}_calibrate_yardstick"] = y
    print(part, "calibrate yardstick", json.dumps(y), flush=True)
    cal = y["model_gb_per_s"]
    if part == "guided":
        guide = 0.3 + 0.05 * torch.rand((P, H, W), generator=g, device="cuda")
        for d in (3, 9, 25):
            t = describe_guided(timed({"k": epf_call(d)})["k"], d, False, cal)
            res["cases"][f"guided_self_d{d}"] = t
            print("guided by itself", d, json.dumps(t), flush=True)
            t = describe_guided(timed({"k": epf_call(d, guide)})["k"], d, True, cal)
            res["cases"][f"guided_guide_d{d}"] = t
            print("guided by a guide", d, json.dumps(t), flush=True)
            save()
        del guide
    else:
        for d in (9, 15):
            r = timed({"fmedian": med_call(d), "guided": epf_call(d)})
            for name, t in r.items():
                res["cases"][f"median_d{d}_{name}"] = t
            ratio = round(r["guided"]["median_ms"] / r["fmedian"]["median_ms"], 4)
            res["cases"][f"median_d{d}_guided_over_fmedian"] = ratio
            res["cases"][f"median_d{d}_guided_no_longer_than_fmedian"] = ratio <= 1.0
            print("median", d, json.dumps(r), flush=True)
            save()

save()
ctx.close()
print("done", flush=True)

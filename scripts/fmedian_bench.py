"""Time the median filter on 6000x4000 float32 planes, 4 per call (HIP events
after warm-up): `python scripts/fmedian_bench.py OUT.json PART [PART ...]`
(profiles/fmedian_6000x4000.json).  Every invocation is one process that runs
the yardstick and the parts named, and merges its results into OUT.json, so
that the parts can run one after the other, each under a time limit of its
own:

    auto     ksize 3, 5, 7, 9, 11, 15 as dispatched (route 0)
    routes   every ksize that has a network: the network (route 1) against
             the selection (route 2), their calls alternating
    narrow   the selection with (route 2) and without (route 3) the narrowing
             to the bits in which a window's extremes differ, ksize 3, 7, 15,
             on the bench scene and on planes of random bits (every bit
             pattern, NaN included), where narrowing cannot help
    word     ksize 3 on WORD input

A call is one launch; its time is taken both around the call (torch events)
and from the events the entry records (`last_kernel_ms`).  The model's bytes
per pixel are one read of the sample (4, or 2 for WORD) and 4 written; the
halo a tile reads again, (64 + 2r)(32 + 2r) / (64 * 32), is not in the model:
the bar (for ksize 3) is 0.9 of the yardstick's rate divided by that
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
PARTS = ("auto", "routes", "narrow", "word")

if len(sys.argv) < 3 or any(p not in PARTS for p in sys.argv[2:]):
    sys.exit(__doc__)
path, parts = sys.argv[1], sys.argv[2:]
assert torch.cuda.is_available(), "fmedian_bench needs a HIP device"
ctx = Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

g = torch.Generator(device="cuda").manual_seed(1)
f32 = 0.2 + 0.05 * torch.rand((P, H, W), generator=g, device="cuda")
npx = P * W * H
out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")

res = json.load(open(path)) if os.path.exists(path) else {}
res.update(width=W, height=H, planes_per_call=P, warmup=WARM, steps=STEPS)
res.setdefault("cases", {})


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def timed(fns):
    """fns: {name: call}; the calls alternate inside every step.  {name: whole-call stats, + kernel stats}."""
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts, ks = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(STEPS):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[n].append(a.elapsed_time(b))
            ks[n].append(FL.last_kernel_ms(ctx))
    r = {}
    for n in fns:
        r[n] = stats(ts[n])
        if ks[n][0]:
            r[n]["launch"] = stats([k[0][2] for k in ks[n]])
            r[n]["launch"]["kernel"] = f"{ks[n][0][0][0]} {ks[n][0][0][1]}"
    return r


def describe(t, ksize, elem, cal):
    r = (ksize - 1) // 2
    t["ksize"] = ksize
    t["ns_per_pixel"] = round(t["median_ms"] * 1e6 / npx, 4)
    t["bytes_per_pixel"] = elem + 4
    t["model_gb_per_s"] = round((elem + 4) * npx / (t["median_ms"] * 1e-3) / 1e9, 1)
    t["halo_amplification"] = round((64 + 2 * r) * (32 + 2 * r) / (64.0 * 32.0), 4)
    t["rate_over_calibrate_rate"] = round(t["model_gb_per_s"] / cal, 4)
    if ksize == 3:
        t["bar"] = round(0.9 / t["halo_amplification"], 4)
        t["meets_bar"] = t["rate_over_calibrate_rate"] >= t["bar"]
    return t


def yardstick(d, elem):
    dark = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
    flat = torch.full((H, W), 0.5, dtype=torch.float32, device="cuda")
    masters = CAL.Masters(dark=dark, flat=flat, norm=0.5, ctx=ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    t = timed({"cal": lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), elem, P, W, H, W * H, masters)})
    t = t["cal"]
    t["model_bytes"] = npx * (elem + 4) + 2 * W * H * 4
    t["model_gb_per_s"] = round(t["model_bytes"] / (t["median_ms"] * 1e-3) / 1e9, 1)
    return t


def call(d, elem, ksize, route):
    return lambda: FL.fmedian_device(ctx, d.data_ptr(), elem, P, W, H, W * H, ksize, 1.0, 1, out.data_ptr(), W * H, route)


def save():
    json.dump(res, open(path, "w"), indent=1)


for part in parts:
    if part == "word":
        d = torch.round(f32 * 65535.0).clamp(0, 65535).to(torch.int32).to(torch.int16)      # WORD bits in int16 storage
        y = yardstick(d, 2)
        res["cases"]["word_calibrate_yardstick"] = y
        t = describe(timed({"k": call(d, 2, 3, 0)})["k"], 3, 2, y["model_gb_per_s"])
        res["cases"]["word_auto_ksize3"] = t
        print("word ksize 3", json.dumps(t), flush=True)
        save()
        continue
    y = yardstick(f32, 4)
    res["cases"][f"{part}_calibrate_yardstick"] = y
    print(part, "calibrate yardstick", json.dumps(y), flush=True)
    cal = y["model_gb_per_s"]
    if part == "auto":
        for ksize in (3, 5, 7, 9, 11, 15):
            t = describe(timed({"k": call(f32, 4, ksize, 0)})["k"], ksize, 4, cal)
            res["cases"][f"auto_ksize{ksize}"] = t
            print("auto", ksize, json.dumps(t), flush=True)
            save()
    elif part == "routes":
        for ksize in range(3, FL.MAX_NETWORK_KSIZE + 1, 2):
            r = timed({"network": call(f32, 4, ksize, 1), "select": call(f32, 4, ksize, 2)})
            for name, t in r.items():
                res["cases"][f"routes_ksize{ksize}_{name}"] = describe(t, ksize, 4, cal)
            res["cases"][f"routes_ksize{ksize}_select_over_network"] = round(
                r["select"]["median_ms"] / r["network"]["median_ms"], 4)
            print("routes", ksize, json.dumps(r), flush=True)
            save()
    else:
        bits = torch.randint(-2 ** 31, 2 ** 31, (P, H, W), generator=g, device="cuda", dtype=torch.int64)
        bits = bits.to(torch.int32).view(torch.float32)
        for scene, d in (("bench", f32), ("random_bits", bits)):
            for ksize in (3, 7, 15):
                r = timed({"narrow": call(d, 4, ksize, 2), "wide": call(d, 4, ksize, 3)})
                for name, t in r.items():
                    res["cases"][f"narrow_{scene}_ksize{ksize}_{name}"] = describe(t, ksize, 4, cal)
                res["cases"][f"narrow_{scene}_ksize{ksize}_wide_over_narrow"] = round(
                    r["wide"]["median_ms"] / r["narrow"]["median_ms"], 4)
                print("narrow", scene, ksize, json.dumps(r), flush=True)
                save()

save()
ctx.close()
print("done", flush=True)

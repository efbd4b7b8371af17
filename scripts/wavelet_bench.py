"""Time the a trous wavelets on 6000x4000 planes, 4 per call, n = 6, type 2
(HIP events after warm-up): `python scripts/wavelet_bench.py [out.json]`
(profiles/wavelet_6000x4000.json).

Per input type (WORD, float32): the transform (`atrous`), the reconstruction
of its stored planes, and the fused `wrecons`, each as a whole call and launch
by launch from the events the entry records between the launches.  A launch's
bytes are the traffic model's, per pixel: one read of c_j (the input's sample
size for the first launch, 4 after it), 4 per plane written (c_{j+1}, w_j or
the residual), 4 + 4 for an accumulator that is read and written (4 when it is
only written), 4 for the row result read or written.  The halo a tiled launch
reads again, (64 + 2h)(32 + 2h) / (64 * 32) of its c_j, is not in the model: the bar is
0.9 of the yardstick's rate divided by that amplification.  The yardstick is
k_calibrate_vec (dark + flat) on the same frames in the same process."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import calibration as CAL  # noqa: E402
from siril_amd import wavelets as WV  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H, P, N, TYPE = 6000, 4000, 4, 6, 2
WARM, STEPS = 3, 15
HBM = 8e12
COEF = (3.0, 2.0, 1.5, 1.0, 1.0, 1.0)
ctx = Context(0)

g = torch.Generator(device="cuda").manual_seed(1)
f32 = 0.2 + 0.05 * torch.rand((P, H, W), generator=g, device="cuda")
u16 = torch.round(f32 * 65535.0).clamp(0, 65535).to(torch.int32).to(torch.int16)      # WORD bits in int16 storage
npx = P * W * H

res = {"width": W, "height": H, "planes_per_call": P, "nbr_layers": N, "type": TYPE, "warmup": WARM, "steps": STEPS,
       "hbm_peak_bytes_per_s": HBM, "cases": {}}


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def rate(t, bytes_):
    t["model_bytes"] = bytes_
    t["model_gb_per_s"] = round(bytes_ / (t["median_ms"] * 1e-3) / 1e9, 1)


def model(form, j0, ns, elem, fused):
    """(bytes per pixel, halo amplification) of one launch."""
    last = j0 + ns == N - 1
    if form == "recon":
        return 4 * ns + 4, 1.0
    if form == "row":
        return 8, 1.0
    cin = elem if j0 == 0 else 4
    if fused:
        b = cin + (4 if j0 > 0 else 0) + 4 + (0 if last else 4)
    else:
        b = cin + 4 * ns + 4
    if form == "col":
        return b + 4, 1.0
    h = 2 * ((1 << (j0 + ns)) - (1 << j0))
    return b, (64 + 2 * h) / 64.0 * (32 + 2 * h) / 32.0


def timed(fn, launches=None, elem=4, fused=False):
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
        if launches is not None:
            ks.append(WV.last_kernel_ms(ctx))
    t = stats(ts)
    if launches is not None:
        t["launches"] = []
        for k, (form, j0, ns, _) in enumerate(ks[0]):
            e = stats([r[k][3] for r in ks])
            bpp, amp = model(form, j0, ns, elem, fused)
            e.update(form=form, first_scale=j0, scales=ns, bytes_per_pixel=bpp, halo_amplification=round(amp, 4))
            rate(e, bpp * npx)
            t["launches"].append(e)
    return t


dark = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
flat = torch.full((H, W), 0.5, dtype=torch.float32, device="cuda")
masters = CAL.Masters(dark=dark, flat=flat, norm=0.5, ctx=ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
planes = torch.empty((P, N, H, W), dtype=torch.float32, device="cuda")
out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")

for name, d, elem in (("word", u16, 2), ("float32", f32, 4)):
    t = timed(lambda: CAL.calibrate_device(ctx, d.data_ptr(), out.data_ptr(), elem, P, W, H, W * H, masters))
    rate(t, npx * (elem + 4) + 2 * W * H * 4)
    cal = t["model_gb_per_s"]
    res["cases"][f"{name}_calibrate_yardstick"] = t
    print(name, "calibrate yardstick", json.dumps(t), flush=True)
    cases = (("atrous", False, lambda: WV.atrous_device(ctx, d.data_ptr(), elem, P, W, H, W * H, N, TYPE,
                                                        planes.data_ptr(), W * H, N * W * H)),
             ("reconstruct", False, lambda: WV.reconstruct_device(ctx, planes.data_ptr(), P, W, H, W * H, N * W * H, COEF,
                                                                  out.data_ptr(), W * H)),
             ("wrecons", True, lambda: WV.wrecons_device(ctx, d.data_ptr(), elem, P, W, H, W * H, COEF, TYPE,
                                                         out.data_ptr(), W * H)))
    for what, fused, fn in cases:
        t = timed(fn, launches=True, elem=elem, fused=fused)
        for e in t["launches"]:
            e["rate_over_calibrate_rate"] = round(e["model_gb_per_s"] / cal, 4)
            e["bar"] = round(0.9 / e["halo_amplification"], 4)
            e["meets_bar"] = e["rate_over_calibrate_rate"] >= e["bar"]
        t["kernel_sum_ms"] = round(sum(e["median_ms"] for e in t["launches"]), 4)
        res["cases"][f"{name}_{what}"] = t
        print(name, what, json.dumps(t), flush=True)
    two = res["cases"][f"{name}_atrous"]["median_ms"] + res["cases"][f"{name}_reconstruct"]["median_ms"]
    res["cases"][f"{name}_fused_speedup"] = round(two / res["cases"][f"{name}_wrecons"]["median_ms"], 4)
    print(name, "atrous + reconstruct over wrecons", res["cases"][f"{name}_fused_speedup"], flush=True)

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "wavelet_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

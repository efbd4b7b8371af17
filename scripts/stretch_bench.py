"""Time the stretches on one 3 x 6000 x 4000 float32 image (HIP events after
warm-up): `python scripts/stretch_bench.py [OUT.json]`
(profiles/stretch_6000x4000.json).

`mtf`, `ght` with B = 3 (independent, then -human with rgbblend), `invght`
and `asinh` through `sgpu_stretch_planes_device`: the whole call (torch events)
and the launch (`last_kernel_ms`), median, min, max.  For each:

  the fraction of the HBM rate: 576 MB (72 M samples read and written as
  float32) over the time, against 8 TB/s and against `k_calibrate_vec` (dark +
  flat) on the same planes in the same process, the streaming yardstick of
  DESIGN 6e;

  the FP64 floor: the FP64 VALU instructions a sample (or a pixel of three)
  costs on that path, counted in the ISA of scripts/micro/stretch_paths.hip
  (FP64_PER_SAMPLE; how: that file's header), times the samples, over the FP64
  VALU issue rate measured in this process by scripts/micro/fp64_rate.hip.
  rgbblend's count is given with and without the per-channel transfers that
  only clipping pixels run.

The same `mtf` and `ght` B = 3 written as plain torch float64 tensor
operations run on the same image in the same process: what a user of the
package had before."""
import ctypes as CT
import json
import math
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import calibration as CAL  # noqa: E402
from siril_amd import stretch as ST  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H, C = 6000, 4000, 3
WARM, STEPS = 3, 15
HBM_BYTES_PER_S = 8e12
# v_*_f64 instructions per sample (mono paths) or per pixel of three samples (colour paths)
FP64_PER_SAMPLE = {"mtf": 34, "ght_b3_independent": 100, "invght_b3_independent": 122, "asinh_mono": 92}
FP64_PER_PIXEL = {"ght_b3_human_rgbblend": (131, 478), "asinh_colour": (135, 135)}      # (no channel clips, all do)

assert torch.cuda.is_available(), "stretch_bench needs a HIP device"
path = sys.argv[1] if len(sys.argv) > 1 else ""
ctx = Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def timed(fn, kernel=False):
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
        if kernel:
            ks.append(ST.last_kernel_ms(ctx)[0])
    r = stats(ts)
    if kernel:
        r["launch"] = stats(ks)
    return r


# a linear stack: a dark sky with noise, a few bright regions, colour casts per channel
g = torch.Generator(device="cuda").manual_seed(1)
img = torch.empty((1, C, H, W), dtype=torch.float32, device="cuda")
for c in range(C):
    img[0, c] = 0.02 + 0.005 * c + 0.01 * torch.rand((H, W), generator=g, device="cuda")
    img[0, c, : H // 8, : W // 8] += 0.2 + 0.25 * c
img[0, :, H // 2: H // 2 + 200, W // 2: W // 2 + 200] += 0.5
out = torch.empty_like(img)
nsamples = C * W * H
model_bytes = 2 * 4 * nsamples


def fp64_rate():
    """FP64 VALU instructions x lanes per second at 8 waves per SIMD."""
    src = os.path.join(ROOT, "scripts", "micro", "fp64_rate.hip")
    co = os.path.join(ROOT, "scripts", "micro", "fp64_rate.co")
    if not os.path.exists(co) or os.path.getmtime(co) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--genco", "--offload-arch=gfx950", "-O3",
                        "-ffp-contract=off", src, "-o", co], check=True)
    hip = CT.CDLL("libamdhip64.so")
    mod, fn = CT.c_void_p(), CT.c_void_p()
    assert hip.hipModuleLoad(CT.byref(mod), co.encode()) == 0
    assert hip.hipModuleGetFunction(CT.byref(fn), mod, b"k_fp64_rate") == 0
    out = torch.zeros(256, dtype=torch.float64, device="cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks, iters = cus * 8, 1 << 15
    args = (CT.c_void_p(out.data_ptr()), CT.c_double(1.0000001), CT.c_double(1e-9), CT.c_int(iters))
    params = (CT.c_void_p * 4)(*[CT.cast(CT.pointer(a), CT.c_void_p) for a in args])
    stream = CT.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        assert hip.hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, stream, params, None) == 0
    launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    hip.hipModuleUnload(mod)
    ms = min(ts)
    rate = blocks * 256 * iters * 16 / (ms * 1e-3)
    return {"compute_units": cus, "blocks": blocks, "iters": iters, "ms": stats(ts), "fp64_lane_instr_per_s": rate,
            "fp64_lane_instr_per_cu_per_ns": round(rate / cus / 1e9, 3)}


res = {"width": W, "height": H, "channels": C, "warmup": WARM, "steps": STEPS, "model_bytes": model_bytes, "cases": {}}
res["fp64_rate"] = rate = fp64_rate()
print("fp64 rate", json.dumps(rate), flush=True)

dark = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
flat = torch.full((H, W), 0.5, dtype=torch.float32, device="cuda")
masters = CAL.Masters(dark=dark, flat=flat, norm=0.5, ctx=ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
cal = timed(lambda: CAL.calibrate_device(ctx, img.data_ptr(), out.data_ptr(), 4, C, W, H, W * H, masters))
cal["model_bytes"] = model_bytes + 2 * W * H * 4
cal["model_gb_per_s"] = round(cal["model_bytes"] / (cal["median_ms"] * 1e-3) / 1e9, 1)
res["cases"]["calibrate_yardstick"] = cal
print("calibrate yardstick", json.dumps(cal), flush=True)


def describe(t, fp64_lane_instr):
    ms = t["launch"]["median_ms"]
    t["model_gb_per_s"] = round(model_bytes / (ms * 1e-3) / 1e9, 1)
    t["fraction_of_hbm_8tb_s"] = round(model_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)
    t["rate_over_calibrate_rate"] = round(t["model_gb_per_s"] / cal["model_gb_per_s"], 4)
    t["fp64_lane_instructions"] = fp64_lane_instr
    t["fp64_floor_ms"] = round(fp64_lane_instr / rate["fp64_lane_instr_per_s"] * 1e3, 4)
    t["time_over_fp64_floor"] = round(ms / t["fp64_floor_ms"], 3)
    t["hbm_floor_ms"] = round(model_bytes / HBM_BYTES_PER_S * 1e3, 4)
    t["bound_by"] = "fp64 issue" if t["fp64_floor_ms"] > t["hbm_floor_ms"] else "hbm"
    return t


def run(name, p, per):
    t = timed(lambda: ST.stretch(img, p, out=out, ctx=ctx), kernel=True)
    res["cases"][name] = describe(t, per)
    print(name, json.dumps(t), flush=True)


ght = dict(D=5.0, B=3.0, LP=0.0, SP=0.03, HP=1.0)
run("mtf", ST.params(ST.MTF, lo=0.015, m=0.05, hi=1.0), FP64_PER_SAMPLE["mtf"] * nsamples)
run("ght_b3_independent", ST.params(ST.GHT, **ght), FP64_PER_SAMPLE["ght_b3_independent"] * nsamples)
# the fraction of pixels whose per-channel transfers run
shown = ST.stretch(img, ST.params(ST.GHT, model="human", clipmode="clip", **ght), ctx=ctx)
clipping = float((shown >= 1.0).any(dim=1).float().mean())
lo, hi = FP64_PER_PIXEL["ght_b3_human_rgbblend"]
run("ght_b3_human_rgbblend", ST.params(ST.GHT, model="human", clipmode="rgbblend", **ght),
    (lo + (hi - lo) * clipping) * W * H)
res["cases"]["ght_b3_human_rgbblend"]["clipping_pixel_fraction"] = round(clipping, 5)
run("invght_b3_independent", ST.params(ST.INVGHT, **ght), FP64_PER_SAMPLE["invght_b3_independent"] * nsamples)
run("asinh_colour", ST.params(ST.ASINH, beta=100.0, offset=0.01, model="even"), FP64_PER_PIXEL["asinh_colour"][0] * W * H)
mono = img.reshape(C, H, W)
mono_out = out.reshape(C, H, W)
t = timed(lambda: ST.stretch(mono, ST.params(ST.ASINH, beta=100.0, offset=0.01), out=mono_out, ctx=ctx), kernel=True)
res["cases"]["asinh_mono"] = describe(t, FP64_PER_SAMPLE["asinh_mono"] * nsamples)
print("asinh_mono", json.dumps(t), flush=True)


# ---- the same in plain torch float64 ----
def torch_mtf(x, lo=0.015, m=0.05, hi=1.0):
    xp = ((x.double().clamp(0.0, 1.0) - lo) / (hi - lo)).clamp(0.0, 1.0)
    return (((m - 1.0) * xp) / ((2.0 * m - 1.0) * xp - m)).float()


def torch_ght(x, D=math.expm1(5.0), B=3.0, SP=0.03):
    x = x.double().clamp(0.0, 1.0)

    def q(u):
        return 1.0 - torch.pow(1.0 + B * D * u, -1.0 / B)
    d = x - SP
    s = torch.where(d < 0.0, -q(-d), q(d))
    s0 = -(1.0 - (1.0 + B * D * SP) ** (-1.0 / B))
    s1 = 1.0 - (1.0 + B * D * (1.0 - SP)) ** (-1.0 / B)
    return ((s - s0) / (s1 - s0)).float()


for name, fn, ours in (("torch_float64_mtf", torch_mtf, "mtf"), ("torch_float64_ght_b3", torch_ght, "ght_b3_independent")):
    ref = fn(img)
    got = ST.stretch(img, ST.params(ST.MTF, lo=0.015, m=0.05, hi=1.0) if ours == "mtf" else ST.params(ST.GHT, **ght),
                     ctx=ctx)
    torch.cuda.synchronize()
    t = timed(lambda: fn(img))
    t["largest_difference_from_the_kernel"] = float((ref - got).abs().max())
    t["time_over_the_kernel"] = round(t["median_ms"] / res["cases"][ours]["launch"]["median_ms"], 2)
    res["cases"][name] = t
    del ref, got
    print(name, json.dumps(t), flush=True)

if path:
    json.dump(res, open(path, "w"), indent=1)
ctx.close()
print("done", flush=True)

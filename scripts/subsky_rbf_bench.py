"""Time the thin-plate-spline background extraction on 6000x4000 planes (HIP
events after warm-up): `python scripts/subsky_rbf_bench.py [out.json]`
(profiles/subsky_rbf_6000x4000.json).

Per input type (WORD, float32) and planes per call (3, 16) at samples = 20,
smooth = 0.5, and 3 float32 planes at samples = 38 (K = 1014, close to the
cap at 3:2): the whole call and its kernels (box medians; selection + system +
solve; evaluation pass) from the events the entry records between the
launches, and `k_bkg_fit`'s time on the same planes next to the solve's.

The yardstick of the evaluation pass is its own instruction count: pairs
(pixels x samples) x the FP64 VALU instructions per pair of the inner loop
(FP64_PER_PAIR, read from the ISA of k_bkg_rbf_apply_vec: 204 in the loop of
four pairs), over the FP64 VALU issue rate measured in this process by a
register-only multiply / add loop (scripts/micro/fp64_rate.hip, compiled to a
code object on first use and loaded with hipModuleLoad)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import background as BKG  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

W, H = 6000, 4000
WARM, STEPS = 2, 10
FP64_PER_PAIR = 51.0        # 204 v_*_f64 in the 4-pair loop body
LOOP_PER_PAIR = 65.0        # 260 instructions of every kind in it
ctx = Context(0)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def fp64_rate():
    """FP64 VALU instructions x lanes per second at 8 waves per SIMD."""
    src = os.path.join(ROOT, "scripts", "micro", "fp64_rate.hip")
    co = os.path.join(ROOT, "scripts", "micro", "fp64_rate.co")
    if not os.path.exists(co) or os.path.getmtime(co) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--genco", "--offload-arch=gfx950", "-O3",
                        "-ffp-contract=off", src, "-o", co], check=True)
    hip = C.CDLL("libamdhip64.so")
    mod, fn = C.c_void_p(), C.c_void_p()
    assert hip.hipModuleLoad(C.byref(mod), co.encode()) == 0
    assert hip.hipModuleGetFunction(C.byref(fn), mod, b"k_fp64_rate") == 0
    out = torch.zeros(256, dtype=torch.float64, device="cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks, iters = cus * 8, 1 << 15
    args = (C.c_void_p(out.data_ptr()), C.c_double(1.0000001), C.c_double(1e-9), C.c_int(iters))
    params = (C.c_void_p * 4)(*[C.cast(C.pointer(a), C.c_void_p) for a in args])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

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


def planes(P):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, :] / W
    y = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] / H
    f32 = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
    for p in range(P):
        f32[p] = 0.1 + 0.002 * p + 0.04 * x + 0.03 * y + 0.02 * x * y + 0.015 * (x - 0.5) ** 2
        f32[p] += 0.002 * torch.randn((H, W), generator=g, device="cuda")
        f32[p, : H // 2, int(0.7 * W):] += 0.2
    return f32


def timed(fn, last):
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
        ks.append(last(ctx))
    return ts, ks


res = {"width": W, "height": H, "warmup": WARM, "steps": STEPS, "fp64_per_pair": FP64_PER_PAIR,
       "loop_instructions_per_pair": LOOP_PER_PAIR, "cases": {}}
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
res["fp64_rate"] = rate = fp64_rate()
print("fp64 rate", json.dumps(rate), flush=True)

f32_all = planes(16)
for name, S, P in (("float32", 20, 3), ("float32", 20, 16), ("word", 20, 3), ("word", 20, 16), ("float32", 38, 3)):
    d = f32_all[:P]
    if name == "word":
        d = torch.round(d * 65535.0).clamp(0, 65535).to(torch.int32).to(torch.int16)
    elem = d.element_size()
    out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
    status = torch.empty(P, dtype=torch.int32, device="cuda")
    kept = torch.empty(P, dtype=torch.int32, device="cuda")
    ts, ks = timed(lambda: BKG.subsky_rbf_device(ctx, d.data_ptr(), elem, P, W, H, W * H, S, 1.0, 0.5, False,
                                                 out.data_ptr(), d_kept=kept.data_ptr(), d_status=status.data_ptr()),
                   BKG.rbf_last_kernel_ms)
    assert not status.cpu().numpy().any()
    t = stats(ts)
    for j, kname in enumerate(("box_median", "select_system_solve", "evaluate", "whole_call")):
        t[kname] = stats([k[j] for k in ks])
    t["kept"] = [int(v) for v in kept.cpu().numpy()]
    t["grid"] = BKG.sample_grid(W, H, S)
    pairs = float(W * H) * float(sum(t["kept"]))
    t["pairs"] = pairs
    floor_ms = pairs * FP64_PER_PAIR / rate["fp64_lane_instr_per_s"] * 1e3
    t["evaluate_fp64_floor_ms"] = round(floor_ms, 4)
    t["evaluate_fraction_of_fp64_issue_rate"] = round(floor_ms / t["evaluate"]["median_ms"], 4)
    t["evaluate_all_instructions_floor_ms"] = round(floor_ms * LOOP_PER_PAIR / FP64_PER_PAIR, 4)
    # the polynomial fit kernel on the same planes, next to the solve
    prm = BKG._params(4, S, 1.0, False)
    _, pk = timed(lambda: BKG.subsky_device(ctx, d.data_ptr(), elem, P, W, H, W * H, prm, out.data_ptr(),
                                            d_status=status.data_ptr()), BKG.last_kernel_ms)
    t["k_bkg_fit_degree4"] = stats([k[1] for k in pk])
    res["cases"][f"{name}_s{S}_p{P}"] = t
    print(name, "samples", S, "planes", P, json.dumps(t), flush=True)
    del out

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "subsky_rbf_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

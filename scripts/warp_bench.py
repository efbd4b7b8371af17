"""Time warp_frames on 6000x4000 frames (HIP events), against shift_frames:
`python scripts/warp_bench.py [out.json]` (profiles/warp_frames_6000x4000.json).

The reference frame of a call is one of its frames and always warps through
the identity, so a call holds two frames: [identity reference, 1.5 degree
rotation].  The same call with two identity frames is timed as well; the
rotated frame alone = t(identity + rotated) - t(identity + identity) / 2."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from siril_amd import registration as Rg  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402
from warp_ref import rotation_H, translation_H  # noqa: E402

W, H = 6000, 4000
WARM, STEPS = 5, 30
ctx = Context(0)
rng = np.random.default_rng(1)
base = (rng.random((2, H, W)) * 60000).astype(np.float32)
ROT = [translation_H(0, 0), rotation_H(W, H, 1.5, 2.3, -4.1)]
IDT = [translation_H(0, 0), translation_H(0, 0)]
res = {"width": W, "height": H, "frames_per_call": 2, "warmup": WARM, "steps": STEPS, "cases": {}}


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


for dtype in (np.float32, np.uint16):
    fr = base.astype(dtype)
    d = torch.from_numpy(fr.view(np.int16) if dtype == np.uint16 else fr).cuda()
    out = torch.empty_like(d)
    name = "float32" if dtype == np.float32 else "word"
    for label, interp, clamp in (("lanczos4_clamp", 4, True), ("lanczos4", 4, False), ("cubic_clamp", 2, True),
                                 ("linear", 1, False), ("nearest", 0, False)):
        t_rot = timed(lambda: Rg.warp_frames(d, ROT, 0, interp, clamp, out=out, ctx=ctx))
        tiles_rot = Rg.warp_last_tiles(ctx)
        t_id = timed(lambda: Rg.warp_frames(d, IDT, 0, interp, clamp, out=out, ctx=ctx))
        tiles_id = Rg.warp_last_tiles(ctx)
        c = {"identity_plus_rotated": t_rot, "tiles_staged_direct": tiles_rot, "identity_twice": t_id,
             "tiles_identity_staged_direct": tiles_id,
             "rotated_frame_ms": round(t_rot["median_ms"] - t_id["median_ms"] / 2, 4)}
        res["cases"][f"{name}_{label}"] = c
        print(name, label, json.dumps(c), flush=True)
    sx, sy = np.array([0, 3], np.int32), np.array([0, -2], np.int32)
    ts = timed(lambda: Rg.shift_frames(d, sx, sy, out=out, ctx=ctx))
    ts["per_frame_ms"] = round(ts["median_ms"] / 2, 4)
    res["cases"][f"{name}_shift_frames"] = ts
    print(name, "shift_frames", json.dumps(ts), flush=True)

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "warp_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

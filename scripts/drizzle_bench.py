"""Time drizzle_frames on 6000x4000 frames (HIP events) against its HBM floor
and against warp_frames LINEAR on the same frames in the same session:
`python scripts/drizzle_bench.py [out.json]` (profiles/drizzle_frames_6000x4000.json).

The reference frame of a call is one of its frames and always maps through
the identity, so a call holds two frames: [identity reference, 1.5 degree
rotation].  The same call with two identity frames is timed as well; the
rotated frame alone = t(identity + rotated) - t(identity + identity) / 2.
The floor of a frame is its input plane read once and its image and weight
plane written once at 8 TB/s."""
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
HBM = 8e12
ctx = Context(0)
rng = np.random.default_rng(1)
base = (rng.random((2, H, W)) * 60000).astype(np.float32)
ROT = [translation_H(0, 0), rotation_H(W, H, 1.5, 2.3, -4.1)]
IDT = [translation_H(0, 0), translation_H(0, 0)]
res = {"width": W, "height": H, "frames_per_call": 2, "warmup": WARM, "steps": STEPS, "hbm_bytes_per_s": HBM,
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
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


for dtype in (np.float32, np.uint16):
    fr = base.astype(dtype)
    d = torch.from_numpy(fr.view(np.int16) if dtype == np.uint16 else fr).cuda()
    name = "float32" if dtype == np.float32 else "word"
    wout = torch.empty_like(d)
    t_rot = timed(lambda: Rg.warp_frames(d, ROT, 0, 1, False, out=wout, ctx=ctx))
    t_id = timed(lambda: Rg.warp_frames(d, IDT, 0, 1, False, out=wout, ctx=ctx))
    warp_ms = round(t_rot["median_ms"] - t_id["median_ms"] / 2, 4)
    res["cases"][f"{name}_warp_linear"] = {"identity_plus_rotated": t_rot, "identity_twice": t_id,
                                           "rotated_frame_ms": warp_ms}
    print(name, "warp_linear", warp_ms, flush=True)
    del wout
    for scale, pixfrac in ((2.0, 1.0), (2.0, 0.5), (1.0, 1.0)):
        ow, oh = Rg.drizzle_output_size(W, H, scale)
        out = torch.empty((2, oh, ow), dtype=torch.float32, device="cuda")
        outw = torch.empty_like(out)
        floor_ms = (W * H * d.element_size() + 2 * ow * oh * 4) / HBM * 1e3
        for kernel in ("square", "turbo", "point"):
            def run(Hs):
                return Rg.drizzle_frames(d, Hs, 0, scale, pixfrac, kernel, out=out, out_weights=outw, ctx=ctx)
            t_rot = timed(lambda: run(ROT))
            tiles_rot = Rg.drizzle_last_tiles(ctx)
            t_id = timed(lambda: run(IDT))
            tiles_id = Rg.drizzle_last_tiles(ctx)
            ms = round(t_rot["median_ms"] - t_id["median_ms"] / 2, 4)
            c = {"identity_plus_rotated": t_rot, "tiles_staged_direct": tiles_rot, "identity_twice": t_id,
                 "tiles_identity_staged_direct": tiles_id, "rotated_frame_ms": ms,
                 "hbm_floor_ms": round(floor_ms, 4), "times_hbm_floor": round(ms / floor_ms, 1),
                 "times_warp_linear": round(ms / warp_ms, 1)}
            res["cases"][f"{name}_{kernel}_scale{scale:g}_pixfrac{pixfrac:g}"] = c
            print(name, kernel, scale, pixfrac, json.dumps(c), flush=True)
        del out, outw

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "drizzle_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

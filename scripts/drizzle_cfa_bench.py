"""Time the CFA drizzle (drizzle_frames(cfa=)) on 6000x4000 frames (HIP events)
against one mono drizzle_frames call and against the three masked mono calls
it replaces, all in one process:
`python scripts/drizzle_cfa_bench.py [out.json]` (profiles/drizzle_cfa_6000x4000.json).

Protocol of scripts/drizzle_bench.py: a call holds two frames, [identity
reference, 1.5 degree rotation]; the same call with two identity frames is timed
as well, and the rotated frame alone = t(identity + rotated) - t(identity +
identity) / 2.  5 warm-up calls, 30 timed, median with min - max.  The masks
w * [colour == c] of the three mono calls are built before the timed region.
Before a case is timed its fused result is compared with the three masked
results bit for bit."""
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
PATTERN = "RGGB"
ctx = Context(0)
rng = np.random.default_rng(1)
base = (rng.random((2, H, W)) * 60000).astype(np.float32)
ROT = [translation_H(0, 0), rotation_H(W, H, 1.5, 2.3, -4.1)]
IDT = [translation_H(0, 0), translation_H(0, 0)]
pat, dim = Rg._cfa_args(PATTERN)
jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
colour = pat[(jj % dim) * dim + (ii % dim)]
MASKS = [torch.from_numpy((colour == c).astype(np.float32)).cuda() for c in range(3)]
del jj, ii, colour
res = {"width": W, "height": H, "frames_per_call": 2, "pattern": PATTERN, "warmup": WARM, "steps": STEPS, "cases": {}}


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


def rotated(fn):
    """Times of fn(Hs) for [identity, rotated] and [identity, identity], and the rotated frame alone."""
    t_rot, t_id = timed(lambda: fn(ROT)), timed(lambda: fn(IDT))
    return {"identity_plus_rotated": t_rot, "identity_twice": t_id,
            "rotated_frame_ms": round(t_rot["median_ms"] - t_id["median_ms"] / 2, 4)}


for dtype in (np.float32, np.uint16):
    fr = base.astype(dtype)
    d = torch.from_numpy(fr.view(np.int16) if dtype == np.uint16 else fr).cuda()
    name = "float32" if dtype == np.float32 else "word"
    for scale, pixfrac in ((2.0, 1.0), (1.0, 1.0)):
        ow, oh = Rg.drizzle_output_size(W, H, scale)
        out = torch.empty((2, 3, oh, ow), dtype=torch.float32, device="cuda")
        outw = torch.empty_like(out)
        mo = torch.empty((2, oh, ow), dtype=torch.float32, device="cuda")
        mw = torch.empty_like(mo)
        for kernel in ("square", "turbo", "point"):
            def fused(Hs):
                return Rg.drizzle_frames(d, Hs, 0, scale, pixfrac, kernel, out=out, out_weights=outw, ctx=ctx,
                                         cfa=PATTERN)

            def mono(Hs, pw=None):
                return Rg.drizzle_frames(d, Hs, 0, scale, pixfrac, kernel, pixel_weights=pw, out=mo, out_weights=mw,
                                         ctx=ctx)

            def masked(Hs):
                for m in MASKS:
                    mono(Hs, m)

            fused(ROT)
            tiles = Rg.drizzle_last_tiles(ctx)
            same = True
            for col, m in enumerate(MASKS):
                mono(ROT, m)
                same = same and torch.equal(mo.view(torch.int32), out[:, col].view(torch.int32)) and \
                    torch.equal(mw.view(torch.int32), outw[:, col].view(torch.int32))
            c = {"fused_cfa": rotated(fused), "mono": rotated(mono), "three_masked_mono": rotated(masked),
                 "tiles_staged_direct": tiles, "fused_equals_masked_bits": bool(same)}
            f, m1, m3 = (c[k]["rotated_frame_ms"] for k in ("fused_cfa", "mono", "three_masked_mono"))
            c["fused_over_mono"] = round(f / m1, 2)
            c["masked_over_fused"] = round(m3 / f, 2)
            res["cases"][f"{name}_{kernel}_scale{scale:g}_pixfrac{pixfrac:g}"] = c
            print(name, kernel, scale, pixfrac, json.dumps(c), flush=True)
        del out, outw, mo, mw

json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "drizzle_cfa_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

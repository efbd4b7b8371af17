"""Time find_stars on 6000x4000 star fields (HIP events), float32 and WORD:
`python scripts/star_bench.py [out.json]` (profiles/star_find_6000x4000.json).

Reported per frame: the whole call with bg / noise given (kernels, read-back
and the host sort), the candidate and measure kernels on their own
(sgpu_star_last_kernel_ms), the call with bg / noise defaulted (adds the
median and bgnoise passes), and the neighbouring single-pass frame kernels
quality_estimate and bgnoise in the same session.  The one-read HBM floor is
the frame's bytes at 8 TB/s.

`python scripts/star_bench.py --psf=gaussian|moffat [out.json]`
(profiles/star_psf_6000x4000.json) times the PSF fit of the found stars
instead: the fit kernel per frame by HIP events
(sgpu_psf_last_kernel_ms) beside the candidate pass and the moment measurement
of the same session, the whole fit_stars call, the mean of accepted
iterations per star and the statuses.  --psf=moffat fits beta as well."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siril_amd import normalization as Nm, registration as Rg, synth  # noqa: E402
from siril_amd.stacking import Context  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
PSF = ([a[6:] for a in sys.argv[1:] if a.startswith("--psf=")] or [None])[0]
if PSF not in (None, "gaussian", "moffat") or any(a.startswith("--") and not a.startswith("--psf=") for a in sys.argv[1:]):
    sys.exit("usage: star_bench.py [--psf=gaussian|moffat] [out.json]")
W, H, N = 6000, 4000, 4
WARM, STEPS = 3, 15
BG, NOISE = 0.05, 0.002
ADU = 60000.0
ctx = Context(0)
res = {"width": W, "height": H, "frames_per_call": N, "warmup": WARM, "steps": STEPS, "stars_planted": 3000,
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
        ts.append(a.elapsed_time(b) / N)
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
            "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(9 * len(ts)) // 10], 4)}


base = torch.from_numpy(synth.star_field(H, W, nstars=3000, background=BG).astype(np.float32)).cuda()
g = torch.Generator(device="cuda")
g.manual_seed(11)
fl = torch.stack([base + torch.randn((H, W), device="cuda", generator=g) * NOISE for _ in range(N)])
for name in ("float32", "word"):
    if name == "float32":
        d, bg, noise, bytes_ = fl, BG, NOISE, 4 * W * H
    else:
        d = (fl * ADU).round_().clamp_(0, 65535).to(torch.int32).to(torch.int16)     # WORD bits
        bg, noise, bytes_ = BG * ADU, NOISE * ADU, 2 * W * H
    c = {"hbm_floor_ms": round(bytes_ / 8e12 * 1e3, 4)}
    kms = []

    def call():
        Rg.find_stars(d, ctx=ctx, bg=bg, noise=noise)
        kms.append(Rg.star_last_kernel_ms(ctx))

    c["find_stars_per_frame"] = timed(call)
    k = np.array(kms[WARM:]) / N
    c["candidates_kernel_ms"] = round(float(np.median(k[:, 0])), 4)
    c["measure_kernel_ms"] = round(float(np.median(k[:, 1])), 4)
    det = {}
    stars = Rg.find_stars(d, ctx=ctx, bg=bg, noise=noise, details=det)
    c["stars_per_frame"] = [len(s) for s in stars]
    c["candidates_per_frame"] = [int(v) for v in det["ncandidates"]]
    if PSF:
        fms = []

        def fit():
            fit.out = Rg.fit_stars(d, stars, ctx=ctx, bg=bg, profile=PSF)
            fms.append(Rg.psf_last_kernel_ms(ctx))

        c["fit_stars_per_frame"] = timed(fit)
        q = np.concatenate(fit.out)
        c["profile"] = PSF
        c["fit_kernel_ms"] = round(float(np.median(np.array(fms[WARM:]) / N)), 4)
        c["fit_kernel_us_per_star"] = round(c["fit_kernel_ms"] * N * 1e3 / len(q), 4)
        c["mean_accepted_iterations"] = round(float(q["iterations"].mean()), 2)
        c["mean_samples"] = round(float(q["nused"].mean()), 1)
        c["status_counts"] = [int(v) for v in np.bincount(q["status"], minlength=7)]
        c["fit_over_candidates"] = round(c["fit_kernel_ms"] / c["candidates_kernel_ms"], 2)
        res["cases"][name] = c
        print(name, json.dumps(c), flush=True)
        continue
    c["find_stars_default_background_per_frame"] = timed(lambda: Rg.find_stars(d, ctx=ctx))
    c["quality_estimate_per_frame"] = timed(lambda: Rg.quality_estimate(d, ctx))
    c["bgnoise_per_frame"] = timed(lambda: Nm.bgnoise(ctx, d))
    c["x_hbm_floor"] = round(c["find_stars_per_frame"]["median_ms"] / c["hbm_floor_ms"], 1)
    c["candidates_x_hbm_floor"] = round(c["candidates_kernel_ms"] / c["hbm_floor_ms"], 1)
    res["cases"][name] = c
    print(name, json.dumps(c), flush=True)

json.dump(res, open(ARGS[0] if ARGS else "star_bench.json", "w"), indent=1)
ctx.close()
print("done", flush=True)

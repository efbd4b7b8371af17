"""Headless entry point: `python -m siril_amd.cli stack <seq> rej w 3 3 [-nonorm | -norm=addscale [-fastnorm]] -32b [-out=file]`
(the scripting command of Siril's siril-cli for the stacking step; see
siril_amd/sequence.py).  Prints the output path and the rejection totals.

`python -m siril_amd.cli calibrate <seq> [-bias=F | -bias="=LEVEL"] [-dark=F] [-flat=F] [-cc=dark [cold hot]]
[-cfa] [-equalize_cfa] [-opt] [-prefix=pp_]`: the calibration step (siril_amd/calibration.py); writes 32-bit
<prefix><name>NNNNN.fit and the new .seq.

`python -m siril_amd.cli register <seq> [-layer=N] [-transf=shift|similarity|affine|homography] [-minpairs=N]
[-maxstars=N] [-noout] [-interp=ne|li|cu|ar|la] [-noclamp] [-prefix=r_] [-psf=moments|gaussian|moffat]`: star-based
global registration (siril_amd/registration.py); rewrites the .seq with the homographies and, unless -noout, writes
the warped 32-bit <prefix><name>NNNNN.fit and their .seq.  -psf=gaussian|moffat measures the stars with a PSF fit.
`register <seq> -cfa=RGGB|BGGR|GBRG|GRBG|<36 letters> -noout` registers colour-filter-array mosaics: the stars are
looked for on a copy of every frame with its non-green pixels interpolated.

`python -m siril_amd.cli seqapplyreg <seq> [-layer=N] [-prefix=r_] [-interp=ne|li|cu|ar|la] [-noclamp]` applies the
homographies `register -noout` wrote, as `register`'s output stage does; `seqapplyreg <seq> -drizzle [-scale=1]
[-pixfrac=1] [-kernel=point|turbo|square] [-flat=FILE] [-layer=N] [-prefix=r_]` drizzles the frames instead: 32-bit
<prefix><name>NNNNN.fit of the scaled size, their weight planes in drizztmp/oweight_<prefix><name>NNNNN.fit, and a
.seq with the drizzle flag set.  With -cfa=RGGB|BGGR|GBRG|GRBG|<36 letters> the frames are mosaics of that pattern:
every input pixel lands in the plane of its own colour, and the frames, the weight files and the .seq have three layers.

`python -m siril_amd.cli seqsubsky <seq> <degree> [-samples=20] [-tolerance=1.0] [-nodither] [-prefix=bkg_]`: polynomial
background extraction of every frame (siril_amd/background.py), degree 1 .. 4, each layer on its own; writes 32-bit
<prefix><name>NNNNN.fit and the new .seq.  -nodither is accepted (the output is float, nothing is dithered); -rbf and
-smooth= are refused.

`python -m siril_amd.cli subsky <image> {-rbf | <degree>} [-samples=20] [-tolerance=1.0] [-smooth=0.5] [-nodither]
[-divide] [-out=FILE]`: background extraction of one image, each layer on its own: the polynomial of the given degree,
or with -rbf a thin-plate spline through the kept sample boxes, evaluated at every pixel; writes one 32-bit image,
<stem>_subsky.fit unless -out= names it.  -smooth= belongs to -rbf; -dither is refused.

`python -m siril_amd.cli wavelet <image> <nbr_layers> <type> [-prefix=]`: the a trous wavelet planes of an image
(siril_amd/wavelets.py), type 1 linear or 2 B3 spline; writes the nbr_layers planes (the details, then the residual)
as 32-bit <prefix><stem>_wavelet<k>.fit.  `python -m siril_amd.cli wrecons <image> c1 ... cn [-type=1|2] [-out=FILE]`
sharpens with them: the planes of an n-layer transform weighted by c1 .. cn and summed, in one fused pass; writes one
32-bit image, <stem>_wrecons.fit unless -out= names it.

`python -m siril_amd.cli fmedian <image> <ksize> <modulation> [-iter=N] [-out=FILE]`: the median filter
(siril_amd/filters.py) of every layer of an image: ksize x ksize windows, ksize odd in 3 .. 15, the median blended
with the sample by modulation in [0, 1], N = 1 .. 8 passes; writes one 32-bit image, <stem>_fmedian.fit unless -out=
names it.

`python -m siril_amd.cli epf <image> [-guided] [-d=N] [-si=X] [-ss=X] [-mod=X] [-guideimage=FILE] [-out=FILE]`: the
edge-preserving filter (siril_amd/filters.py) of every layer of an image: with -guided a guided filter
(eps = si^2, si in [0, 1] sample units, a d x d window, d odd in 3 .. 25 or 0 for 2 round(1.5 ss) + 1) steered by the
image itself or by -guideimage=; writes one 32-bit image, <stem>_epf.fit unless -out= names it.  Without -guided the
command means the bilateral filter, which is not built and is refused.

The stretches (siril_amd/stretch.py), each on every layer of an image, each writing one 32-bit image,
<stem>_<command>.fit unless -out= names it:
`python -m siril_amd.cli mtf <image> <low> <mid> <high> [channels] [-out=FILE]`,
`autostretch <image> [-linked] [shadowsclip [targetbg]] [-out=FILE]` (defaults -2.8 and 0.25),
`linstretch <image> -BP= [-out=FILE]`, `asinh <image> [-human] <stretch> [offset] [-out=FILE]`,
`ght <image> -D= [-B=] [-LP=] [-SP=] [-HP=] [-human|-even|-independent] [-clipmode=clip|rescale|rgbblend] [channels]
[-out=FILE]`, and `invght`, `modasinh`, `invmodasinh` with ght's options (the modasinh pair has no -B=); channels is
one of R, G, B, RG, RB, GB."""
import sys
import time


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "calibrate":
        from siril_amd.calibration import run_calibrate
        t0 = time.perf_counter()
        out, k = run_calibrate(argv)
        print(f"Calibrated to {out} in {time.perf_counter() - t0:.3f} s" +
              ("" if k is None else "; dark factors " + " ".join(f"{v:.4f}" for v in k)))
        return 0
    if argv and argv[0] == "seqsubsky":
        from siril_amd.background import run_seqsubsky
        t0 = time.perf_counter()
        out, info = run_seqsubsky(argv)
        print(f"Background extracted to {out} in {time.perf_counter() - t0:.3f} s; sample boxes kept per plane "
              f"{int(info['kept'].min())} .. {int(info['kept'].max())}")
        return 0
    if argv and argv[0] == "subsky":
        from siril_amd.background import run_subsky
        t0 = time.perf_counter()
        out, info = run_subsky(argv)
        print(f"Background extracted to {out} in {time.perf_counter() - t0:.3f} s; sample boxes kept per layer "
              + " ".join(str(int(v)) for v in info["kept"].ravel()))
        return 0
    if argv and argv[0] == "wavelet":
        from siril_amd.wavelets import run_wavelet
        t0 = time.perf_counter()
        out = run_wavelet(argv)
        print(f"Wavelet planes written to {out[0]} .. {out[-1]} in {time.perf_counter() - t0:.3f} s")
        return 0
    if argv and argv[0] == "wrecons":
        from siril_amd.wavelets import run_wrecons
        t0 = time.perf_counter()
        out = run_wrecons(argv)
        print(f"Reconstructed to {out} in {time.perf_counter() - t0:.3f} s")
        return 0
    if argv and argv[0] == "fmedian":
        from siril_amd.filters import run_fmedian
        t0 = time.perf_counter()
        out = run_fmedian(argv)
        print(f"Median filtered to {out} in {time.perf_counter() - t0:.3f} s")
        return 0
    if argv and argv[0] == "epf":
        from siril_amd.filters import run_epf
        t0 = time.perf_counter()
        out = run_epf(argv)
        print(f"Edge-preserving filtered to {out} in {time.perf_counter() - t0:.3f} s")
        return 0
    if argv and argv[0] in ("mtf", "autostretch", "linstretch", "asinh", "ght", "invght", "modasinh", "invmodasinh"):
        from siril_amd.stretch import run_stretch
        t0 = time.perf_counter()
        out = run_stretch(argv)
        print(f"Stretched ({argv[0]}) to {out} in {time.perf_counter() - t0:.3f} s")
        return 0
    if argv and argv[0] == "register":
        from siril_amd.registration import run_register
        t0 = time.perf_counter()
        out, _, info = run_register(argv)
        print(f"Registered to {out} in {time.perf_counter() - t0:.3f} s; {int(info['registered'].sum())} of "
              f"{len(info['registered'])} frames, pairs " + " ".join(str(int(v)) for v in info["npairs"]))
        return 0
    if argv and argv[0] == "seqapplyreg":
        from siril_amd.registration import run_seqapplyreg
        t0 = time.perf_counter()
        out, _, info = run_seqapplyreg(argv)
        print(f"Applied registration to {out} in {time.perf_counter() - t0:.3f} s; "
              f"{int(info['registered'].sum())} of {len(info['registered'])} frames" +
              (f", drizzled to {info['size'][0]} x {info['size'][1]}" if "size" in info else ""))
        return 0
    if not argv or argv[0] != "stack":
        print(__doc__, file=sys.stderr)
        return 2
    from siril_amd.sequence import run_command
    t0 = time.perf_counter()
    out, (lo, hi) = run_command(" ".join(argv))
    print(f"Stacked to {out} in {time.perf_counter() - t0:.3f} s; rejected low {lo}, high {hi}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

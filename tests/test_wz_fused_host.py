"""The fused kernel of the WINSORIZED moment path (stack_wz.h:
k_stack_wz_fused1) against the two kernels it replaces, on the host
(tests/hostsim/wz_fused_main.cpp): wz_prepare1 with the LDS rank store, then
wz_finish_cap, against wz_prepare1 with the HBM record store, the tile staged
as the head stages it, then wz_finish_cap -- route, WzState bytes, PixOut,
meta words, moments, c0 and every stored rank -- at N = 65, 72, 73, 100, 104,
105, 120, 121 and 128 on the split test's 14 column families, kept of 1-3 and
39-41, constant columns and walks past the 16 stored ranks.  The program is a
stand-alone host build with the address and undefined-behaviour sanitizers,
run once as its own process; it also fails when a family misses its case."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "wz_fused_main.cpp")
EXE = os.path.join(ROOT, "tests", "hostsim", "wz_fused_main")


def _build():
    csrc = os.path.join(ROOT, "siril_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("stack_sorted_impl.h", "stack_wz.h", "sgpu_kparams.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(map(os.path.getmtime, deps)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                        "-ffp-contract=off", "-I" + csrc, "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", EXE,
                        "-fsanitize=address,undefined"], check=True)
    return EXE


def test_wz_fused_matches_two_kernel_form():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "wz_fused ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

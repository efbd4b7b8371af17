"""The straight-line rank store of the fused kernel's LDS tile
(RankStore::store_full_lds, stack_wz.h) at the fused form's depth of 20 ranks
per end -- and at 18 and 16 -- against the run-time slot loops
(RankStore::store), on the host (tests/hostsim/wz_depth_main.cpp): every kept
of every real-slot bucket 72 .. 128, the R words of the lane's column bit for
bit, hi0 / mid0 / mid1, the other lanes' columns untouched, and every rank's
fetch / fetch_lo / fetch_hi.  The program is a stand-alone host build with the
address and undefined-behaviour sanitizers, run once as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "wz_depth_main.cpp")
EXE = os.path.join(ROOT, "tests", "hostsim", "wz_depth_main")


def _build():
    csrc = os.path.join(ROOT, "siril_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("stack_sorted_impl.h", "stack_wz.h", "sgpu_kparams.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(map(os.path.getmtime, deps)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                        "-ffp-contract=off", "-I" + csrc, "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", EXE,
                        "-fsanitize=address,undefined"], check=True)
    return EXE


def test_wz_depth_store_matches_slot_loops():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "wz_depth ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

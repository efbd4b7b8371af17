"""Clamp walks of the WINSORIZED moment path (stack_wz.h: wz_walk,
RankStore::fetch_lo / fetch_hi, the one-exit iteration loop of wz_round)
against a verbatim copy of the form they replace
(tests/hostsim/wz_walk_main.cpp): after every round the state bytes, the
return code and `more`, at the end route, result bits, rl, rh, nkept, pmin and
pmax, on seeded column families at N = 65, 100 and 128 -- the split test's 14,
planted clamp counts of 1, 2, 3, 4, 5 and 9 at one end, walks that leave the
stored ranks, kept of 1, 2, 3, 39, 40 and 41, constant and 16-bit columns.
The program is a stand-alone host build with the address and undefined-
behaviour sanitizers, run once as its own process; it also fails when a
planted family misses its case."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "wz_walk_main.cpp")
EXE = os.path.join(ROOT, "tests", "hostsim", "wz_walk_main")


def _build():
    csrc = os.path.join(ROOT, "siril_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("stack_sorted_impl.h", "stack_wz.h", "sgpu_kparams.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(map(os.path.getmtime, deps)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                        "-ffp-contract=off", "-I" + csrc, "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", EXE,
                        "-fsanitize=address,undefined"], check=True)
    return EXE


def test_wz_walk_matches_reference_rounds():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "wz_walk ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

"""Split rounds of the WINSORIZED moment path, restated on the host
(tests/hostsim/wz_split_main.cpp): head pass with a rounds cap, state through
memory, constants rebuilt, two tail passes -- bit for bit wz_finish's result on
seeded column families, for caps 1, 2 and 3.  The program is a stand-alone
host build with the address and undefined-behaviour sanitizers, run once as
its own process; it also fails when its columns do not exercise the resume."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "wz_split_main.cpp")
EXE = os.path.join(ROOT, "tests", "hostsim", "wz_split_main")


def _build():
    csrc = os.path.join(ROOT, "siril_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, h) for h in ("stack_sorted_impl.h", "stack_wz.h", "sgpu_kparams.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(map(os.path.getmtime, deps)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                        "-ffp-contract=off", "-I" + csrc, "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", EXE,
                        "-fsanitize=address,undefined"], check=True)
    return EXE


def test_wz_split_matches_wz_finish():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "wz_split ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

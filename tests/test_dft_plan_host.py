"""The FFT pass plan (siril_amd/csrc/fft_plan.h factorize) compiled without a
device into a stand-alone program (tests/hostsim/dft_plan_main.cpp) with
AddressSanitizer and UndefinedBehaviorSanitizer, and run once: for every
length in [2, 8192] the radix list equals the one of the factorize that still
carried the plan-shape A/B knobs (kept verbatim in the program), with both
knobs unset."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def test_dft_plan_unchanged_for_every_length(tmp_path):
    exe = str(tmp_path / "dft_plan_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostsim", "dft_plan_main.cpp"), "-o", exe], check=True)
    # the knobs of the old function are cleared by the program itself; set
    # here, they must not matter
    env = dict(os.environ, SGPU_DFT_R10="0", SGPU_DFT_PLAN="10,10")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not r.stderr.strip()
    last = r.stdout.strip().split("\n")[-1].split()
    assert last[:3] == ["dft", "plan", "ok"] and int(last[3]) == 8191
    # 0 differences: nothing but the closing line is printed
    assert r.stdout.strip().count("\n") == 0, r.stdout[:2000]
    # lengths with a plan: every prime factor <= 61 (4000 = 5 x 8 x 10 x 10 among them)
    def planned(n):
        for p in range(2, 62):
            while n % p == 0:
                n //= p
        return n == 1
    assert int(last[4]) == sum(planned(n) for n in range(2, 8193))

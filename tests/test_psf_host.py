"""The PSF fit's host side (siril_amd/csrc/psf_host.h: argument checks, list
flattening, frame table) compiled without a device into a stand-alone program
(tests/hostsim/psf_host_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, and run once."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no C++ compiler found")


def test_psf_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "psf_host_main")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "hostsim", "psf_host_main.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "psf host ok" and not r.stderr.strip()

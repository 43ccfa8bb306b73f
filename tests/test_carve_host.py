"""CPU-only: the workspace carve helper (fvgp_amd/csrc/carve.h) by itself.  tests/host/carve_test.cpp includes nothing else of the
project; it is built here with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_carve_helper_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} has no sanitizer runtime")
    exe = tmp_path / "carve_test"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SANITIZE, "-I", os.path.join(ROOT, "fvgp_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "carve_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "carve ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]

"""The offset arithmetic of the generic 3x3 / stride 2 / padding 1 convolution kernels
(ppo_amd/csrc/conv3x3s2_any_index.h) walked on the host: tests/conv3x3s2_any_index_check.cpp is compiled as an ordinary
C++ program with AddressSanitizer and UndefinedBehaviorSanitizer and run directly over the geometries
tests/test_conv3x3s2_any_gpu.py launches.  It asserts that every (m, k) of the three implicit GEMMs lands inside its
tensor or is a padding tap (exactly the taps the zero-padded stride-2 convolution defines as such), that the nine taps
of each forward output and the taps of each dx element are exactly those of a brute-force enumeration, and that the
weight-gradient slabs partition the reduction."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, cin, cout, h, w) of the INPUT: the list of tests/test_conv3x3s2_any_gpu.py (kept in step by
# test_geometry_lists_agree there)
GEOMETRIES = [
    (1, 1, 1, 1, 1), (2, 1, 2, 2, 1), (2, 2, 1, 1, 2), (3, 2, 3, 3, 4), (4, 2, 16, 5, 6), (5, 3, 5, 7, 9),
    (2, 17, 33, 5, 6), (3, 12, 16, 33, 31), (2, 16, 32, 42, 42), (2, 4, 16, 84, 84),
]


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    pytest.fail("no host C++ compiler (g++ / c++ / clang++) on PATH")


def test_index_header_walk(tmp_path):
    exe = str(tmp_path / "conv3x3s2_any_index_check")
    cxx = _host_compiler()
    # the sanitizer runtimes are linked into the program itself, so it needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-I", os.path.join(ROOT, "ppo_amd", "csrc"), os.path.join(ROOT, "tests", "conv3x3s2_any_index_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    args = [",".join(str(v) for v in g) for g in GEOMETRIES]
    run = subprocess.run([exe, *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    ok = [line for line in run.stdout.splitlines() if line.startswith("ok ")]
    assert len(ok) == len(GEOMETRIES), run.stdout
    assert all(int(line.split()[1]) > 0 for line in ok)

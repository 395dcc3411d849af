"""The offset arithmetic of the strided-convolution kernels (ppo_amd/csrc/conv_strided_index.h) walked on the host:
tests/conv_strided_index_check.cpp is compiled as an ordinary C++ program with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly over the geometries tests/test_conv_strided_gpu.py launches.  It asserts
that every (m, k) of the implicit GEMMs and every dx element lands inside its tensor, that the taps of each dx element
are exactly those of a brute-force enumeration, and that the weight-gradient slabs partition the reduction."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, cin, h, w, cout, kh, kw, stride): the three Nature layers at 84x84 (n = 3) and at the fixture's 36x36 (n = 1), a
# geometry with (h - kh) % stride != 0, one whose n*ho*wo (60) is no multiple of the 64-row tile (with a non-square
# window), and one with a single output channel
GEOMETRIES = [
    (3, 4, 84, 84, 32, 8, 8, 4), (3, 32, 20, 20, 64, 4, 4, 2), (3, 64, 9, 9, 64, 3, 3, 1),
    (1, 4, 36, 36, 32, 8, 8, 4), (1, 32, 8, 8, 64, 4, 4, 2), (1, 64, 3, 3, 64, 3, 3, 1),
    (2, 3, 15, 14, 16, 4, 4, 3), (2, 5, 11, 13, 20, 3, 2, 2), (2, 2, 9, 9, 1, 3, 3, 2),
]


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    pytest.fail("no host C++ compiler (g++ / c++ / clang++) on PATH")


def test_index_header_walk(tmp_path):
    exe = str(tmp_path / "conv_strided_index_check")
    cxx = _host_compiler()
    # the sanitizer runtimes are linked into the program itself, so it needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-I", os.path.join(ROOT, "ppo_amd", "csrc"), os.path.join(ROOT, "tests", "conv_strided_index_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    args = [",".join(str(v) for v in g) for g in GEOMETRIES]
    run = subprocess.run([exe, *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    ok = [line for line in run.stdout.splitlines() if line.startswith("ok ")]
    assert len(ok) == len(GEOMETRIES), run.stdout
    assert all(int(line.split()[1]) > 0 for line in ok)

"""csrc/resize.h under the host's sanitizers: builds tests/resize_main.cpp (a program of its own, AddressSanitizer and
UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process.  The program
drives the scaler over the cases of tests/movie_restatement.py (and an identity) on buffers of exactly the stated sizes,
with and without padded strides, and checks what the kernels rely on in every table; it must exit clean.  No GPU."""
import os
import shutil
import subprocess

import movie_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "resize_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_resize_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "resize_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and lines[-2] == "%d cases" % (len(R.CASES) + 1) and len(lines) == len(R.CASES) + 1 + 2, run.stdout
    for (w, h), (ow, oh) in R.CASES:
        assert "%d x %d -> %d x %d" % (w, h, ow, oh) in lines

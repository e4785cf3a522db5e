"""csrc/ortho.h under the host's sanitizers: builds tests/ortho_main.cpp (a program of its own, AddressSanitizer and
UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process.  The program
walks rasters whose hits lie exactly on the source's last row and column, at the camera's own position, at den == 0 and at
coordinates beyond 2^20, on buffers of exactly the stated sizes, with and without padded strides; it must exit clean.  No
GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "ortho_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
CASES = ("exact", "exact_one_sample", "exact_half_cells", "oblique_camera_inside", "oblique_near_edge", "oblique_horizon", "pole", "up", "flat", "far")


def test_ortho_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ortho_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and lines[-2] == "%d cases" % len(CASES) and len(lines) == len(CASES) + 2, run.stdout
    seen = dict(line.split(": ") for line in lines[:-2])
    assert tuple(seen) == CASES
    assert seen["exact"] == "120 of 224 seen" and seen["exact_one_sample"] == "1 of 25 seen"
    assert seen["up"].startswith("0 of") and seen["flat"].startswith("0 of") and seen["pole"].startswith("0 of")
    for name in ("exact_half_cells", "oblique_camera_inside", "oblique_near_edge", "oblique_horizon"):
        n, total = int(seen[name].split()[0]), int(seen[name].split()[2])
        assert 0 < n < total, (name, seen[name])

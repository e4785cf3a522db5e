"""csrc/map_raster.h under the host's sanitizers: builds tests/map_raster_main.cpp (a program of its own, AddressSanitizer
and UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process.  The program
walks cells, outline pairs and arrows at and beyond the coordinate limits into planes of exactly the picture's size,
asserts the hit bound of DESIGN.md 7.7 for every arrow it draws, and resolves every pixel under 16 texts of 48 characters;
it must exit clean.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "map_raster_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_map_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "map_raster_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and len(lines) == 7, run.stdout
    assert "picture 1400 x 40, 2 view(s)" in run.stdout and "picture 70 x 700, 1 view(s)" in run.stdout

"""csrc/plot_raster.h under the host's sanitizers: builds tests/plot_raster_main.cpp (a program of its own,
AddressSanitizer and UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child
process.  The program replays the background kernel's index arithmetic lane by lane on buffers of exactly the size, walks
pairs and dots at and beyond the coordinate limits into count planes of exactly Wo x Ho words, and resolves every pixel
under the longest stamp; it must exit clean.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "plot_raster_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_plot_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plot_raster_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and len(lines) == 19, run.stdout
    assert "background 4000 x 8 -> 1200 x 2" in run.stdout and "background 65535 x 2 -> 8 x 1" in run.stdout

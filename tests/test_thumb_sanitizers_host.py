"""csrc/thumb_raster.h under the host's sanitizers: builds tests/thumb_main.cpp (a program of its own, AddressSanitizer and
UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process.  The program
drives the size rule over the edges of its ranges, the host statement of the thumbnail on buffers of exactly the stated
sizes -- up to 65535-wide one-row and 65535-tall one-column images --, walks k_jpeg_thumb's decomposition lane by lane with a
column-sum array of exactly one pass, and pastes insets at the picture's edges; it must exit clean.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "thumb_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_thumbnail_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "thumb_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and len(lines) == 1 + 38 + 4 + 1, run.stdout
    assert "65535 x 1 x 3 -> 16384 x 1" in run.stdout and "1 x 65535 x 1 -> 1 x 1" in run.stdout and "picture 16384 x 3" in run.stdout

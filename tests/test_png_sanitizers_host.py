"""csrc/png_enc.h and csrc/png_enc_host.h under the host's sanitizers: builds tests/png_main.cpp (a program of its own,
AddressSanitizer and UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child
process.  The program drives the coder over the edge cases of tests/png_cases.py on buffers of exactly the stated sizes --
pictures, filtered rows, files, and files a byte short --, checks every file's frame with CRCs and an Adler-32 computed
bit by bit and byte by byte, reads every length and distance code back by RFC 1951's tables, and compares the Adler-32
by pieces with its definition; it must exit clean.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "png_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_png_coder_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "png_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and lines[-2] == "24 pictures" and len(lines) == 24 + 2 + 2, run.stdout
    assert "pitch 32767: 10922 x 2, N 65534" in run.stdout and "1 x 16384: 1 x 16384, N 65536" in run.stdout

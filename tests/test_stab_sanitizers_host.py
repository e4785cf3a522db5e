"""csrc/stab.h under the host's sanitizers: builds tests/stab_main.cpp (a program of its own, AddressSanitizer and
UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process.  The program
runs the host statement on tables, flags, working arrays and results of exactly the stated sizes -- every table length and
vertex count of the catalogue, anchor counts on both sides of every length at which np_sum changes strategy, scattered and
coincident anchors, NaN and infinity in the table's last floats, out of place and in place -- walks the leaf machine over
every chunk length, and flags coordinates on and beyond every edge of a mask; it must exit clean.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "stab_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
CASES = 20 + 26 + 4 + 2


def test_stab_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stab_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and lines[-2] == "%d cases" % CASES and len(lines) == CASES + 2, run.stdout
    seen = dict(line.split(": ") for line in lines[:-2])
    assert seen["na9 model1"].startswith("status 1,") and seen["na10 model0"].split(",")[0] in ("status 0", "status 2")
    assert seen["na16400 model1"].startswith("status 0, at least") and seen["one-point model1"] == "status 4"
    assert int(seen["scatter model0"].split()[1]) & 2 and 1 < int(seen["walk"].split()[2]) <= 128 and int(seen["flags"].split()[0]) > 10

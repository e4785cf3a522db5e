"""csrc/drift.h under the host's sanitizers: builds tests/drift_main.cpp (a program of its own, AddressSanitizer and
UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child process on the catalogue's
binary dump (tests/drift_cases.py) with the numpy restatement's results beside every case.  The program runs the host statement
on arrays of exactly the stated sizes, must reproduce every result bit for bit and exit clean.  No GPU."""
import os
import shutil
import subprocess

import drift_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "drift_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_drift_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    cases = DC.catalogue()
    dump = tmp_path / "catalogue.bin"
    dump.write_bytes(DC.dump(cases, [DC.expected(c) for c in cases]))
    exe = str(tmp_path / "drift_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and lines[-2] == "%d cases" % len(cases) and len(lines) == len(cases) + 3, run.stdout
    stages = [k for k, c in enumerate(cases) if c["name"] == "stages"][0]
    assert lines[stages].endswith("4 drifters, 1 steps, order 4, 1 alive"), lines[stages]
    tide = [k for k, c in enumerate(cases) if c["name"].startswith("tide_33x65_m18")][0]
    assert lines[tide].startswith("case %d: tide, 33 x 65 nodes, 1000 drifters" % tide), lines[tide]

"""The budgeted chain of a crop job (csrc/jpeg_enc_host.h: encode_budgeted_host, on the decisions of csrc/jpeg_enc.h that
the device-sized kernels take) under the host's sanitizers: builds tests/jpeg_enc_budget_main.cpp (a program of its own,
AddressSanitizer and UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a child
process.  The program walks the chain in the kernels' order with `packed` and `out` buffers of exactly the capacity, over
scans that fit, scans that overflow at each of the two exits, a coefficient without a code and arbitrary control words; it
must exit clean.  No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "jpeg_enc_budget_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_budgeted_chain_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_enc_budget_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.rstrip().splitlines()
    assert lines[-1] == "done" and len(lines) == 9, run.stdout
    # the fixture of the exit behind the FF count is the one the GPU test uses, and both exits were taken
    assert "stripes 200 x 9 quality 95: 78 blocks, packed 980, stuffed 1026, 14 per block" in run.stdout
    behind = [int(m) for m in re.findall(r"behind the FF count (\d+)", run.stdout)]
    over = [int(m) for m in re.findall(r"over (\d+) \(", run.stdout)]
    assert sum(behind) >= 2 and sum(over) - sum(behind) >= 8, run.stdout

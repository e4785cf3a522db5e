"""csrc/lk_uniform_math.h on the device, exhaustively: builds tests/recip_exact_main.hip (a program of its own) and runs it as a
child process under a time limit.  recip_exact must be __fdiv_rn(1.f, x), bit for bit, for every float from 2^-23 (the
tracker's `D < FLT_EPSILON` test has failed) to 2^32 (every window sum is below 2^36 and carries 2^-20:
tests/test_lk_limits.py), and the one-instruction floor must be (int)floorf(x) for every float that is not a NaN (what the
tracker makes of a NaN point is tests/test_gpu_lk_floors.py's matter)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "recip_exact_main.hip")
CSRC = os.path.join(ROOT, "iceberg_tracking_code_amd", "csrc")


@pytest.mark.gpu
def test_reciprocal_and_floor_are_exact_for_every_float(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "recip_exact_main")
    # the library's own flags (build.py): -ffp-contract=off, so that the helper's fma are the only fused operations
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC,
                    SOURCE, "-o", exe], check=True, timeout=300)
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"reciprocal: bits 0x34000000 \.\. 0x4f800000 \(2\^-23 \.\. 2\^32\), (\d+) values, mismatches (\d+)", run.stdout)
    assert m and int(m.group(1)) == 0x4f800000 - 0x34000000 + 1 and int(m.group(2)) == 0, run.stdout
    m = re.search(r"floor: bits 0x00000000 \.\. 0xffffffff without the NaNs, 4278190082 values, mismatches (\d+)", run.stdout)
    assert m and int(m.group(1)) == 0, run.stdout


def test_range_is_the_one_the_tracker_can_reach():
    """No GPU: the header's range constants are 2^-23 and 2^32, and 2^32 bounds D for the largest sums of the limits test."""
    import numpy as np
    text = open(os.path.join(CSRC, "lk_uniform_math.h")).read()
    lo = int(re.search(r"RECIP_LO_BITS = (0x[0-9a-f]+)u", text).group(1), 16)
    hi = int(re.search(r"RECIP_HI_BITS = (0x[0-9a-f]+)u", text).group(1), 16)
    assert np.array([lo, hi], np.uint32).view(np.float32).tolist() == [2.0 ** -23, 2.0 ** 32]
    # A11, A22 < 2^36 * 2^-20 (35 x 35 pixels of 4080^2, FLT_SCALE): D = A11 A22 - A12^2 <= A11 A22 < 2^32
    top = 35 * 35 * 4080 * 4080
    assert top < 2 ** 36 and (top / 2.0 ** 20) ** 2 < 2.0 ** 32

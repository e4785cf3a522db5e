"""Cases for tests/np_sums_main.cpp (csrc/np_sums.h and csrc/cube_means.h on the host), the program's build and its file
format, and the orders of addition the tests tell apart.  Shared by test_np_sums_host.py and
test_np_sums_sanitizers_host.py; no GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "np_sums_main.cpp")

# ---- the lengths of a contiguous sum -------------------------------------------------------------------------------------
SUM_LENGTHS = list(range(1101)) + [2047, 2048, 2049, 4095, 4096, 4103, 4104, 8191, 8192, 8193, 16385, 100003]
SUM_SEED = 7


def sum_values(n, attempt):
    """n values over seven decades, so that the order of the additions shows in the bits."""
    rng = np.random.default_rng([SUM_SEED, n, attempt])
    return rng.normal(size=n) * 10.0 ** rng.integers(-4, 3, n)


def sum_case(n):
    """The values of length n: the first draw that tells numpy's order from a wrong one (about one draw in twenty
    gives the same bits either way, more among the shortest).  Below 16 terms there is nothing to choose by."""
    for attempt in range(64):
        x = sum_values(n, attempt)
        if n < 16 or tells_orders_apart(x):
            return x
    raise AssertionError("no draw of %d values tells the orders apart" % n)


def left_to_right(x):
    """A wrong order: one term after the other (np.add.accumulate is the plain loop)."""
    return float(np.add.accumulate(np.concatenate([[0.0], x]))[-1])


def _leaf(x):
    n = len(x)
    if n < 8:
        return left_to_right(x)
    r = x[:8].copy()
    whole = n - n % 8
    for t in range(8, whole, 8):
        r += x[t:t + 8]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for t in range(whole, n):
        res += x[t]
    return res


def unaligned_pairwise(x):
    """A wrong order: numpy's pairwise routine with the halves of a long run not aligned to 8 terms."""
    n = len(x)
    if n <= 128:
        return _leaf(x)
    return unaligned_pairwise(x[:n // 2]) + unaligned_pairwise(x[n // 2:])


def one_run_pairwise(x):
    """A wrong order beyond 8192 terms: numpy's pairwise routine over the whole run at once, as if the reduction were
    not buffered."""
    n = len(x)
    if n <= 128:
        return _leaf(x)
    half = n // 2 - (n // 2) % 8
    return one_run_pairwise(x[:half]) + one_run_pairwise(x[half:])


def tells_orders_apart(x):
    """np.sum(x) differs in its bits from at least one of the two wrong orders, left to right and halves not aligned
    to 8 -- and beyond the 8192 elements of numpy's buffer also from the single pairwise run."""
    want = float(np.sum(x))
    if len(x) > 8192 and float(0.0 + one_run_pairwise(x)) == want:
        return False
    return left_to_right(x) != want or float(0.0 + unaligned_pairwise(x)) != want


# ---- the geometries of spatial_mean: (rows, cols, c) -----------------------------------------------------------------------
SHAPES = [(1, 1), (1, 40), (40, 1), (3, 3), (23, 5), (5, 23), (37, 5), (100, 7), (7, 100), (33, 33), (9, 14), (101, 89),
          (300, 2), (2, 300), (130, 17), (17, 130), (64, 64), (20, 260)]
COARSENESS = [2, 3, 5, 7, 8, 9, 12, 16, 17, 33, 64, 90, 91, 96, 127, 128, 129, 140, 300]
GEOMETRIES = [(r, c_, c) for r, c_ in SHAPES for c in COARSENESS]
GEOMETRIES += [g for c in (90, 91, 127, 128, 129, 181, 182, 513) for g in ((c + 3, c - 1, c), (2 * c + 5, c - 1, c))]
GEOMETRIES += [(2, 2 * c + 7, c) for c in (8192, 8193)]          # at least two coarse columns, rows of > 8192 terms
# the largest of them: the longest single run (513 * 513 terms), the longest rows, the widest and the tallest field
LARGEST = [(516, 512, 513), (1031, 512, 513), (2, 2 * 8193 + 7, 8193), (101, 89, 300), (20, 260, 300), (300, 2, 300),
           (94, 90, 91), (300, 2, 129), (1, 1, 2), (23, 5, 8)]


def field(rows, cols, nan_share, seed):
    rng = np.random.default_rng([seed, rows, cols])
    a = rng.normal(0.1, 0.3, (rows, cols)) * 10.0 ** rng.integers(-3, 2, (rows, cols))
    if nan_share:
        a[rng.random((rows, cols)) < nan_share] = np.nan
    return a


def spatial_mean_numpy(a, c):
    """Blocks of c x c cells averaged with np.mean after zero padding to a multiple of c; the padded cells count."""
    rows, cols = a.shape
    pr, pc = -(-rows // c) * c, -(-cols // c) * c
    padded = np.zeros((pr, pc))
    padded[:rows, :cols] = a
    return np.mean(padded.reshape(pr // c, c, pc // c, c), axis=(1, 3))


# ---- the program -------------------------------------------------------------------------------------------------------------

def build(tmp_path, extra_flags=("-O2",)):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "np_sums_main")
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off"] + list(extra_flags) + [SOURCE, "-o", exe], check=True)
    return exe


def run(exe, tmp_path, cases, timeout=300):
    """cases: ("sum", x) or ("mean", field, c).  Returns the program's results in the same order: (np_sum, 0.0 +
    np_pairwise_sum) for a sum, the coarse field for a mean."""
    src, dst = os.path.join(str(tmp_path), "cases.bin"), os.path.join(str(tmp_path), "results.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for case in cases:
            if case[0] == "sum":
                f.write(struct.pack("<ii", 0, len(case[1])))
                f.write(np.ascontiguousarray(case[1], "<f8").tobytes())
            else:
                f.write(struct.pack("<iiii", 1, case[1].shape[0], case[1].shape[1], case[2]))
                f.write(np.ascontiguousarray(case[1], "<f8").tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().splitlines()[-1] == "done", done.stdout
    flat = np.fromfile(dst, "<f8")
    out, at = [], 0
    for case in cases:
        if case[0] == "sum":
            out.append((flat[at], flat[at + 1]))
            at += 2
        else:
            rows, cols = case[1].shape
            cr, cc = -(-rows // case[2]), -(-cols // case[2])
            out.append(flat[at:at + cr * cc].reshape(cr, cc))
            at += cr * cc
    assert at == len(flat)
    return out, done.stdout

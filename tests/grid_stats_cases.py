"""Value families and lengths for the per-cell statistics (csrc/grid_stats.h), the build of tests/grid_stats_main.cpp and
its file format, and the comparison rule.  Shared by test_grid_stats_host.py and test_gpu_grid_stats.py."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "grid_stats_main.cpp")

LENGTHS = list(range(1, 301)) + [2047, 2048, 8191, 8192, 8193, 9000, 16384, 20000, 100003]


def _decades(rng, n):
    return rng.normal(size=n) * 10.0 ** rng.integers(-5, 5, n)


def _all_equal(rng, n):
    return np.full(n, rng.normal() * 3.7)


def _low_byte(rng, n):
    """one value whose mantissa's lowest byte varies: the radix select decides in its last pass"""
    base = np.array([0.1234567], np.float64).view(np.uint64)[0] & ~np.uint64(0xff)
    return (base | rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)


def _sign_or_exponent(rng, n):
    """one mantissa; sign and exponent vary: the select decides in its first two passes"""
    return np.ldexp(1.2345678901234567, rng.integers(-40, 40, n)) * rng.choice([-1.0, 1.0], n)


def _straddle(rng, n):
    """the two middle terms are equal duplicates and their neighbours are not"""
    a = np.sort(_decades(rng, n))
    if n >= 4:
        a[n // 2] = a[n // 2 - 1]
        if n >= 6:
            a[n // 2 + 1] = a[n // 2 - 1]
    return rng.permutation(a)


def _mixed(rng, n):
    return rng.normal(0.2, 0.4, n)


FAMILIES = dict(decades=_decades, all_equal=_all_equal, low_byte=_low_byte, sign_or_exponent=_sign_or_exponent,
                straddle=_straddle, mixed=_mixed)


def values(family, n, seed=5):
    return np.ascontiguousarray(FAMILIES[family](np.random.default_rng([seed, n, sorted(FAMILIES).index(family)]), n))


def family_of(n):
    """every length gets one family, in turn"""
    names = sorted(FAMILIES)
    return names[n % len(names)]


def special_cases():
    inf, nan = np.inf, np.nan
    out = [[-0.0], [0.0], [-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0, 0.0],
           [inf], [-inf], [-inf, inf], [inf, inf], [-inf, -inf, 1.0], [1.0, inf, 2.0, -inf], [1.0, 2.0, inf, inf],
           [1e308, 1e308], [1e308, 1e308, 1e308], [-1e308, 1e308], [5e-324, 0.0, -5e-324],
           [nan], [nan, 1.0], [1.0, nan]]
    rng = np.random.default_rng(3)
    for n in (3, 8, 9, 129, 300):
        for place in (0, n // 2, n - 1):
            a = _decades(rng, n)
            a[place] = nan
            out.append(a)
    return [np.array(a, np.float64) for a in out]


def same(got, want):
    """bit for bit, except that a NaN equals a NaN of any sign and payload"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def build(tmp_path, extra_flags=("-O2",)):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "grid_stats_main")
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off"] + list(extra_flags) + [SOURCE, "-o", exe], check=True)
    return exe


def run(exe, tmp_path, segments, timeout=300):
    """segments: float64 arrays.  Returns (n, 5): std, median, mad, the lower (or only) middle term and the count of
    terms <= it (both 0 when the segment is empty or holds a NaN), and the program's output."""
    src, dst = os.path.join(str(tmp_path), "segments.bin"), os.path.join(str(tmp_path), "stats.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(segments)))
        for a in segments:
            f.write(struct.pack("<i", len(a)))
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().splitlines()[-1] == "done", done.stdout
    return np.fromfile(dst, "<f8").reshape(len(segments), 5), done.stdout

"""csrc/corner_keys.h -- the response key, the 64-bit candidate key and the quality threshold that the corner detector's
sources (k_corners.hip, k_corners_fast.hip, k_min_distance.hip, k_tail.hip) share -- run on the host
(tests/corner_keys_main.cpp, a program of its own built with the host compiler and -ffp-contract=off) and compared with
numpy, bit for bit.  No GPU, no tolerance."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import strip_arm_frames as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "corner_keys_main.cpp")

FLT_MIN, FLT_MAX, INF = 0x00800000, 0x7f7fffff, 0x7f800000
SIGN = 0x80000000
NAMED = [b | s for b in (0, 1, FLT_MIN, 0x3f800000, FLT_MAX, INF) for s in (0, SIGN)]   # 0, denormal, FLT_MIN, 1, FLT_MAX, inf
XY = (0, 1, 255, 256, 65535)
QUALITIES = (0.0, 0.007, 0.01, 1.0)


def patterns():
    """the named bit patterns and 4000 random ones, NaNs excluded"""
    rng = np.random.default_rng(20)
    r = rng.integers(0, 1 << 32, 6000, dtype=np.uint64).astype(np.uint32)
    r = r[(r & 0x7fffffff) <= INF][:4000]
    assert len(r) == 4000
    return np.concatenate([np.array(NAMED, np.uint32), r])


def responses():
    """a dozen responses between 1e-12 and 1"""
    return np.array([1e-12, 3.3e-11, 7e-10, 2.5e-8, 1e-6, 4.4e-5, 1e-3, 0.0123, 0.1, 0.25, 0.7, 1.0], np.float32)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("corner_keys"))
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe, src, dst = (os.path.join(tmp, n) for n in ("corner_keys_main", "cases.bin", "results.bin"))
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-O2", SOURCE, "-o", exe], check=True)
    bits = patterns()
    packs = [(int(b), x, y) for b in (0x3f800000, 0x00000001, 0xbf800000) for x in XY for y in XY]
    thresholds = [(0, q) for q in QUALITIES] + [(F.ordered_key(v), q) for v in responses() for q in QUALITIES]
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(bits)) + bits.astype("<u4").tobytes())
        f.write(struct.pack("<i", len(packs)) + b"".join(struct.pack("<Iii", *p) for p in packs))
        f.write(struct.pack("<i", len(thresholds)) + b"".join(struct.pack("<Id", *t) for t in thresholds))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0 and done.stdout.rstrip().splitlines()[-1] == "done", done.stdout + done.stderr
    out = np.fromfile(dst, "<u4")
    a, b = 2 * len(bits), 2 * len(bits) + 6 * len(packs)
    assert len(out) == b + len(thresholds)
    return dict(bits=bits, keys=out[:a].reshape(-1, 2), packs=packs, packed=out[a:b].reshape(-1, 6), thresholds=thresholds,
                thr=out[b:])


def test_key_is_the_numpy_statement_and_key_to_float_inverts_it(results):
    bits, keys = results["bits"], results["keys"]
    want = np.array([F.ordered_key(v) for v in bits.view(np.float32)], np.uint32)
    assert np.array_equal(keys[:, 0], want)
    assert np.array_equal(keys[:, 1], bits)      # back to the very bits, -0 and the denormals included
    assert (keys[:, 0] != 0).all()               # 0 is below every float


def test_key_order_is_float_order_with_minus_zero_below_plus_zero(results):
    bits, keys = results["bits"], results["keys"][:, 0].astype(np.int64)
    values = bits.view(np.float32).astype(np.float64)
    order = np.argsort(keys, kind="stable")
    v, b = values[order], bits[order]
    assert (np.diff(v) >= 0).all()               # keys ascending => floats never descending
    ties = np.flatnonzero((np.diff(v) == 0) & (np.diff(keys[order]) != 0))
    assert len(ties) == 1 and b[ties[0]] == SIGN and b[ties[0] + 1] == 0      # the one pair of equal floats with two keys
    # and the other way round: a larger float has a larger key
    by_value = np.argsort(values, kind="stable")
    assert (np.diff(keys[by_value])[np.diff(values[by_value]) > 0] > 0).all()


def test_candidate_key_round_trips_and_orders_like_the_raster_address(results):
    packs, got = results["packs"], results["packed"]
    for (b, x, y), (lo, hi, rk, gx, gy, xy) in zip(packs, got):
        rkey = F.ordered_key(np.array([b], np.uint32).view(np.float32)[0])
        assert (int(hi), int(rk), int(gx), int(gy)) == (rkey, rkey, x, y), (b, x, y)
        assert int(lo) == int(xy) == (y << 16) | x
    w = 65536
    for b in {p[0] for p in packs}:
        same = [(int(hi) << 32 | int(lo), y * w + x) for (pb, x, y), (lo, hi, *_rest) in zip(packs, got) if pb == b]
        assert len(same) == len(XY) ** 2
        assert [a for _, a in sorted(same)] == sorted(a for _, a in same)      # key order == raster order, no ties
        assert len({k for k, _ in same}) == len(same)


def test_threshold_is_the_float_of_the_double_product(results):
    seen = 0
    for (max_key, q), got in zip(results["thresholds"], results["thr"]):
        if max_key == 0:
            assert got == 0, q                    # +0.0: no maximum published
            continue
        response = next(v for v in responses() if F.ordered_key(v) == max_key)
        want = np.float32(np.float64(response) * q)
        assert got == want.view(np.uint32), (response, q)
        seen += 1
    assert seen == len(responses()) * len(QUALITIES)

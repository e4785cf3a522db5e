"""The lanes' functions of csrc/jpeg_lanes.h from states that are not the true ones, under the host's sanitizers: builds
tests/jpeg_lanes_states.cpp (a program of its own, with AddressSanitizer and UndefinedBehaviorSanitizer linked
statically, nothing of the library in it) and runs it as a child process on every catalogue stream, the photos and the
damaged files.  The asynchronous ingest relies on what this shows: on a file that does not settle, scan, write and DC
pass run on untrue entry states and must neither store outside the coefficients, read outside the file, nor hang.
No GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import time

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_streams as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "jpeg_lanes_states.cpp")
SUBSEQ = (32, 512)          # the program runs both
PAIRS = 4                   # arbitrary (state, first block) pairs per lane
GENEROUS = dict(max_hops=256, max_rounds=255)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _files():
    from test_gpu_jpeg_async import _damaged
    files = [(s.label, s.data) for s in js.catalogue()]
    files += [("photo 120x88 s%d" % s, jc.encode(jc.photo(120, 88, 21), quality=85, subsampling=s)) for s in (0, 1, 2)]
    return files, _damaged()[1]


def _blob(data):
    """what jpeg_lanes_states.cpp reads (Blob::load), from icelk_jpeg_index; None where that call does not take the file"""
    from iceberg_tracking_code_amd import _lib as L
    lib = L.load()
    info, scan = L.JpegInfo(), L.JpegScan()
    if lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, None) != 0:
        return None, None
    n = scan.segments
    begin, end = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    tables = (C.c_uint8 * L.JPEG_TABLE_BYTES)()
    assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), begin, end, n, tables) == 0
    head = [len(data), n, scan.blocks_per_mcu, scan.blocks_per_segment, scan.total_blocks, info.mcus_x, info.mcus_y, info.hmax, info.vmax,
            info.blocks_x[0], info.blocks_x[1], info.coef_offset[0], info.coef_offset[1], info.coef_offset[2], info.coef_count, info.ncomp]
    head += list(scan.component) + list(scan.dc_table) + list(scan.ac_table)
    lanes = {S: sum(max(1, -(-(end[s] - begin[s]) * 8 // S)) for s in range(n)) for S in SUBSEQ}
    return struct.pack("<%dQ" % len(head), *head) + bytes(begin) + bytes(end) + bytes(tables) + bytes(data), lanes


def _build(tmp_path, source=SOURCE, opt="-O1"):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_lanes_states")
    subprocess.run([cxx, "-std=c++17", opt, "-g", "-fno-omit-frame-pointer"] + SANITIZE + [source, "-o", exe], check=True)
    return exe


def test_lanes_from_arbitrary_states_under_sanitizers(tmp_path):
    from iceberg_tracking_code_amd import read_jpeg_lanes
    t0 = time.monotonic()
    exe = _build(tmp_path)
    t_build = time.monotonic() - t0
    good, damaged = _files()
    blobs, expected = [], 0
    for k, (label, data) in enumerate(good + damaged):
        blob, lanes = _blob(data)
        if blob is None:
            assert k >= len(good), label       # only a damaged file may be refused by the index
            continue
        path = str(tmp_path / ("%02d.blob" % k))
        with open(path, "wb") as f:
            f.write(blob)
        blobs.append((label, data, path, k < len(good)))
        # per S: write_lane once per lane in steps 1 and 2, PAIRS times write_lane and decode<false> in step 3
        expected += sum(lanes[S] * (2 + 2 * PAIRS) for S in SUBSEQ)
    assert len(blobs) >= len(good) >= 37
    t0 = time.monotonic()
    run = subprocess.run([exe, str(PAIRS)] + [p for _, _, p, _ in blobs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    t_run = time.monotonic() - t0
    out, err = run.stdout.decode(), run.stderr.decode()
    print(out)
    print("build %.1f s, run %.1f s, %d files, %d calls expected" % (t_build, t_run, len(blobs), expected))
    assert run.returncode == 0, (run.returncode, err[:4000])
    lines = out.strip().splitlines()
    assert len(lines) == len(blobs) * len(SUBSEQ) + 2
    assert lines[-1] == "calls %d" % expected, (lines[-1], expected)
    drawn = [int(v) for v in lines[-2].split()[1:]]
    assert len(drawn) == 8 and all(v > 0 for v in drawn), drawn      # every kind of p, kNoState, every kind of `first`
    # step 1 made the coefficients of the library's own CPU statement: the rebuilt Scan and segment table are the device's
    compared = 0
    for label, data, path, is_good in blobs:
        for S in SUBSEQ:
            try:
                j, st = read_jpeg_lanes(data, S, **GENEROUS)
            except ValueError:
                assert not is_good, label
                continue
            if is_good:
                assert st["fallback"] == 0, (label, S, st)
            elif st["fallback"] != 0:
                continue
            got = np.fromfile("%s.S%d.coef" % (path, S), np.int16)
            assert got.shape == j.coef.shape and np.array_equal(got, j.coef), (label, S, int(np.count_nonzero(got != j.coef)))
            compared += 1
    assert compared >= len(good) * len(SUBSEQ)

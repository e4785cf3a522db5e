"""The host statement of the fused crop-and-forward kernel (csrc/jpeg_crop_fwd_host.h: csrc/jpeg_rgb.h at the crop box of
the decoded planes, then the forward statement of csrc/jpeg_resave_host.h) under the host's sanitizers: builds
tests/jpeg_crop_fwd_host_main.cpp (a program of its own, AddressSanitizer and UndefinedBehaviorSanitizer linked statically,
nothing of the library in it), runs it as a child process on planes exactly as large as the library allocates them
(8 x blocks in both directions), and compares its coefficients with `read_jpeg` of Pillow's cropped file and with the numpy
statement built from jpeg_restatement.py and jpeg_resave_restatement.py.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_crop_fwd_cases as cc
import jpeg_restatement as jr
import jpeg_resave_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "jpeg_crop_fwd_host_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _planes(data):
    """(info, the three component planes at 8 x blocks in both directions, chroma mode): what k_jpeg_idct leaves"""
    from iceberg_tracking_code_amd import read_jpeg
    j = read_jpeg(data)
    i = j.info
    planes = [jr._plane(jr.idct_blocks(j.blocks(c), j.quant(c))) for c in range(3)]
    sub_x, sub_y, fancy = i.hmax == 2, i.vmax == 2, i.comp_w[1] > 2
    mode = 0 if not sub_x else ((2 if fancy else 4) if sub_y else (1 if fancy else 3))
    return i, planes, mode


def _numpy_rgb(i, planes, mode):
    """the decoded image by jpeg_restatement.py from the same planes"""
    w, h = i.width, i.height
    hs, vs = i.hmax, i.vmax
    cb, cr = (jr.upsample(p[:i.comp_h[1], :i.comp_w[1]], hs, vs, mode in (1, 2))[:h, :w] for p in planes[1:])
    return jr.to_rgb(planes[0][:h, :w], cb, cr)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("crop_fwd") / "jpeg_crop_fwd_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    return exe


def test_host_statement_under_sanitizers(program, tmp_path):
    from iceberg_tracking_code_amd import read_jpeg
    decoded, blobs, want = {}, [], []
    for k, (label, data, size, box, q) in enumerate(cc.cases()):
        if data not in decoded:
            i, planes, mode = _planes(data)
            decoded[data] = (i, planes, mode, _numpy_rgb(i, planes, mode))
        i, planes, mode, rgb = decoded[data]
        left, top, bw, bh = box
        head = [i.width, i.comp_w[1], i.comp_h[1], mode] + [p.shape[1] for p in planes] + [p.shape[0] for p in planes] + \
               [left, top, bw, bh, 75 if q is None else q, 0]
        path = str(tmp_path / ("case%d.blob" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<16i", *head) + b"".join(np.ascontiguousarray(p).tobytes() for p in planes))
        blobs.append(path)
        pillow = read_jpeg(cc.pillow_crop_file(data, box, q)).coef
        restated = np.concatenate([p.ravel() for p in rr.coefficients(rgb[top:top + bh, left:left + bw], 75 if q is None else q)[1]])
        want.append((label, pillow, restated))
    run = subprocess.run([program] + blobs, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    for path, (label, pillow, restated) in zip(blobs, want):
        got = np.fromfile(path + ".coef", np.int16)
        assert got.shape == pillow.shape and np.array_equal(got, pillow), (label, int(np.count_nonzero(got != pillow)))
        assert np.array_equal(got, restated), label

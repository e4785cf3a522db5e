"""The host statement of the JPEG writer (csrc/jpeg_enc_host.h on csrc/jpeg_enc.h) under the host's sanitizers: builds
tests/jpeg_enc_host_main.cpp (a program of its own, AddressSanitizer and UndefinedBehaviorSanitizer linked statically,
nothing of the library in it), runs it as a child process on images whose buffers -- pixels, coefficients, header, file --
are exactly as large as the calls are told or report, and compares the files it wrote with the library's and with Pillow's.
No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np

import jpeg_resave_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "jpeg_enc_host_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
# (width, height, quality, bytes a row is longer than its pixels)
CASES = ((1, 1, 75, 0), (3, 3, 75, 1), (16, 17, 75, 0), (17, 33, 1, 5), (41, 7, 100, 0), (33, 16, 20, 2), (99, 131, 75, 0), (250, 333, 95, 3))


def test_host_writer_under_sanitizers(tmp_path):
    from iceberg_tracking_code_amd import resave_bytes
    from PIL import Image
    import io
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_enc_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE + [SOURCE, "-o", exe], check=True)
    blobs, images = [], []
    for k, (w, h, q, extra) in enumerate(CASES):
        kind = rc.CONTENTS[k % len(rc.CONTENTS)] if k else "full"        # noise, the saturated extremes and stripes among them
        rgb = rc.content(kind, w, h, seed=k)
        rows = np.zeros((h, 3 * w + extra), np.uint8)
        rows[:, :3 * w] = rgb.reshape(h, 3 * w)
        path = str(tmp_path / ("case%d.blob" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<4i", w, h, rows.strides[0], q) + rows.tobytes())
        blobs.append(path)
        images.append((rgb, q))
    run = subprocess.run([exe] + blobs, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "extremes:" in run.stdout and run.stdout.rstrip().endswith("done")
    n = len(CASES) + 1     # every case's file and the extremes', through the file assembler at exactly and one short of its length
    assert "assembled: %d of %d" % (n, n) in run.stdout
    for path, (rgb, q) in zip(blobs, images):
        with open(path + ".jpg", "rb") as f:
            got = f.read()
        assert got == resave_bytes(rgb, q, comment=b"blob"), path
        f = io.BytesIO()
        Image.fromarray(rgb).save(f, "JPEG", quality=q, comment=b"blob")
        assert got == f.getvalue(), path

"""What an orthophoto costs (profiles/ortho.txt is one run's output), at a real size: one 3456 x 2304
Pillow-written JPEG (4:2:0, quality 90) of the full-size camera onto a 2000 x 1500 raster of 2 m that straddles the near
edge of its footprint.  After three warm-up rounds, REPEATS rounds of begin + add_jpeg_file (+ write as a PNG in the
second table): the host clock around the calls, each of which ends in a wait for the device -- median, min, max -- and the
per-kernel times of the profiling table (HIP events) over the same rounds: the decoder's kernels, ortho_fill and
ortho_add.  From the bytes ortho_add moves per pixel (one `best` load, at most four 3-byte samples, 12 bytes stored where
the pixel changes) its rate is printed beside the time; it is a gather, so the rate is a floor of what the memory system
did, not a share of its peak.  Then the host statement on the same inputs, one core, for scale, and the bytes compared.
Needs an MI355X.

    python tools/ortho_bench.py [output file]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import jpeg_cases as jc
from iceberg_tracking_code_amd import CameraModel, Context, orthophoto_host

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
REPEATS, WARM = 20, 3
W, H = 3456, 2304
E0, N0 = 497812.37, 6521034.81


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def med(v):
    return "median %.3f ms (min %.3f, max %.3f) of %d" % (statistics.median(v), min(v), max(v), len(v))


camera = CameraModel(image_width=W, image_height=H, sensor_width=22.3, easting=E0, northing=N0, elevation=431.62, antenna_height=1.35,
                     theta=201.4, phi=11.85, psi=1.27, sigma=24.6)
raster = dict(x0=E0 - 3600.0, y0=N0 + 800.0, res=2.0, width=2000, height=1500)
photo = jc.photo(W, H, 3)
data = jc.encode(photo, quality=90, subsampling=2)
pixels = jc.pil_decode(data)
say("source %d x %d JPEG 4:2:0 quality 90, %d bytes; raster %d x %d of %g m" % (W, H, len(data), raster["width"], raster["height"], raster["res"]))

ctx = Context(64, 64, n_slots=1, max_pts=1024)
kernels = ("jpeg_huff", "jpeg_idct", "jpeg_out", "ortho_fill", "ortho_add")


def round_of(write):
    ctx.ortho_begin(raster)
    t0 = time.perf_counter()
    ctx.ortho_add(camera, 0, data)
    t1 = time.perf_counter()
    result = ctx.ortho_write("png") if write else None
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), result


for write in (False, True):
    for _ in range(WARM):
        _, _, last = round_of(write)
    ctx.prof_reset()
    ctx.prof_enable(True)
    t_add, t_write = [], []
    for _ in range(REPEATS):
        a, w, last = round_of(write)
        t_add.append(a)
        t_write.append(w)
    ctx.prof_enable(False)
    say("begin + add_jpeg_file%s, %d rounds after %d warm-up rounds" % (" + write (PNG)" if write else "", REPEATS, WARM))
    say("  add_jpeg_file (decode + ortho_add + wait), host clock: " + med(t_add))
    if write:
        say("  write (PNG coded on the device, R G B and cover to the host), host clock: " + med(t_write))
        say("  the PNG: %d bytes" % len(last["file"]))
    table = ctx.prof_table()
    say("  per kernel (HIP events around each launch, mean over the rounds):")
    for k in kernels:
        if k in table:
            say("    %-12s launches %4d  avg %9.1f us" % (k, table[k]["launches"], table[k]["avg_us"]))

final = ctx.ortho_write()
seen = int(np.count_nonzero(final["cover"]))
px = raster["width"] * raster["height"]
us = ctx.prof_table()["ortho_add"]["avg_us"]
moved = 8 * px + seen * (12 + 12)
say("ortho_add: %d of %d pixels seen (%.1f %%); %.1f MB by the byte count (8 B best a pixel, 12 B of samples and 12 B stored a seen pixel)"
    " in %.1f us: %.0f GB/s" % (seen, px, 100.0 * seen / px, moved / 1e6, us, moved / us / 1e3))
t = time.perf_counter()
host = orthophoto_host([(camera, pixels)], raster)
say("host statement (one core) on the same pixels: %.1f ms; equal rgb: %s, equal cover: %s"
    % (1e3 * (time.perf_counter() - t), np.array_equal(host["rgb"], final["rgb"]), np.array_equal(host["cover"], final["cover"])))
ctx.close()
say("done")

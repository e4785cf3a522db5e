"""What the PNG file of a window's map costs (profiles/png_map.txt is one run's output): one 1400-wide
two-panel map of tests/map_cases.py with four insets, `Context.map_draw` with format="jpeg" against format="png" on one
handle, medians of 20 calls in turn after three warm-up calls each, the file sizes beside Pillow's, the per-kernel times
of the profiling table for both formats, and the coder alone on uniform noise.  Needs an MI355X.

    python tools/png_map_cost.py [output file]"""
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from PIL import Image

import map_cases as mc
import thumb_cases as tc
from iceberg_tracking_code_amd import Context, encode_png_host

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


pic = mc.picture(1400, 2, 0)
insets = tc.inset_cases(1400, pic["height"])["corners"]
ctx = Context(64, 64, n_slots=1, max_pts=1 << 12)
for q in insets:
    ctx.map_inset_set(q["index"], q["pixels"])
full = dict(pic, insets=[{k: v for k, v in q.items() if k != "pixels"} for q in insets])
say("picture %d x %d, %d arrows in panel 0, %d insets" % (pic["width"], pic["height"], len(pic["panels"][0]["arrows"]), len(insets)))
files = {}
for fmt in ("jpeg", "png"):
    for _ in range(3):
        files[fmt], rgb = ctx.map_draw(full, want_rgb=True, format=fmt)
times = {"jpeg": [], "png": []}
for _ in range(20):
    for fmt in ("jpeg", "png"):
        t = time.perf_counter()
        ctx.map_draw(full, format=fmt)
        times[fmt].append(1e3 * (time.perf_counter() - t))
for fmt in ("jpeg", "png"):
    say("map_draw format=%s: median %.3f ms (min %.3f, max %.3f) of 20, file %d bytes" % (fmt, statistics.median(times[fmt]), min(times[fmt]), max(times[fmt]), len(files[fmt])))
assert np.array_equal(np.asarray(Image.open(io.BytesIO(files["png"]))), rgb)
t = time.perf_counter()
host = encode_png_host(rgb)
say("host statement of the same file: %.1f ms, equal bytes: %s" % (1e3 * (time.perf_counter() - t), host == files["png"]))
for level in (0, 1, None):
    buf = io.BytesIO()
    t = time.perf_counter()
    Image.fromarray(rgb).save(buf, "PNG", **({} if level is None else dict(compress_level=level)))
    say("Pillow PNG compress_level=%s: %d bytes, %.1f ms" % (level, len(buf.getvalue()), 1e3 * (time.perf_counter() - t)))
for fmt in ("jpeg", "png"):
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(20):
        ctx.map_draw(full, format=fmt)
    ctx.prof_enable(False)
    say("per kernel, format=%s (20 pictures, HIP events):" % fmt)
    for name, v in ctx.prof_table().items():
        say("  %-22s launches %4d  avg %9.1f us" % (name, v["launches"], v["avg_us"]))
# the coder alone on noise: every byte a token, the parse's chunk hops at their most
noise = np.random.default_rng(0).integers(0, 256, (736, 1400, 3), dtype=np.uint8)
ctx.png_encode(noise)
ctx.prof_reset()
ctx.prof_enable(True)
for _ in range(5):
    ctx.png_encode(noise)
ctx.prof_enable(False)
say("per kernel, png_encode of 1400 x 736 uniform noise (5 pictures):")
for name, v in ctx.prof_table().items():
    say("  %-22s launches %4d  avg %9.1f us" % (name, v["launches"], v["avg_us"]))
ctx.close()
say("done")

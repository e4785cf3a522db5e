"""What a movie frame costs (profiles/movie_frame.txt is one run's output), at the real sizes: a 1200 x 800
segment picture and a 1400-wide two-panel map of tests/map_cases.py, both scaled to 2000 pixels wide.  Per picture: the
picture call and `Context.picture_frame` on one handle, medians of 20 calls in turn after three warm-up calls each; the
frame against the host statement (`movie.frame_host`) and against Pillow's resize and save on one core, bytes compared; the
per-kernel times of the profiling table (HIP events) for 20 frames: resize, forward DCT, entropy coder -- what is left of
the call is the two waits for the device inside the coder, the download of the coded frame and the host's share.  Needs an
MI355X.

    python tools/movie_frame_cost.py [output file]"""
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
from iceberg_tracking_code_amd import Context, frame_host, movie_size, synth

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
QUALITY, N = 90, 20


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def med(v):
    return "median %.3f ms (min %.3f, max %.3f) of %d" % (statistics.median(v), min(v), max(v), len(v))


ctx = Context(2400, 1600, n_slots=1, max_pts=1 << 12)
ctx.upload_gray(0, synth.frame(2400, 1600, 0, 0))
rng = np.random.default_rng(5)
start = rng.uniform((0, 0), (2400, 1600), (3000, 2))
tracks = (start[:, None, :] + np.cumsum(rng.normal(0, 12, (3000, 3, 2)), axis=1)).astype(np.float32)
the_map = mc.picture(1400, 2, 0)
kinds = {"segment picture": lambda **kw: ctx.plot_tracks(0, tracks, 1200, "20190714-123005 120/60", 85, **kw),
         "window map": lambda **kw: ctx.map_draw(the_map, **kw)}
for name, draw in kinds.items():
    for _ in range(3):
        _, rgb = draw(want_rgb=True)
    h, w = rgb.shape[:2]
    size = movie_size(w, h)
    for _ in range(3):
        frame = ctx.picture_frame(size, QUALITY)
    say("%s %d x %d -> frame %d x %d, quality %d, %d bytes" % (name, w, h, size[0], size[1], QUALITY, len(frame)))
    t_pic, t_frame = [], []
    for _ in range(N):
        t = time.perf_counter()
        draw()
        t_pic.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        ctx.picture_frame(size, QUALITY)
        t_frame.append(1e3 * (time.perf_counter() - t))
    say("  the picture call:    " + med(t_pic))
    say("  picture_frame:       " + med(t_frame))
    t = time.perf_counter()
    host = frame_host(rgb, size, QUALITY)
    say("  frame_host (one core): %.1f ms, equal bytes: %s" % (1e3 * (time.perf_counter() - t), host == frame))
    pil = []
    for _ in range(3):
        buf = io.BytesIO()
        t = time.perf_counter()
        Image.fromarray(rgb).resize(size, Image.BICUBIC).save(buf, "JPEG", quality=QUALITY)
        pil.append(1e3 * (time.perf_counter() - t))
    say("  Pillow resize + save (one core): best %.1f ms of 3, equal bytes: %s" % (min(pil), buf.getvalue() == frame))
    draw()
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(N):
        ctx.picture_frame(size, QUALITY)
    ctx.prof_enable(False)
    total = 0.0
    say("  per kernel, %d frames (HIP events):" % N)
    for kernel, v in ctx.prof_table().items():
        say("    %-20s launches %4d  avg %9.1f us" % (kernel, v["launches"], v["avg_us"]))
        total += v["total_ms"] / N
    say("  kernels together %.3f ms a frame; the rest of the call (two waits inside the coder, download, host): %.3f ms"
        % (total, statistics.median(t_frame) - total))
ctx.close()
say("done")

"""What the picture of a segment costs: `SegmentTracker.plot_closed` -- rasterised and coded on the device
-- beside the host route it replaces: `download_level` + `seg_read` + the reference's matplotlib calls (s1:405-434).

    python tools/plot_overlay.py [--width 3456 --height 2304] [--reps 20] [--out profiles/plot_overlay.json]

A synthetic sequence at the reference's detector and tracker parameters gives a closed segment of some ten thousand
tracks of 3 vertices.  Then, on that one segment and frame:
  wall     the whole call, host clock, the call waits for the device: median / min / max over --reps after 3 warm-up calls
  kernels  HIP events around every kernel of the call (icelk_prof_enable), in a run of the same calls of its own: the
           average per launch of the four plot kernels, the forward kernel and the coder's kernels
  host     the route without the feature, where matplotlib is present: frame and tracks copied back, the figure drawn
           with the reference's calls and saved as PNG at 80 dpi into memory; 3 repetitions
One JSON line on stdout; --out writes it to a file as well.  Needs a GPU."""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def host_route(ctx, slot, stamp_lines):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.collections as mc
    import matplotlib.pyplot as plt
    t0 = time.perf_counter()
    frame_gray = ctx.download_level(slot, 0)
    tracks, _ = ctx.seg_read(closed=True)
    t1 = time.perf_counter()
    plt.ioff()
    figsize = (15.0, 15.0 * frame_gray.shape[0] / frame_gray.shape[1])
    fig, ax = plt.subplots(1, 1, figsize=figsize, facecolor="w")
    ax.imshow(frame_gray, cmap="gray")
    ax.add_collection(mc.LineCollection(tracks, color="red", alpha=0.4))
    endpoints = np.float32([tr[-1] for tr in tracks]).reshape(-1, 2)
    ax.plot(endpoints[:, 0], endpoints[:, 1], ".", color="red", ms=2.5, alpha=0.6)
    ax.set_xlim([0, frame_gray.shape[1]])
    ax.set_ylim([frame_gray.shape[0], 0])
    ax.set_xticklabels([])
    ax.set_yticklabels([])
    fig.tight_layout()
    ax.annotate("\n".join(stamp_lines), (0.03, 0.93), xycoords="axes fraction", fontsize=22, color="#2b8cbe")
    buf = io.BytesIO()
    plt.savefig(buf, format="png", dpi=80)
    plt.close(fig)
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), len(buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3456)
    ap.add_argument("--height", type=int, default=2304)
    ap.add_argument("--plot-width", type=int, default=1200)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from iceberg_tracking_code_amd import SegmentTracker
    stamp = "20190724-100200 120/60"
    trk = SegmentTracker(a.width, a.height, 2, max_pts=1 << 18)
    try:
        seg = None
        for k in range(3):
            seg = trk.push_synth(300 * k, -200 * k, seed=77)
        first, tracks, _ = seg
        ctx, slot = trk.ctx, trk.cur
        call = lambda: trk.plot_closed(a.plot_width, stamp, a.quality)
        for _ in range(3):
            data = call()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
        ctx.prof_reset()
        ctx.prof_enable(True)
        for _ in range(a.reps):
            call()
        ctx.prof_enable(False)
        table = {k: round(v["avg_us"], 2) for k, v in ctx.prof_table().items() if k.startswith(("plot_", "jpeg_fwd", "jpeg_enc_"))}
        launches = {k: v["launches"] // a.reps for k, v in ctx.prof_table().items() if k in table}
        res = dict(tool="plot_overlay", frame=[a.width, a.height], tracks=int(len(tracks)), vertices=int(tracks.shape[1]),
                   plot_width=a.plot_width, quality=a.quality, file_bytes=len(data), reps=a.reps,
                   wall_ms=dict(median=round(statistics.median(wall), 3), min=round(min(wall), 3), max=round(max(wall), 3)),
                   kernel_avg_us=table, kernel_launches_per_call=launches,
                   kernels_us_per_call=round(sum(table[k] * launches[k] for k in table), 1),
                   plot_kernels_us_per_call=round(sum(table[k] * launches[k] for k in table if k.startswith("plot_")), 1))
        try:
            host = [host_route(ctx, slot, ["Displacement over 120 seconds, tracking every 60 seconds", stamp.split()[0]]) for _ in range(3)]
            res["host_route_ms"] = dict(copy_back=round(statistics.median(h[0] for h in host), 2),
                                        matplotlib=round(statistics.median(h[1] for h in host), 1), png_bytes=host[-1][2])
        except ImportError:
            res["host_route_ms"] = "not measured: matplotlib is not installed"
    finally:
        trk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

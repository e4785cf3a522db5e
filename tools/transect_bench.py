#!/usr/bin/env python3
"""One day binned into the boxes around a mooring (transect.utm_to_transect's device pass) -> profiles/transect.txt.

    python tools/transect_bench.py [--cams 2] [--hours 24] [--per-hour 21000] [--nr 7] [--width 200] [--repeat 3] [--out PATH]

The day: --cams cameras x --hours hourly files of --per-hour velocities over a ~7 x 5 km fjord, 30-minute windows (24 h:
48 of them), a lattice of (2 floor(nr / 2) + 1)^2 boxes of --width m, turned by -45 degrees, in the middle of the fjord.
Reported, every run listed:
  device pass   the kernels of icelk_boxes_bin_windows (assign, sort, reduce; HIP events), and its assign kernel alone
                (the profiling table's boxes_day_assign);
  the gridder   the same for icelk_grid_bin_windows on the same points, 200 m cells: its assign kernel tests the nine
                cells around a point where the boxes' kernel tests every box;
  the CPU loop  what a user of the reference runs today: for every window and every box
                matplotlib.path.Path(poly).contains_points over the window's points, np.sum(u_sel) / n, np.hypot -- wall
                time on one core, the windows' points selected beforehand and not timed.  Skipped without matplotlib.
"""
import argparse
import datetime as dt
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iceberg_tracking_code_amd import BoxSet, Context, day_grid, transect  # noqa: E402

DAY = dt.datetime(2022, 7, 12)
SPACING = 200


def make_day(root, cams, hours, per_hour):
    rng = np.random.default_rng(7)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 60))
    rad = rng.uniform(2200, 2600, 60)
    fjord = {"x": 500000.0 + np.round(1.4 * rad * np.cos(ang), 1), "y": 6500000.0 + np.round(rad * np.sin(ang), 1)}
    names = ["cam%d" % c for c in range(cams)]
    for name in names:
        ws = os.path.join(root, name, "utm")
        os.makedirs(ws)
        for hr in range(hours):
            e0 = day_grid.epoch_seconds(DAY + dt.timedelta(hours=hr))
            n = per_hour
            t = np.sort(rng.integers(e0, e0 + 3600, n)).astype(np.int64)
            x = rng.uniform(min(fjord["x"]), max(fjord["x"]), n)
            y = rng.uniform(min(fjord["y"]), max(fjord["y"]), n)
            u, v = rng.normal(0.2, 0.4, n), rng.normal(-0.1, 0.3, n)
            np.savez(os.path.join(ws, (DAY + dt.timedelta(hours=hr)).strftime("%Y%m%d_%H00") + "_60s_utm.npz"),
                     x=x, y=y, u=u, v=v, speed=np.hypot(u, v), time=t)
    schedule = [dict(camera=n, start_day=20220701, end_day=20220731, start_time="00:00", tracking_duration=float(hours))
                for n in names]
    return names, schedule, [], fjord


def cpu_loop(boxes, windows):
    import matplotlib.path as mplPath
    t = time.perf_counter()
    total = 0
    for x, y, u, v in windows:
        points = np.vstack((x, y)).T
        for poly in boxes.polygons:
            sel = mplPath.Path(poly).contains_points(points)
            n = int(sel.sum())
            total += n
            if n:
                np.hypot(np.sum(u[sel]) / n, np.sum(v[sel]) / n)
    return time.perf_counter() - t, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=2)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--per-hour", type=int, default=21000)
    ap.add_argument("--nr", type=int, default=7)
    ap.add_argument("--width", type=float, default=200.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transect.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            names, schedule, drifts, fjord = make_day(tmp, a.cams, a.hours, a.per_hour)
            boxes = BoxSet.around_mooring([500000.0, 6500000.0], azimuth=-45, width=a.width, nr=a.nr)
            plan = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
            say("day: %d cameras x %d h x %d velocities/h, %d windows of 30 min, %d mooring boxes of %g m"
                % (a.cams, a.hours, a.per_hour, len(plan.windows), len(boxes), a.width))

            def boxes_pass():
                timing = {}
                transect._transect_day(ctx, plan, boxes, 5, "map", False, timing)
                return timing

            def grid_pass():
                timing = {}
                day_grid._grid_day(ctx, plan, fjord, SPACING, 5, timing)
                return timing

            results = {}
            for label, run, kernel in (("boxes", boxes_pass, "boxes_day_assign"), ("gridder", grid_pass, "grid_day_assign")):
                run()                                                # warm-up: allocations, code objects
                ctx.prof_enable(True)
                try:
                    rows = []
                    for _ in range(a.repeat):
                        ctx.prof_reset()
                        timing = run()
                        ctx.sync()
                        rows.append((timing["kernels_ms"], ctx.prof_table()[kernel]["total_ms"]))
                finally:
                    ctx.prof_enable(False)
                results[label] = rows
                say("%-8s device pass (assign, sort, reduce; HIP events), %d runs: %s ms; %s alone: %s ms; %d points"
                    % (label, a.repeat, ", ".join("%.3f" % r[0] for r in rows), kernel, ", ".join("%.3f" % r[1] for r in rows),
                       timing["points"]))
            b, g = min(r[1] for r in results["boxes"]), min(r[1] for r in results["gridder"])
            say("assign kernels, best of each: boxes %.3f ms, gridder %.3f ms: %.2fx for B / 9 = %.2f times the box tests"
                % (b, g, b / g, len(boxes) / 9.0))
            d = day_grid.load_day(plan)
            group = day_grid.window_of_points(d["t"], d["off"], d["fcam"], d["lo"], d["hi"], d["wf0"], d["wf1"])
            windows = [[d[k][group == w] for k in ("x", "y", "u", "v")] for w in sorted(set(group[group >= 0]))]
            try:
                runs = [cpu_loop(boxes, windows) for _ in range(a.repeat)]
                best = min(r[0] for r in runs)
                say("CPU loop (matplotlib contains_points per window and box, np.sum / n, np.hypot; one core, selection not timed), "
                    "%d runs: %s s; %d points in boxes" % (a.repeat, ", ".join("%.3f" % r[0] for r in runs), runs[0][1]))
                say("CPU loop vs device pass: %.0fx" % (best / (min(r[0] for r in results["boxes"]) * 1e-3)))
            except ImportError:
                say("CPU loop: matplotlib is not installed here")
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of the s3 day driver (day_grid.utm_to_gridded_utm) on one synthetic day -> profiles/r07_grid_day.txt.

    python tools/grid_day_bench.py [--cams 4] [--hours 12] [--per-hour 250000] [--repeat 3] [--out PATH] [--stats]

The day: --cams cameras x --hours hourly files of --per-hour velocities (int64 epoch times, 10 % of each file in the
neighbouring hours, a quarter of the points on cell edges), clock drifts of tens of seconds, 30-minute windows, 200 m
cells over a ~7 x 5 km fjord.  Reported, each the best of --repeat runs:
  device pass   the kernels of icelk_grid_bin_windows (assign, sort, reduce; HIP events), points/s of loaded points;
  driver        utm_to_gridded_utm(save=False) wall time: np.load of every hour file, planning, upload, kernels,
                read-back, packing -- split into its stages;
  per window    bin_velocities once per window on that window's points (selected with numpy beforehand, not timed),
                the way a loop around the one-window entry point runs.
With --stats (-> profiles/grid_stats.txt) instead: the device pass without and with the per-cell statistics (std, median,
MAD: icelk_grid_bin_windows_stats), every run listed; the statistics' kernels one by one (HIP events of the profiling
table); and the numpy route on the same points -- per (window, cell) np.std(ddof=1), np.median and the MAD expression for
u and v on one core, the points of every cell selected beforehand and not timed.
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

from iceberg_tracking_code_amd import Context, bin_velocities, day_grid, utm_to_gridded_utm  # noqa: E402
from iceberg_tracking_code_amd.gridding import create_grid_across_fjord  # noqa: E402

DAY = dt.datetime(2022, 7, 12)
SPACING = 200
STATS_KERNELS = ("grid_segments", "grid_std", "grid_select")


def make_day(root, cams, hours, per_hour):
    rng = np.random.default_rng(7)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 60))
    rad = rng.uniform(2200, 2600, 60)
    fjord = {"x": 500000.0 + np.round(1.4 * rad * np.cos(ang), 1), "y": 6500000.0 + np.round(rad * np.sin(ang), 1)}
    left, top = min(fjord["x"]), max(fjord["y"])
    names = ["cam%d" % c for c in range(cams)]
    for name in names:
        ws = os.path.join(root, name, "utm")
        os.makedirs(ws)
        for hr in range(6, 6 + hours):
            e0 = day_grid.epoch_seconds(DAY + dt.timedelta(hours=hr))
            n = per_hour
            t = np.sort(rng.integers(e0 - 180, e0 + 3780, n)).astype(np.int64)
            x = rng.uniform(left, max(fjord["x"]), n)
            y = rng.uniform(min(fjord["y"]), top, n)
            k = n // 8
            x[:k] = left + SPACING * rng.integers(0, 36, k)
            y[k:2 * k] = top - SPACING * rng.integers(0, 26, k)
            u, v = rng.normal(0.2, 0.4, n), rng.normal(-0.1, 0.3, n)
            np.savez(os.path.join(ws, (DAY + dt.timedelta(hours=hr)).strftime("%Y%m%d_%H00") + "_60s_utm.npz"),
                     x=x, y=y, u=u, v=v, speed=np.hypot(u, v), time=t)
    schedule = [dict(camera=n, start_day=20220701, end_day=20220731, start_time="06:00", tracking_duration=float(hours))
                for n in names]
    drifts = [dict(cam=n, start_date=20220701, end_date=20220731, drift_start_sec=10.0 * c + 0.3, drift_pday_sec=1.5)
              for c, n in enumerate(names)]
    return names, schedule, drifts, fjord


def cells_of_the_day(plan, fjord):
    """The day's points as _grid_day loads them, split by (window, cell): [(u, v)] in concatenation order.  The cell is
    the floor index, so a point on an edge lies in one cell here where the gridder may put it in two or none: good for a
    timing, not for a comparison."""
    parts = [day_grid._load_hour_file(f["path"]) for f in plan.files]
    x, y, u, v, t = (np.concatenate([p[k] for p in parts]) for k in range(5))
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in parts])
    fcam = np.array([f["cam"] for f in plan.files], np.int32)
    lo, hi = (np.array([c[k] for c in plan.cameras], np.int64) for k in ("lo", "hi"))
    wf0, wf1 = (np.array([c[k] for c in plan.cameras], np.int32) for k in ("f0", "f1"))
    w = day_grid.window_of_points(t, off, fcam, lo, hi, wf0, wf1).astype(np.int64)
    left, top = min(fjord["x"]), max(fjord["y"])
    i, j = np.floor((x - left) / SPACING).astype(np.int64), np.floor((top - y) / SPACING).astype(np.int64)
    rows = int(j.max()) + 1
    seg = (w * (int(i.max()) + 1) + i) * rows + j
    keep = np.flatnonzero(w >= 0)
    order = keep[np.argsort(seg[keep], kind="stable")]
    cuts = np.flatnonzero(np.diff(seg[order])) + 1
    return list(zip(np.split(u[order], cuts), np.split(v[order], cuts)))


def numpy_route(cells):
    t = time.perf_counter()
    for pair in cells:
        for a in pair:
            if len(a) > 1:
                np.std(a, ddof=1)
            m = np.median(a)
            np.median(np.abs(a - m))
    return time.perf_counter() - t


def stats_report(ctx, a, say, names, tmp, schedule, drifts, fjord):
    def one_pass(stats):
        timing = {}
        p = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
        day_grid._grid_day(ctx, p, fjord, SPACING, 5, timing, stats=stats)
        return timing

    one_pass(False)                                          # warm-up: allocations, code objects
    one_pass(True)
    off = [one_pass(False)["kernels_ms"] for _ in range(a.repeat)]
    say("device pass without statistics (assign, sort, reduce; HIP events), %d runs: %s ms"
        % (a.repeat, ", ".join("%.2f" % x for x in off)))
    on = []
    ctx.prof_enable(True)
    try:
        for _ in range(a.repeat):
            ctx.prof_reset()
            timing = one_pass(True)
            ctx.sync()
            table = ctx.prof_table()
            on.append((timing["kernels_ms"], [table[k]["total_ms"] for k in STATS_KERNELS]))
    finally:
        ctx.prof_enable(False)
    npts = timing["points"]
    say("device pass with statistics (+ segments, std, select), %d runs: %s ms" % (a.repeat, ", ".join("%.2f" % x for x, _ in on)))
    for k, name in enumerate(STATS_KERNELS):
        say("  %-14s %s ms" % (name, ", ".join("%.3f" % per[k] for _, per in on)))
    best_on, best_off = min(x for x, _ in on), min(off)
    say("statistics add %.2f ms to %.2f ms (best of each): %.3g points/s with them" % (best_on - best_off, best_off, npts / (best_on * 1e-3)))
    plan = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
    cells = cells_of_the_day(plan, fjord)
    sizes = np.array([len(u) for u, _ in cells])
    say("segments with points: %d; points per segment: median %d, 99th percentile %d, largest %d"
        % (len(cells), np.median(sizes), np.percentile(sizes, 99), sizes.max()))
    host = min(numpy_route(cells) for _ in range(a.repeat))
    say("numpy route on one core (np.std, np.median, MAD per segment for u and v; selection not timed): %.3f s" % host)
    say("numpy route vs the statistics' kernels: %.1fx" % (host / ((best_on - best_off) * 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--hours", type=int, default=12)
    ap.add_argument("--per-hour", type=int, default=250000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", action="store_true")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "grid_stats.txt" if a.stats else "r07_grid_day.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write_out():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            t = time.perf_counter()
            names, schedule, drifts, fjord = make_day(tmp, a.cams, a.hours, a.per_hour)
            say("day: %d cameras x %d h x %d velocities/h, 30-min windows, %d m cells (written in %.1f s)"
                % (a.cams, a.hours, a.per_hour, SPACING, time.perf_counter() - t))
            plan = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
            grid = create_grid_across_fjord(ctx, fjord, SPACING)
            say("windows %d, hour files loaded %d, kept cells %d of %d" % (len(plan.windows), len(plan.files),
                                                                          len(grid[0]), grid[4] * grid[5]))
            if a.stats:
                stats_report(ctx, a, say, names, tmp, schedule, drifts, fjord)
                return write_out()
            # the driver, stage by stage, and the device pass alone
            stages, walls, first = [], [], None
            for _ in range(a.repeat):
                timing = {}
                t = time.perf_counter()
                p = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
                out = day_grid._grid_day(ctx, p, fjord, SPACING, 5, timing)
                walls.append(time.perf_counter() - t)
                stages.append(timing)
                first = first or out
            t = time.perf_counter()
            full = utm_to_gridded_utm(names, tmp, "utm", tmp, schedule, drifts, fjord, DAY, 0.5, SPACING, 5, ctx=ctx,
                                      save=False)
            wall_public = time.perf_counter() - t
            assert [n for n, _ in full] == [n for n, _ in first]
            best = min(range(a.repeat), key=lambda k: walls[k])
            s = stages[best]
            npts = s["points"]
            kern = min(x["kernels_ms"] for x in stages)
            say("points loaded (all windows' files): %d" % npts)
            say("device pass (kernels, HIP events): %.2f ms = %.3g points/s" % (kern, npts / (kern * 1e-3)))
            say("driver wall (plan + load + device call + pack): %.3f s = %.3g points/s; stages of that run: "
                "load %.3f s, device call (upload + kernels + read-back) %.3f s, pack %.3f s"
                % (walls[best], npts / walls[best], s["load_s"], s["device_call_s"], s["pack_s"]))
            say("utm_to_gridded_utm (own call, save=False): %.3f s" % wall_public)
            # the per-window loop over the one-window entry point, on the same points
            sel = []
            for w, (start, end) in enumerate(plan.windows):
                parts = []
                for c in plan.cameras:
                    for f in range(c["f0"][w], c["f1"][w] + 1):
                        with np.load(plan.files[f]["path"]) as z:
                            tt = z["time"].astype(np.float64)
                            m = (tt >= c["lo"][w]) & (tt < c["hi"][w])
                            parts.append([z[k][m] for k in ("x", "y", "u", "v")])
                if parts:
                    sel.append([np.concatenate([q[k] for q in parts]) for k in range(4)])
            nsel = sum(len(q[0]) for q in sel)
            loop = []
            for _ in range(a.repeat):
                t = time.perf_counter()
                for x, y, u, v in sel:
                    bin_velocities(ctx, x, y, u, v, fjord, SPACING, 5, grid=grid)
                loop.append(time.perf_counter() - t)
            say("per-window bin_velocities loop (%d calls, %d selected points, selection not timed): %.3f s = "
                "%.3g points/s" % (len(sel), nsel, min(loop), nsel / min(loop)))
            say("device pass vs per-window loop: %.1fx" % (min(loop) / (kern * 1e-3)))
    finally:
        ctx.close()
    write_out()


if __name__ == "__main__":
    main()

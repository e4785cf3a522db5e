#!/usr/bin/env python3
"""Rate of the s4 averages (postprocess.average_periods, icelk_cube_average) on a season-sized cube
-> profiles/s4_average.txt.

    python tools/s4_bench.py [--rows 45] [--cols 70] [--windows 6000] [--days 125] [--repeat 7] [--out PATH]

The cube: --rows x --cols cells (a 200 m grid over a ~14 x 9 km fjord, the cells inside an elliptic outline kept),
--windows 30-minute windows spread over --days days, 35 % of the kept entries NaN -- estimates of a season, no real one
is at hand.  The request: the reference's __main__ loop, one period of 12:00 + 22 h per day, at coarseness 1 and 4.
Reported per coarseness:
  device pass   the kernels of icelk_cube_average (HIP events around them, uploads and read-backs excluded), warmed,
                best and spread of --repeat runs; algorithmic bytes (3 fields x 8 B x selected windows x cells read,
                the outputs written) over that time, as a share of the 8 TB/s HBM peak;
  whole call    average_periods wall time (selection on the host, tables up, kernels, results back, host clock around a
                call that ends in a device synchronise);
  upload        VelocityCube(...) wall time: the transposition to [window][cell] in numpy and the copy to the device;
  numpy         the reference's way on the same cube in this process, one core: per period np.nanmean, np.nanmean,
                np.nansum over cube[:, :, mask], then spatial_mean.
"""
import argparse
import datetime as dt
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iceberg_tracking_code_amd import Context, VelocityCube, average_periods, postprocess  # noqa: E402

T0 = dt.datetime(2022, 5, 1)
HBM_PEAK = 8.0e12


def make_cube(rows, cols, windows, days):
    rng = np.random.default_rng(5)
    steps = np.sort(rng.choice(days * 48, windows, replace=False))
    tt = np.array([postprocess.epoch_seconds(T0 + dt.timedelta(minutes=30 * int(s))) for s in steps], np.float64)
    shape = (rows, cols, windows)
    yy, xx = np.meshgrid(6500000.0 - 200.0 * np.arange(rows), 500000.0 + 200.0 * np.arange(cols), indexing="ij")
    inside = ((xx - xx.mean()) / (0.5 * 200.0 * cols)) ** 2 + ((yy - yy.mean()) / (0.5 * 200.0 * rows)) ** 2 < 1.0
    hole = (rng.random(shape) < 0.35) | ~inside[:, :, None]
    u, v = rng.normal(0.1, 0.3, shape), rng.normal(-0.05, 0.2, shape)
    count = rng.integers(4, 60000, shape).astype(np.float64)
    for a in (u, v, count):
        a[hole] = np.nan
    return dict(x=xx, y=yy, u=u, v=v, count=count, time=tt), int(inside.sum())


def numpy_way(data, periods, coarseness):
    out = []
    tt = data["time"]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for start, end in periods:
            mask = (tt >= postprocess.epoch_seconds(start)) & (tt < postprocess.epoch_seconds(end))
            if not mask.any():
                out.append(None)
                continue
            f = [np.nanmean(data["u"][:, :, mask], 2), np.nanmean(data["v"][:, :, mask], 2),
                 np.nansum(data["count"][:, :, mask], 2)]
            if coarseness > 1:
                f = [postprocess.spatial_mean_host(a, coarseness) for a in f]
            out.append(f)
    return out


def same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45)
    ap.add_argument("--cols", type=int, default=70)
    ap.add_argument("--windows", type=int, default=6000)
    ap.add_argument("--days", type=int, default=125)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s4_average.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    data, kept = make_cube(a.rows, a.cols, a.windows, a.days)
    ncells = a.rows * a.cols
    periods = [(T0 + dt.timedelta(days=d, hours=12), T0 + dt.timedelta(days=d, hours=34)) for d in range(a.days)]
    say("tools/s4_bench.py --rows %d --cols %d --windows %d --days %d --repeat %d; numpy %s"
        % (a.rows, a.cols, a.windows, a.days, a.repeat, np.__version__))
    say("cube: %d x %d cells (%d inside the outline), %d windows of 30 min over %d days, 35 %% NaN; %.1f MB per field"
        % (a.rows, a.cols, kept, a.windows, a.days, ncells * a.windows * 8 / 1e6))
    say("request: %d periods (12:00 + 22 h of every day), all in one icelk_cube_average call" % len(periods))
    ctx = Context(64, 64, n_slots=1, max_pts=1024)
    try:
        ups = []
        for _ in range(3):
            t = time.perf_counter()
            cube = VelocityCube(data, ctx)
            ups.append(time.perf_counter() - t)
            cube.close()
        cube = VelocityCube(data, ctx)
        say("upload (VelocityCube: numpy transposition to [window][cell] + copy of 3 fields, host clock): best %.1f ms "
            "of 3 (%.1f .. %.1f)" % (min(ups) * 1e3, min(ups) * 1e3, max(ups) * 1e3))
        for coarseness in (1, 4):
            average_periods(cube, periods, coarseness)                       # warm-up: code objects, allocations
            kern, wall, got, sel = [], [], None, 0
            for _ in range(a.repeat):
                timing = {}
                t = time.perf_counter()
                got = average_periods(cube, periods, coarseness, timing=timing)
                wall.append(time.perf_counter() - t)
                kern.append(timing["kernels_ms"])
                sel = timing["selected"]
            cr, cc = -(-a.rows // coarseness), -(-a.cols // coarseness)
            bytes_read = 3 * 8 * sel * ncells
            bytes_written = 4 * 8 * len(periods) * ncells + (4 * 8 * len(periods) * cr * cc if coarseness > 1 else 0)
            best = min(kern)
            say("coarseness %d: %d selected windows in all" % (coarseness, sel))
            say("  device pass (kernels, HIP events): best %.3f ms of %d (%.3f .. %.3f); algorithmic bytes %.1f MB read "
                "+ %.2f MB written = %.1f GB/s = %.2f %% of the 8 TB/s peak"
                % (best, a.repeat, min(kern), max(kern), bytes_read / 1e6, bytes_written / 1e6,
                   (bytes_read + bytes_written) / (best * 1e-3) / 1e9,
                   100.0 * (bytes_read + bytes_written) / (best * 1e-3) / HBM_PEAK))
            say("  whole call (average_periods, host clock): best %.3f ms of %d (%.3f .. %.3f)"
                % (min(wall) * 1e3, a.repeat, min(wall) * 1e3, max(wall) * 1e3))
            t = time.perf_counter()
            ref = numpy_way(data, periods, coarseness)
            t_np = time.perf_counter() - t
            ok = all((r is None and g["time_str"] is None) or
                     (r is not None and same(g["u"], r[0]) and same(g["v"], r[1]) and same(g["count"], r[2]))
                     for g, r in zip(got, ref))
            if not ok:
                raise SystemExit("device results differ from numpy's")
            say("  numpy, the reference's way (per period nanmean, nanmean, nansum%s; one core, one run): %.1f ms; "
                "results equal bit for bit; whole call vs numpy: %.1fx, kernels vs numpy: %.0fx"
                % (", spatial_mean x 3" if coarseness > 1 else "", t_np * 1e3, t_np / min(wall), t_np / (best * 1e-3)))
        cube.close()
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

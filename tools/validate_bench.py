#!/usr/bin/env python3
"""What the normalised median test costs the s3 day driver -> profiles/validate_day.txt.

    python tools/validate_bench.py [--cams 4] [--hours 12] [--per-hour 250000] [--repeat 3] [--out PATH]

The day is tools/grid_day_bench.py's (4 cameras x 12 h x 2.5e5 velocities per hour, 30-minute windows, 200 m cells); the
validation runs with its defaults on a lattice of 400 m.  Reported, in one process and after a warm-up of both passes:
  plain pass       the kernels of icelk_grid_bin_windows (assign, sort, reduce; HIP events), every run and the best;
  validated pass   the kernels of icelk_grid_bin_windows_validated (assign, sort, pools, judge, then the gridder's), likewise;
  the validation's kernels one by one (the profiling table: HIP events around each launch, a run of its own);
  the pools: how many (window, cell) had points, the largest, and how many took each fetch path (order keys staged in LDS up
  to 2048 terms, recomputed from global memory above).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grid_day_bench import DAY, SPACING, make_day  # noqa: E402
from iceberg_tracking_code_amd import Context, day_grid, validate_velocities, validation_lattice  # noqa: E402
from iceberg_tracking_code_amd.validate import validate_options  # noqa: E402

KERNELS = ("validate_assign", "validate_pools", "validate_judge")
POOL_LDS_TERMS = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--hours", type=int, default=12)
    ap.add_argument("--per-hour", type=int, default=250000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_day.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    options = validate_options(True, SPACING)
    ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            t = time.perf_counter()
            names, schedule, drifts, fjord = make_day(tmp, a.cams, a.hours, a.per_hour)
            say("day: %d cameras x %d h x %d velocities/h, 30-min windows, %d m cells, validation lattice %d m (written in %.1f s)"
                % (a.cams, a.hours, a.per_hour, SPACING, options["side"], time.perf_counter() - t))

            def one_pass(validate):
                timing = {}
                p = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
                day_grid._grid_day(ctx, p, fjord, SPACING, 5, timing, validate=validate)
                return timing

            one_pass(None)                                   # warm-up: allocations, code objects
            one_pass(options)
            plain = [one_pass(None)["kernels_ms"] for _ in range(a.repeat)]
            timings = [one_pass(options) for _ in range(a.repeat)]
            valid = [x["kernels_ms"] for x in timings]
            npts = timings[0]["points"]
            say("points loaded (all windows' files): %d; rejected: %d" % (npts, int(timings[0]["rejected"].sum())))
            say("plain pass (assign, sort, reduce; HIP events), %d runs: %s ms; best %.2f ms" % (a.repeat, ", ".join("%.2f" % x for x in plain), min(plain)))
            say("validated pass (validation + the same gridder chain), %d runs: %s ms; best %.2f ms" % (a.repeat, ", ".join("%.2f" % x for x in valid),
                                                                                                      min(valid)))
            say("validated / plain (best of each): %.2fx; the validation adds %.2f ms = %.3g points/s through it"
                % (min(valid) / min(plain), min(valid) - min(plain), npts / ((min(valid) - min(plain)) * 1e-3)))
            ctx.prof_reset()
            ctx.prof_enable(True)
            try:
                one_pass(options)
                ctx.sync()
            finally:
                ctx.prof_enable(False)
            table = ctx.prof_table()
            for k in KERNELS:
                say("  %-16s %.3f ms (%d launch)" % (k, table[k]["total_ms"], table[k]["launches"]))
            # the pools themselves: the same statement through the stand-alone entry point, the windows as groups
            plan = day_grid.plan_day(names, tmp, "utm", schedule, drifts, DAY, 0.5, SPACING)
            L = day_grid.load_day(plan)
            group = day_grid.window_of_points(L["t"], L["off"], L["fcam"], L["lo"], L["hi"], L["wf0"], L["wf1"])
            r = validate_velocities(ctx, L["x"], L["y"], L["u"], L["v"], validation_lattice(fjord, options["side"]),
                                    groups=(group, L["lo"].shape[1]))
            pools = r["pool_n"][r["pool_n"] > 0]
            say("pools with points of their own: %d of %d (window, cell); terms: median %d, largest %d" % (len(pools), r["pool_n"].size,
                                                                                                        np.median(pools), pools.max()))
            say("fetch path: %d pools staged in LDS (<= %d terms), %d walked global memory" % ((pools <= POOL_LDS_TERMS).sum(), POOL_LDS_TERMS,
                                                                                              (pools > POOL_LDS_TERMS).sum()))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

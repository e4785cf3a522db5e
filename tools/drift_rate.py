#!/usr/bin/env python3
"""Rate of the virtual drifters (drift.drift: icelk_cube_drift, icelk_drift_tide) on a season-sized cube -> profiles/drift_rate.txt.

    python tools/drift_rate.py [--rows 45] [--cols 70] [--windows 6000] [--drifters 100000] [--steps 1440] [--step 60] [--order 4]
                               [--repeat 5] [--host-drifters 1000] [--out PATH]

The season is synthetic: --rows x --cols cells 200 m apart, --windows 30-minute windows without a gap, a slow gyre around the
middle of the lattice (so that drifters stay inside for a day) under an M2 + K1 tide and noise, 5 % of the nodes NaN; the fit
is a mean + M2, S2, N2, K1, O1 (m = 11).  --drifters seeds, uniform over the middle of the lattice, are released at random steps
of the first day; --steps steps of --step seconds, min_nodes 2.  Reported, per source:
  kernels    the drift kernel and the visits kernel (HIP events around the two; the tables' upload and the read-back excluded),
             after a warm-up run: best and spread of --repeat runs, and drifter-steps per second -- steps actually taken, the
             sum over the drifters of stop_step - release, over the best time;
  whole call drift() wall time (schedule on the host, kernels, results back);
  host       drift_host on one core with --host-drifters of the same seeds, one run, for scale only; its results equal the
             device's bit for bit (checked here).
ICELK_LIBRARY selects another build of the library (tools/build_variant.sh); the line "library" says which one ran.  There is no
threshold: the numbers are recorded, not gated."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iceberg_tracking_code_amd import Context, DriftResult, VelocityCube, _lib, drift, drift_host, fit_tides  # noqa: E402

T0 = 1627776000.0
CONSTITUENTS = ("M2", "S2", "N2", "K1", "O1")


def make_season(rows, cols, windows, rng):
    time_ = T0 + 1800.0 * np.arange(windows)
    yy, xx = np.meshgrid(6500000.0 - 200.0 * np.arange(rows), 500000.0 + 200.0 * np.arange(cols), indexing="ij")
    w = 2 * np.pi / (3 * 86400.0)                                         # one turn of the gyre in three days
    hours = (time_ - T0) / 3600.0
    tide = 0.05 * np.cos(np.deg2rad(28.9841042) * hours) + 0.02 * np.sin(np.deg2rad(15.0410686) * hours)
    u = (-w * (yy - yy.mean()))[:, :, None] + tide[None, None, :] + 0.01 * rng.normal(size=(rows, cols, windows))
    v = (w * (xx - xx.mean()))[:, :, None] + 0.5 * tide[None, None, :] + 0.01 * rng.normal(size=(rows, cols, windows))
    count = rng.integers(4, 600, (rows, cols, windows)).astype(np.float64)
    hole = rng.random((rows, cols, windows)) < 0.05
    for a in (u, v, count):
        a[hole] = np.nan
    return dict(x=xx, y=yy, u=u, v=v, count=count, time=time_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45)
    ap.add_argument("--cols", type=int, default=70)
    ap.add_argument("--windows", type=int, default=6000)
    ap.add_argument("--drifters", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=1440)
    ap.add_argument("--step", type=float, default=60.0)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-drifters", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_rate.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(7)
    data = make_season(a.rows, a.cols, a.windows, rng)
    n = a.drifters
    sx = data["x"][0, 0] + 200.0 * (a.cols - 1) * rng.uniform(0.3, 0.7, n)
    sy = data["y"][0, 0] - 200.0 * (a.rows - 1) * rng.uniform(0.3, 0.7, n)
    release = rng.integers(0, a.steps, n).astype(np.int32)
    kw = dict(start=T0 + 3600.0, nsteps=a.steps, step=a.step, order=a.order, min_nodes=2, every=60, visits=True)
    say("tools/drift_rate.py --rows %d --cols %d --windows %d --drifters %d --steps %d --step %g --order %d --repeat %d; numpy %s"
        % (a.rows, a.cols, a.windows, n, a.steps, a.step, a.order, a.repeat, np.__version__))
    say("library: %s" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("host load average at the start (1, 5, 15 min): %.1f %.1f %.1f on %d CPUs" % (os.getloadavg() + (os.cpu_count(),)))
    say("season: %d x %d nodes, %d windows of 30 min, 5 %% NaN; two windows are %.0f KB of u, v, count"
        % (a.rows, a.cols, a.windows, 2 * 3 * 8 * a.rows * a.cols / 1e3))
    ctx = Context(64, 64, n_slots=1, max_pts=1024)
    results = {}
    try:
        with VelocityCube(data, ctx) as cube:
            fit = fit_tides(cube, CONSTITUENTS)
            say("fit: mean + %s, m = %d; %d of %d cells fitted; the coefficients are %.0f KB"
                % (", ".join(CONSTITUENTS), fit.coef_u.shape[2], int((fit.status == 0).sum()), a.rows * a.cols, 2 * 8 * fit.coef_u.size / 1e3))
            for name, source in (("cube", cube), ("tide", (fit, cube))):
                drift(source, sx, sy, release=release, **kw)                       # warm-up: code objects, allocations
                kern, wall = [], []
                for _ in range(a.repeat):
                    timing = {}
                    t = time.perf_counter()
                    results[name] = drift(source, sx, sy, release=release, timing=timing, **kw)
                    wall.append(time.perf_counter() - t)
                    kern.append(timing["kernels_ms"])
                r = results[name]
                taken = int((r.stop_step - release)[r.status != 4].sum())
                say("%s source: %d drifters, %d alive at the end, %d drifter-steps taken of %d at most"
                    % (name, n, int((r.status == 0).sum()), taken, int((a.steps - release).sum())))
                say("  kernels (drift, visits; HIP events): best %.3f ms of %d (%.3f .. %.3f) = %.3g drifter-steps/s"
                    % (min(kern), a.repeat, min(kern), max(kern), taken / (min(kern) * 1e-3)))
                say("  whole call (drift, host clock): best %.2f ms of %d (%.2f .. %.2f)" % (min(wall) * 1e3, a.repeat, min(wall) * 1e3, max(wall) * 1e3))
    finally:
        ctx.close()
    m = min(a.host_drifters, n)
    for name, source in (("cube", data), ("tide", (fit, data))):
        t = time.perf_counter()
        host = drift_host(source, sx[:m], sy[:m], release=release[:m], **kw)
        t_host = time.perf_counter() - t
        dev = results[name]
        for k in DriftResult.FIELDS:
            got = getattr(dev, k)
            if not np.array_equal(getattr(host, k), got if k == "time" else got[..., :m], equal_nan=True):
                raise SystemExit("the device's %s differs from the host statement's (%s source)" % (k, name))
        taken = int((host.stop_step - release[:m])[host.status != 4].sum())
        say("host statement, %s source (drift_host, one core, one run, %d drifters): %.1f ms = %.3g drifter-steps/s; its drifters equal "
            "the device's bit for bit" % (name, m, t_host * 1e3, taken / t_host))
    say("host load average at the end: %.1f %.1f %.1f" % os.getloadavg())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of the per-cell harmonic fit (tides.fit_tides, icelk_cube_tide_fit) on a season-sized cube -> profiles/tides.txt.

    python tools/tides_bench.py [--rows 45] [--cols 70] [--windows 6000] [--days 125] [--repeat 7] [--lstsq-cells 200] [--out PATH]

The cube is tools/s4_bench.py's: --rows x --cols cells, --windows 30-minute windows over --days days, 35 % NaN.  The fit: a
mean and M2, S2, N2, K1, O1 (m = 11), with and without the residual cube.  Reported:
  kernels       normal, solve, residual, finish (HIP events around the four, uploads and read-backs excluded), warmed, best and
                spread of --repeat runs; the cube's bytes the rule needs (3 fields read once per pass, two passes, the residual
                cubes written) over that time -- the normal kernel re-reads the cube once per matrix row, which this does not
                count;
  whole call    fit_tides wall time (basis on the host, kernels, results back; a host clock around a call that ends in a device
                synchronise);
  host          fit_tides_host, csrc/tides.h on one core; results equal the device's bit for bit (checked here);
  lstsq         np.linalg.lstsq cell by cell on each cell's samples, timed on --lstsq-cells cells and scaled to the cube; its
                coefficients are compared with the fit's.
There is no threshold: the numbers are recorded, not gated."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from iceberg_tracking_code_amd import Context, VelocityCube, fit_tides, fit_tides_host, tide_basis  # noqa: E402
from s4_bench import make_cube  # noqa: E402

CONSTITUENTS = ("M2", "S2", "N2", "K1", "O1")
FIELDS = ("coef_u", "coef_v", "rms_u", "rms_v", "explained_u", "explained_v", "n", "first", "last", "status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45)
    ap.add_argument("--cols", type=int, default=70)
    ap.add_argument("--windows", type=int, default=6000)
    ap.add_argument("--days", type=int, default=125)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--lstsq-cells", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tides.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    data, kept = make_cube(a.rows, a.cols, a.windows, a.days)
    ncells = a.rows * a.cols
    m = 1 + 2 * len(CONSTITUENTS)
    say("tools/tides_bench.py --rows %d --cols %d --windows %d --days %d --repeat %d; numpy %s"
        % (a.rows, a.cols, a.windows, a.days, a.repeat, np.__version__))
    say("cube: %d x %d cells (%d inside the outline), %d windows of 30 min over %d days, 35 %% NaN; %.1f MB per field"
        % (a.rows, a.cols, kept, a.windows, a.days, ncells * a.windows * 8 / 1e6))
    say("fit: mean + %s, m = %d terms, %d chunks of 256 windows" % (", ".join(CONSTITUENTS), m, -(-a.windows // 256)))
    ctx = Context(64, 64, n_slots=1, max_pts=1024)
    fits = {}
    try:
        with VelocityCube(data, ctx) as cube:
            for residual in (False, True):
                fit_tides(cube, CONSTITUENTS, residual=residual)                   # warm-up: code objects, allocations
                kern, wall = [], []
                for _ in range(a.repeat):
                    timing = {}
                    t = time.perf_counter()
                    fits[residual] = fit_tides(cube, CONSTITUENTS, residual=residual, timing=timing)
                    wall.append(time.perf_counter() - t)
                    kern.append(timing["kernels_ms"])
                cube_bytes = 2 * 3 * 8 * ncells * a.windows + (2 * 8 * ncells * a.windows if residual else 0)
                say("%s the residual cube:" % ("with" if residual else "without"))
                say("  kernels (normal, solve, residual, finish; HIP events): best %.3f ms of %d (%.3f .. %.3f); the cube's bytes %.1f MB "
                    "= %.1f GB/s" % (min(kern), a.repeat, min(kern), max(kern), cube_bytes / 1e6, cube_bytes / (min(kern) * 1e-3) / 1e9))
                say("  whole call (fit_tides, host clock): best %.2f ms of %d (%.2f .. %.2f)"
                    % (min(wall) * 1e3, a.repeat, min(wall) * 1e3, max(wall) * 1e3))
    finally:
        ctx.close()
    fit = fits[True]
    say("fitted cells: %d of %d; median rms_u %.4f m/s" % (int((fit.status == 0).sum()), ncells, float(np.nanmedian(fit.rms_u))))
    t = time.perf_counter()
    host = fit_tides_host(data, CONSTITUENTS, residual=True)
    t_host = time.perf_counter() - t
    for k in FIELDS + ("residual_u", "residual_v"):
        if not np.array_equal(getattr(host, k), getattr(fit, k), equal_nan=True):
            raise SystemExit("the device's %s differs from the host statement's" % k)
    say("host statement (fit_tides_host with the residual cube, one core, one run): %.1f ms; every output equals the device's bit for bit"
        % (t_host * 1e3))
    B = tide_basis(data["time"], CONSTITUENTS, fit.t0)
    cells = np.flatnonzero(fit.status.ravel() == 0)[:a.lstsq_cells]
    u, v = data["u"].reshape(ncells, -1), data["v"].reshape(ncells, -1)
    worst = 0.0
    t = time.perf_counter()
    for c in cells:
        take = np.isfinite(u[c]) & np.isfinite(v[c])
        cu = np.linalg.lstsq(B[take], u[c, take], rcond=None)[0]
        cv = np.linalg.lstsq(B[take], v[c, take], rcond=None)[0]
        worst = max(worst, np.abs(cu - fit.coef_u.reshape(ncells, m)[c]).max(), np.abs(cv - fit.coef_v.reshape(ncells, m)[c]).max())
    t_np = time.perf_counter() - t
    if len(cells):
        say("np.linalg.lstsq cell by cell (u and v, one core): %.1f ms for %d cells = %.0f ms scaled to the %d fitted cells; largest "
            "|coefficient - fit| %.2e" % (t_np * 1e3, len(cells), t_np * 1e3 * int((fit.status == 0).sum()) / len(cells),
                                           int((fit.status == 0).sum()), worst))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of the calibration misfit on the device (calibration.ShorelineScene, icelk_calib_cost / icelk_calib_residuals)
-> profiles/calibration_cost.txt.

    python tools/calib_bench.py [--points 180] [--vertices 5000] [--lattice 32] [--repeat 7] [--out PATH]

The scene: --points shoreline points with 1 px digitising noise on a 3456 x 2304 photo, --vertices irregularly spaced
waterline vertices (the projection of the same curve under known parameters) -- a synthetic scene, no real one is at
hand.  Reported, each warmed, best and spread of --repeat runs:
  lattice       the rmse on a --lattice^4 lattice over the union box (icelk_calib_cost): HIP-event time of the kernels
                summed over the launches, and point pairs (candidates x points x vertices) per second;
  residuals     one icelk_calib_residuals launch of 5 x 240 candidates, what an iteration of the fit issues for the 240
                rows of a workbook: HIP-event time and point pairs per second;
  calibrate     the whole calibrate(...) call for 240 overlapping boxes with a 16^4 lattice, 8 lattice seeds and two
                refinement rounds, by the host clock;
  numpy         the misfit restated in numpy (unfused dx * dx + dy * dy, min, sqrt) in this process, one core, on a
                subset of the candidates: results compared bit for bit, point pairs per second;
  inner loop    the instruction mix of the kernels' vertex loop, from hipcc -S of csrc/k_calib.hip with the build's flags.
No peak f64 vector rate of the card has been measured here, so no roofline fraction is given.
"""
import argparse
import collections
import itertools
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iceberg_tracking_code_amd import Context, ShorelineScene, calibrate  # noqa: E402
from iceberg_tracking_code_amd import build as icelk_build  # noqa: E402

CAM = dict(image_width=3456, image_height=2304, sensor_width=22.3, easting=497812.37, northing=6521034.81)
H = 430.27
TRUE = np.array([201.4, 11.85, 1.27, 24.6])


def numpy_residuals(theta, phi, psi, sigma, x, y, water):
    """One candidate, as optimizefun_calibration computes it."""
    theta, phi, psi = np.radians(theta), np.radians(phi), np.radians(psi)
    sigma = (CAM["image_width"] / CAM["sensor_width"]) * sigma
    xi, yi = x - CAM["image_width"] / 2.0, y - CAM["image_height"] / 2.0
    st, ct, sp, cp, ss, cs = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi), np.sin(psi), np.cos(psi)
    X = (ct * cp, st * cp, sp)
    U = (st * cs - ct * sp * ss, -ct * cs - st * sp * ss, cp * ss)
    V = (-st * ss - ct * sp * cs, ct * ss - st * sp * cs, cp * cs)
    den = sigma * X[2] + xi * U[2] + yi * V[2]
    tx = H * (sigma * X[0] + xi * U[0] + yi * V[0]) / den + CAM["easting"]
    ty = H * (sigma * X[1] + xi * U[1] + yi * V[1]) / den + CAM["northing"]
    out = np.empty(len(x))
    for a in range(0, len(x), 64):
        dx = water[None, :, 0] - tx[a:a + 64, None]
        dy = water[None, :, 1] - ty[a:a + 64, None]
        out[a:a + 64] = np.sqrt(np.min(dx * dx + dy * dy, axis=1))
    return out, tx, ty


def make_scene(points, vertices):
    rng = np.random.default_rng(11)
    t = np.sort(rng.uniform(0.0, 1.0, vertices))
    xd, yd = 120.0 + 3200.0 * t, 1350.0 + 380.0 * np.sin(3.0 * t + 1.0) ** 2 + 250.0 * t
    _, wx, wy = numpy_residuals(*TRUE, xd, yd, np.zeros((1, 2)))
    pick = np.sort(rng.choice(vertices, points, replace=False))
    return xd[pick] + rng.normal(0, 1.0, points), yd[pick] + rng.normal(0, 1.0, points), np.stack([wx, wy], 1)


def workbook_rows():
    """240 overlapping boxes from 2 x 4 x 10 x 3 starts: the size of the reference's calibration workbook."""
    rows = []
    for i, j, k, m in itertools.product(range(2), range(4), range(10), range(3)):
        mid = TRUE + np.array([-2.0 + 4.0 * i, -1.5 + 1.0 * j, -0.9 + 0.2 * k, -1.0 + 1.0 * m])
        rows.append(np.stack([mid - [4.0, 1.5, 1.0, 1.5], mid + [4.0, 1.5, 1.0, 1.5]], 1).ravel())
    return np.array(rows)


def inner_loop_mix():
    """Mnemonic counts of the blocks of k_calib.hip's device code that loop on themselves around a batch of scalar
    vertex loads, one entry per kernel."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k_calib.s")
        subprocess.check_call([icelk_build._hipcc()] + icelk_build.FLAGS + ["--cuda-device-only", "-S",
                              os.path.join(icelk_build.CSRC, "k_calib.hip"), "-o", asm])
        text = open(asm).read()
    found = []
    for label, body in re.findall(r"^(\.LBB\d+_\d+):[^\n]*\n(.*?)(?=^\.L|\Z)", text, flags=re.S | re.M):
        if "s_load_dwordx16" in body and re.search(r"s_cbranch_\w+\s+" + re.escape(label) + r"\b", body):
            ops = [m.split()[0] for m in body.splitlines() if m.startswith("\t") and not m.strip().startswith((";", "."))]
            found.append(collections.Counter(ops))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=180)
    ap.add_argument("--vertices", type=int, default=5000)
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_cost.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    x, y, water = make_scene(a.points, a.vertices)
    rows = workbook_rows()
    lo, hi = rows[:, 0::2].min(axis=0), rows[:, 1::2].max(axis=0)
    say("tools/calib_bench.py --points %d --vertices %d --lattice %d --repeat %d; numpy %s"
        % (a.points, a.vertices, a.lattice, a.repeat, np.__version__))
    ctx = Context(64, 64, n_slots=1, max_pts=1024)
    try:
        with ShorelineScene(ctx, x, y, water, **CAM) as scene:
            bounds = list(zip(lo, hi))
            scene.lattice(bounds, 8, H)                                       # warm-up: code object, allocations
            kern, pairs = [], 0
            for _ in range(a.repeat):
                timing = {}
                axes, cost = scene.lattice(bounds, a.lattice, H, timing=timing)
                kern.append(timing["kernels_ms"])
                pairs = timing["pairs"]
            say("lattice %d^4 = %d candidates x %d points x %d vertices = %.3e point pairs (icelk_calib_cost, %d launches)"
                % (a.lattice, a.lattice ** 4, a.points, a.vertices, pairs, -(-a.lattice ** 4 // (1 << 18))))
            say("  kernels (HIP events): best %.1f ms of %d (%.1f .. %.1f) = %.3e point pairs/s"
                % (min(kern), a.repeat, min(kern), max(kern), pairs / (min(kern) * 1e-3)))
            # a subset of the lattice in numpy
            rng = np.random.default_rng(3)
            sub = rng.choice(cost.size, 48, replace=False)
            idx = np.unravel_index(sub, cost.shape)
            t = time.perf_counter()
            ref = np.array([np.mean(numpy_residuals(axes[0][i], axes[1][j], axes[2][k], axes[3][m], x, y, water)[0] ** 2)
                            ** 0.5 for i, j, k, m in zip(*idx)])
            t_np = time.perf_counter() - t
            if not np.array_equal(ref, cost.ravel()[sub], equal_nan=True):
                raise SystemExit("device lattice differs from numpy's")
            np_rate = 48 * a.points * a.vertices / t_np
            say("  numpy, one core, 48 of the nodes: %.1f ms each = %.3e point pairs/s; equal bit for bit; the whole "
                "lattice would take %.0f s; kernels vs numpy: %.0fx"
                % (t_np / 48 * 1e3, np_rate, pairs / np_rate, pairs / np_rate / (min(kern) * 1e-3)))
            # one launch of the fit: 240 points and their four neighbours each
            cand = np.repeat((rows[:, 0::2] + rows[:, 1::2]) / 2, 5, axis=0)
            for j in range(4):
                cand[j + 1::5, j] *= 1.0 + 1.5e-8
            scene.residuals(*cand.T, H)
            kern = []
            for _ in range(a.repeat):
                timing = {}
                res = scene.residuals(*cand.T, H, timing=timing)
                kern.append(timing["kernels_ms"])
            say("residuals of 5 x 240 = %d candidates = %.3e point pairs (icelk_calib_residuals, one launch)"
                % (len(cand), timing["pairs"]))
            say("  kernel (HIP events): best %.3f ms of %d (%.3f .. %.3f) = %.3e point pairs/s"
                % (min(kern), a.repeat, min(kern), max(kern), timing["pairs"] / (min(kern) * 1e-3)))
            if not np.array_equal(res[7], numpy_residuals(*cand[7], x, y, water)[0], equal_nan=True):
                raise SystemExit("device residuals differ from numpy's")
            fit = dict(lattice_n=16, top_k=8, refine=2)
            calibrate(scene, H, rows, **fit)
            wall = []
            for _ in range(a.repeat):
                t = time.perf_counter()
                result = calibrate(scene, H, rows, **fit)
                wall.append(time.perf_counter() - t)
            say("calibrate: 240 boxes + 16^4 lattice, 8 lattice seeds, 2 refinement rounds (%d seeds, %d iterations in "
                "all, best rmse %.4f m)" % (len(result.rmse), int(result.iterations.sum()), result.rmse[result.best]))
            say("  whole call (host clock): best %.1f ms of %d (%.1f .. %.1f)"
                % (min(wall) * 1e3, a.repeat, min(wall) * 1e3, max(wall) * 1e3))
    finally:
        ctx.close()
    for k, mix in enumerate(inner_loop_mix()):
        valu = sum(n for op, n in mix.items() if op.startswith("v_"))
        say("inner loop %d (8 vertices a pass): %s; %d vector instructions = %.3f per point pair"
            % (k, ", ".join("%d %s" % (n, op) for op, n in sorted(mix.items())), valu, valu / 8.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

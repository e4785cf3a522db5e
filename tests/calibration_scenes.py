"""What the calibration tests on the CPU and on the GPU share.  Seeded synthetic scenes for the fit tests: a shoreline curve in the lower half of a
3456 x 2304 photo, where `den` of the projection is positive for every parameter set of the boxes, its projection under
known parameters as the waterline, and a subset of the curve's points -- with or without digitising noise -- as the
shoreline points; the conditions a fit has to meet; the scipy fit the noisy bound refers to; the golden file."""
import os

import numpy as np

import calibration_restatement as R

CAM = dict(imwidth=3456, imheight=2304, sensor_width=22.3, E=497812.37, N=6521034.81)
H = 430.27

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibration_golden.npz")
FIT = dict(lattice_n=5, top_k=8, refine=3)      # what the fit tests run with, on the CPU and on the device


def same_bits(a, b):
    """Equal bit for bit where neither is NaN, NaN in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def golden_scene(g, name):
    cam = dict(zip(g["cam_keys"].tolist(), g["cam_values"].tolist()))
    scene = R.Scene(g[name + "_x"], g[name + "_y"], g[name + "_water"], cam["imwidth"], cam["imheight"],
                    cam["sensor_width"], cam["E"], cam["N"])
    return cam, scene


def make(seed, noise_px=0.0, M=60, W=1500):
    """dict(scene = the restatement's Scene, true = (theta, phi, psi, sigma), rows = three overlapping boxes in
    the workbook's layout, x, y, water)."""
    rng = np.random.default_rng(seed)
    true = np.array([201.4, 11.85, 1.27, 24.6]) + rng.uniform(-1, 1, 4) * np.array([3.0, 1.0, 0.6, 0.8])
    a, b, c = rng.uniform(250, 450), rng.uniform(2.0, 4.0), rng.uniform(0, 3)
    t = np.sort(rng.uniform(0.0, 1.0, W))          # irregular spacing, as a hand-digitised line has
    xd = 120.0 + 3200.0 * t
    yd = 1350.0 + a * np.sin(b * t + c) ** 2 + 250.0 * t
    wx, wy = R.project(*true, H, xd, yd, CAM["imwidth"], CAM["imheight"], CAM["sensor_width"], CAM["E"], CAM["N"])
    water = np.stack([wx, wy], 1)
    pick = np.sort(rng.choice(W, M, replace=False))
    x = xd[pick] + rng.normal(0, noise_px, M) if noise_px else xd[pick].copy()
    y = yd[pick] + rng.normal(0, noise_px, M) if noise_px else yd[pick].copy()
    half = np.array([5.0, 2.5, 2.0, 2.0])
    rows = []
    for _ in range(3):
        mid = true + rng.uniform(-0.6, 0.6, 4) * half
        rows.append(np.stack([mid - half, mid + half], 1).ravel())
    scene = R.Scene(x, y, water, CAM["imwidth"], CAM["imheight"], CAM["sensor_width"], CAM["E"], CAM["N"])
    return dict(scene=scene, true=true, rows=np.array(rows), x=x, y=y, water=water)


def union_box(rows):
    rows = np.asarray(rows)
    return rows[:, 0::2].min(axis=0), rows[:, 1::2].max(axis=0)


def scipy_best_rmse(scene, seeds, lower, upper):
    """The smallest final rmse of scipy.optimize.least_squares (bounded, default tolerances) on the restatement,
    started from each of `seeds`."""
    from scipy.optimize import least_squares
    best = np.inf
    for s in seeds:
        s = np.clip(s, lower + 1e-9, upper - 1e-9)
        fit = least_squares(lambda p: scene.evaluate(p[0], p[1], p[2], p[3], H)[0], s, bounds=(lower, upper))
        best = min(best, float(np.mean(fit.fun ** 2) ** 0.5))
    return best


def fit_conditions(result, scene, true, noise):
    """What the issue asks of a fit; prints every figure before it asserts."""
    print("rmse", result.rmse, "seed rmse", result.seed_rmse, "iterations", result.iterations, "best", result.best)
    ok = ~np.isnan(result.seed_rmse)
    assert (result.rmse[ok] <= result.seed_rmse[ok]).all()          # a step is taken only when it improves
    best = result.rmse[result.best]
    if not noise:
        assert best <= 0.005
        tx0, ty0 = scene.project(*true, H)
        tx1, ty1 = scene.project(*result.params[result.best], H)
        shift = np.hypot(tx0 - tx1, ty0 - ty1).max()
        print("largest shift of a projected shoreline point", shift)
        assert shift <= 0.005
    return best

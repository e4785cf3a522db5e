#!/usr/bin/env python3
"""Generates tests/golden/calibration_golden.npz by RUNNING THE REFERENCE (development container only).

What runs: the reference's own `optimizefun_calibration` (s0_2_camera_calibration.py:240-275) with its `photo_to_utm`
(117-152) and `closest_node` (231-238), imported from /root/reference, on synthetic scenes made here.  What is
committed: only this script and the data it produced (inputs + the reference's outputs) -- no reference source.

Absent from the image and NOT emulated: `shapefile` (pyshp) and `geopandas`, which s0_2 imports at module level and the
three functions never touch -- empty placeholder modules let the import statements pass; and lmfit, whose Parameters
object the misfit only asks for `.valuesdict()`: a four-line object with that method stands in.

Per scene: the inputs, about 60 candidates (theta, phi, psi, sigma, H), and per candidate the reference's residual
vector, the tx, ty of photo_to_utm, np.mean(res ** 2) and its ** 0.5.  Scenes: a (M = 1, W = 1); b (M = 7, W = 129,
duplicated vertices, points equidistant from two vertices); c (M = 180, W = 5000).  The candidates include phi / psi
for which `den` changes sign across the points, phi = psi = 0 with a point on the image's middle row (den exactly 0),
NaN parameters and theta beyond +-360.

Usage (development container):  python tests/golden/make_calibration_golden.py
"""
import os
import sys
import types
import warnings

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "calibration_golden.npz")

CAM = dict(imwidth=3456, imheight=2304, sensor_width=22.3, E=497812.37, N=6521034.81)
TRUE = dict(theta=201.4, phi=11.85, psi=1.27, sigma=24.6, H=430.27)


class Params:
    def __init__(self, **values):
        self.values = values

    def valuesdict(self):
        return dict(self.values)


def candidates(rng, n):
    """(n, 5) theta, phi, psi, sigma, H: a cloud around TRUE and the special cases of the docstring."""
    base = np.array([TRUE[k] for k in ("theta", "phi", "psi", "sigma", "H")])
    c = base + rng.normal(0, 1, (n, 5)) * np.array([4.0, 2.0, 1.5, 1.2, 0.8])
    c[0] = base
    c[1, 1:3] = 0.0, 0.0                       # den = yi exactly: 0 for a point on the middle row
    c[2, 1:3] = 3.0, 0.0                       # den changes sign across the points
    c[3, 1:3] = -2.5, 40.0
    c[4, 1:3] = 0.5, -75.0
    c[5, 0] = np.nan
    c[6, 3] = np.nan
    c[7, 4] = np.nan
    c[8, 0] = base[0] + 360.0
    c[9, 0] = base[0] - 720.0
    c[10, 0] = 1234.5
    c[11, 1] = 90.0
    c[12, 3] = 0.0                             # sigma 0: den from the points alone
    c[13, 4] = 0.0                             # H 0: everything projects onto the camera position
    c[14, 1:3] = 0.0, 90.0                     # den = xi exactly
    return c


def scene_a(rng):
    x, y = np.array([1700.0]), np.array([1500.0])
    return x, y, np.array([[CAM["E"] - 800.0, CAM["N"] - 2100.0]])


def scene_b(rng):
    # vertices on an integer lattice around the area the points fall into, every vertex twice in places: exact ties
    x = np.array([400.0, 1728.0, 1728.0, 2000.0, 3000.0, 100.0, 3456.0])
    y = np.array([1400.0, 1152.0, 2000.0, 1152.0, 1700.0, 2304.0, 1300.0])       # 1152: the middle row
    gx, gy = np.meshgrid(np.arange(8), np.arange(8))
    w = np.stack([CAM["E"] - 2000.0 + 500.0 * gx.ravel(), CAM["N"] - 6000.0 + 750.0 * gy.ravel()], 1)
    w = np.concatenate([w, w[::-1], w[17:18]])                                    # 64 + 64 + 1 = 129
    return x, y, w


def scene_c(rng, ooc):
    # a shoreline across the lower part of the photo; the waterline is its projection under TRUE, densified and
    # displaced by a few metres, so the distances look like those of a real calibration
    s = np.sort(rng.uniform(0, 1, 180))
    x = 150.0 + 3150.0 * s + rng.normal(0, 1.0, 180)
    y = 1500.0 + 500.0 * np.sin(3.0 * s) ** 2 + 120.0 * s + rng.normal(0, 1.0, 180)
    y[17] = 1152.0
    t = np.linspace(0, 1, 5000)
    xd = 100.0 + 3250.0 * t
    yd = 1500.0 + 500.0 * np.sin(3.0 * t) ** 2 + 120.0 * t
    cam = dict(theta=np.radians(TRUE["theta"]), phi=np.radians(TRUE["phi"]), psi=np.radians(TRUE["psi"]),
               sigma=(CAM["imwidth"] / CAM["sensor_width"]) * TRUE["sigma"])
    tx, ty = ooc.photo_to_utm(xd - CAM["imwidth"] / 2.0, yd - CAM["imheight"] / 2.0, CAM["E"], CAM["N"], TRUE["H"], cam)
    w = np.stack([tx, ty], 1) + rng.normal(0, 2.0, (5000, 2))
    return x, y, w


def main():
    sys.path.insert(0, REF)
    for name in ("shapefile", "geopandas"):
        sys.modules[name] = types.ModuleType(name)      # placeholders, see the docstring
    import s0_2_camera_calibration as s0_2
    rng = np.random.default_rng(20240902)
    out = {"cam_keys": np.array(sorted(CAM)), "cam_values": np.array([float(CAM[k]) for k in sorted(CAM)])}
    scenes = dict(a=scene_a(rng), b=scene_b(rng), c=scene_c(rng, s0_2))
    for name, (x, y, w) in scenes.items():
        cand = candidates(rng, 60)
        res, txs, tys = [], [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for th, ph, ps, sg, H in cand.tolist():
                p = Params(theta=th, phi=ph, psi=ps, sigma=sg, H=H)
                d = s0_2.optimizefun_calibration(p, x, y, CAM["imwidth"], CAM["imheight"], CAM["sensor_width"],
                                                 CAM["E"], CAM["N"], w)
                cam = dict(theta=np.radians(th), phi=np.radians(ph), psi=np.radians(ps),
                           sigma=(CAM["imwidth"] / CAM["sensor_width"]) * sg)
                tx, ty = s0_2.photo_to_utm(x - CAM["imwidth"] / 2.0, y - CAM["imheight"] / 2.0, CAM["E"], CAM["N"], H,
                                           cam)
                res.append(np.array(d))
                txs.append(tx)
                tys.append(ty)
        res = np.array(res)
        out.update({name + "_x": x, name + "_y": y, name + "_water": w, name + "_cand": cand, name + "_res": res,
                    name + "_tx": np.array(txs), name + "_ty": np.array(tys),
                    name + "_meansq": np.array([np.mean(r ** 2) for r in res]),
                    name + "_rmse": np.array([np.mean(r ** 2) ** 0.5 for r in res])})
        print(name, "M", len(x), "W", len(w), "NaN", int(np.isnan(res).sum()), "inf", int(np.isinf(res).sum()),
              "median", float(np.nanmedian(res)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays; numpy", np.__version__)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/ortho_golden.npz by RUNNING THE REFERENCE's Camera.utm_to_photo,
photocords_uncropped_to_cropped, photo_to_utm and project_vectorfield_to_utm (imports/camtools.py:286-430) in the
development container.  Committed: this script and the data (calibrations and map points in, photo coordinates out); no
reference source.

As in make_utm_golden.py and make_mask_golden.py, `shapefile` is an empty placeholder (imported at camtools.py:16, used
by none of these methods) and the Camera instance is created with __new__, its `cam` / `pic` dictionaries filled with the
same expressions and numpy scalar types as Camera.__init__ (camtools.py:127-179).

Three cameras, each on a raster of at most 64 x 48 cells whose centres are tx = x0 + i res, ty = y0 - j res:
  down     the calibration of make_utm_golden.py with phi = +11.85: the optical axis points below the horizon
  up       the same with phi = -11.85: the water is behind the image plane, every hit inside the frame is a mirror point
  rolled   a rolled camera with crops on both axes and a tide

Usage (development container):  python tests/golden/make_ortho_golden.py
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ortho_golden.npz")

BASE = dict(image_width=3456, image_height=2304, sensor_width=22.3, easting=497812.37, northing=6521034.81,
            elevation=431.62, antenna_height=1.35, theta=201.4, phi=11.85, psi=1.27, sigma=24.6,
            crop_left=0, crop_right=0, crop_top=1000, crop_bottom=4)

CAMERAS = [
    # name, calibration, tide or None, raster (dx0, dy0 of the top-left centre relative to the camera, res, width, height)
    ("down", dict(BASE), None, (-3000.0, 900.0, 50.0, 64, 48)),
    ("up", dict(BASE, phi=-11.85), None, (-150.0, 1450.0, 50.0, 64, 48)),
    ("rolled", dict(BASE, theta=33.7, phi=9.4, psi=-7.3, crop_left=200, crop_right=100, crop_top=300, crop_bottom=50,
                    elevation=212.4), 0.8125, (-400.0, 2600.0, 62.5, 60, 45)),
]


def camera_dicts(calib, tide):
    """cam / pic exactly as Camera.__init__ builds them (camtools.py:127-179)."""
    p = {k: (np.int64(v) if isinstance(v, int) else np.float64(v)) for k, v in calib.items()}
    cam, pic = {}, {}
    pic["width"] = p["image_width"]
    pic["height"] = p["image_height"]
    cam["chipsize"] = p["sensor_width"]
    cam["E"] = p["easting"]
    cam["N"] = p["northing"]
    cam["H"] = p["elevation"] - p["antenna_height"]
    cam["theta"] = np.radians(p["theta"])
    cam["phi"] = np.radians(p["phi"])
    cam["psi"] = np.radians(p["psi"])
    cam["sigma"] = (pic["width"] / cam["chipsize"]) * p["sigma"]
    pic["cropleft"] = p["crop_left"]
    pic["cropright"] = p["crop_right"]
    pic["croptop"] = p["crop_top"]
    pic["cropbottom"] = p["crop_bottom"]
    if tide is not None:
        cam["H"] = cam["H"] - float(tide)
    return cam, pic


def main():
    sys.path.insert(0, REF)
    sys.modules["shapefile"] = types.ModuleType("shapefile")   # placeholder, see the docstring
    import imports.camtools as ct
    rng = np.random.default_rng(20261021)
    out = {"names": np.array([c[0] for c in CAMERAS]), "calib_keys": np.array(sorted(BASE))}
    for name, calib, tide, (dx0, dy0, res, width, height) in CAMERAS:
        cam = ct.Camera.__new__(ct.Camera)
        cam.cam, cam.pic = camera_dicts(calib, tide)
        x0, y0 = float(calib["easting"]) + dx0, float(calib["northing"]) + dy0
        j, i = np.mgrid[0:height, 0:width]
        tx = x0 + i.astype(np.float64) * res
        ty = y0 - j.astype(np.float64) * res
        with np.errstate(all="ignore"):
            x, y = cam.utm_to_photo(tx, ty)
            xs, ys = cam.photocords_uncropped_to_cropped(x, y)
            bx, by = cam.photo_to_utm(x, y)   # the hit projected forward again
        out[name + "_calib"] = np.array([float(calib[k]) for k in sorted(BASE)], np.float64)
        out[name + "_tide"] = np.array(np.nan if tide is None else tide, np.float64)
        out[name + "_raster"] = np.array([x0, y0, res, width, height], np.float64)
        for key, v in (("tx", tx), ("ty", ty), ("x", x), ("y", y), ("xs", xs), ("ys", ys), ("back_tx", bx), ("back_ty", by)):
            out["%s_%s" % (name, key)] = np.asarray(v, np.float64)
        # a vector field on the cropped frame's lower part, as s3 would hand it over in uncropped coordinates
        n = 200
        px = rng.uniform(0, float(calib["image_width"]), n)
        py = rng.uniform(float(calib["image_height"]) * 0.55, float(calib["image_height"]), n)
        u, v = rng.normal(0, 6.0, n), rng.normal(0, 6.0, n)
        with np.errstate(all="ignore"):
            field = cam.project_vectorfield_to_utm(px, py, u, v)
        out[name + "_field_in"] = np.stack([px, py, u, v])
        out[name + "_field_out"] = np.stack([np.asarray(a, np.float64) for a in field])
        w = int(calib["image_width"]) - int(calib["crop_left"]) - int(calib["crop_right"])
        h = int(calib["image_height"]) - int(calib["crop_top"]) - int(calib["crop_bottom"])
        with np.errstate(invalid="ignore"):
            inside = (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1)
        print(name, tx.shape, "inside the cropped frame:", int(inside.sum()), "of", inside.size)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays; numpy", np.__version__)


if __name__ == "__main__":
    main()

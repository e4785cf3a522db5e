"""An independent numpy statement of the orthophoto's rules (csrc/ortho.h), written from the rules and not
from the header: whole-array expressions in the reference's order (camtools.py:347-390, 427-428), numpy's element-wise
double arithmetic (no fused multiply-add), integer sampling weights.  tests/test_ortho_host.py holds the host statement to
it byte for byte (rgb, cover) and bit for bit (best)."""
import numpy as np

SAMPLING = ("bilinear", "nearest")


def coords(cam, raster, size, max_range=0.0):
    """cam: the dict of CameraModel.as_dict(); size = (sw, sh).  dict(xs, ys, d2, seen) of (height, width) arrays."""
    f = np.float64
    X, U, V = (np.asarray(cam[k], f) for k in ("X", "U", "V"))
    sigma, H, E, N = f(cam["sigma"]), f(cam["H"]), f(cam["E"]), f(cam["N"])
    sw, sh = size
    j, i = np.mgrid[0:raster["height"], 0:raster["width"]]
    tx = f(raster["x0"]) + i.astype(f) * f(raster["res"])
    ty = f(raster["y0"]) - j.astype(f) * f(raster["res"])
    with np.errstate(all="ignore"):
        tx = tx - E
        ty = ty - N
        a = U[2] / H * tx - U[0]
        b = V[2] / H * tx - V[0]
        c = U[2] / H * ty - U[1]
        d = V[2] / H * ty - V[1]
        p = sigma * (X[0] - X[2] / H * tx)
        q = sigma * (X[1] - X[2] / H * ty)
        den = a * d - b * c
        xi = (d * p - b * q) / den
        yi = (-c * p + a * q) / den
        xs = xi + f(cam["half_w"]) - f(cam["crop_left"])
        ys = yi + f(cam["half_h"]) - f(cam["crop_top"])
        w = sigma * X[2] + xi * U[2] + yi * V[2]
        d2 = tx * tx + ty * ty
        seen = (den != 0) & (w != 0) & ((w > 0) == (H > 0)) & (H != 0)
        if max_range > 0:
            seen &= d2 <= f(max_range) * f(max_range)
        seen &= (xs >= 0) & (xs <= sw - 1) & (ys >= 0) & (ys <= sh - 1)
    return dict(xs=xs, ys=ys, d2=d2, seen=seen)


def sample(img, xs, ys, sampling):
    """img (h, w) or (h, w, 3) uint8; xs, ys 1-D, inside the image -> (n, 3) uint8"""
    src = img[:, :, None] if img.ndim == 2 else img
    sh, sw = src.shape[:2]
    fx = np.floor(xs * 256.0).astype(np.int64)
    fy = np.floor(ys * 256.0).astype(np.int64)
    if sampling == "nearest":
        out = src[(fy + 128) >> 8, (fx + 128) >> 8]
    else:
        ix, iy, ax, ay = fx >> 8, fy >> 8, (fx & 255)[:, None], (fy & 255)[:, None]
        ix1, iy1 = np.minimum(ix + 1, sw - 1), np.minimum(iy + 1, sh - 1)
        p00, p10, p01, p11 = (src[r, c].astype(np.int64) for r, c in ((iy, ix), (iy, ix1), (iy1, ix), (iy1, ix1)))
        acc = (256 - ax) * (256 - ay) * p00 + ax * (256 - ay) * p10 + (256 - ax) * ay * p01 + ax * ay * p11 + 32768
        out = (acc >> 16).astype(np.uint8)
    return np.repeat(out, 3, axis=1) if out.shape[1] == 1 else out


def orthophoto(views, raster, max_range=0.0, sampling="bilinear", fill=(255, 255, 255)):
    """views: [(CameraModel, pixels)].  dict(rgb, cover, best)"""
    assert sampling in SAMPLING
    shape = (raster["height"], raster["width"])
    rgb = np.empty(shape + (3,), np.uint8)
    rgb[...] = np.asarray(fill, np.uint8)
    cover = np.zeros(shape, np.uint8)
    best = np.full(shape, np.inf)
    for index, (camera, img) in enumerate(views):
        c = coords(camera.as_dict(), raster, (img.shape[1], img.shape[0]), max_range)
        take = c["seen"] & (c["d2"] < best)
        rgb[take] = sample(img, c["xs"][take], c["ys"][take], sampling)
        cover[take] = index + 1
        best[take] = c["d2"][take]
    return dict(rgb=rgb, cover=cover, best=best)

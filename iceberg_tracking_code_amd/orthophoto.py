"""The orthophoto: camera photographs rectified onto a map raster -- the inverse direction of `utm.project_tracks`.

Every cell of the raster is projected into the photograph by the reference's `Camera.utm_to_photo` (camtools.py:334-392)
and its crop offsets (camtools.py:423-430), sampled there, and the cameras are merged into one mosaic in which the nearest
camera wins.  The rule is csrc/ortho.h; the per-pixel work runs in the HIP kernel `k_ortho_add`
(csrc/k_ortho.hip) through `Context.ortho_begin / ortho_add / ortho_write`, and the picture leaves through the picture
writer, so a PNG holds the pixels exactly, a JPEG is what Pillow writes of them, and `MovieWriter.add_picture` makes a
movie frame of it.  Here are the host-only parts: the raster of a map view, the world file, the host statement and the
drivers.  There is no CPU fallback: `orthophoto_host` is the statement tests compare the device against.

What the picture is not: nothing is averaged where a raster cell covers many source pixels, and there is no terrain --
everything is taken at sea level, as in the reference.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from .jpeg import UnsupportedJpeg

SAMPLING = {"bilinear": 0, "nearest": 1}
FORMATS = {"jpeg": 0, "png": 1}
_EXT = {"png": ("png", "pgw"), "jpeg": ("jpg", "jgw")}


def ortho_raster(limits, res):
    """The raster that covers (xmin, xmax, ymin, ymax) -- `velocity_map.map_view`'s limits -- with cells of `res` metres:
    dict(x0, y0, res, width, height), (x0, y0) the centre of the top-left pixel."""
    xmin, xmax, ymin, ymax = (float(v) for v in limits)
    res = float(res)
    if not (res > 0 and xmax > xmin and ymax > ymin):
        raise ValueError("res <= 0 or empty limits")
    return dict(x0=xmin + res / 2, y0=ymax - res / 2, res=res, width=int(math.ceil((xmax - xmin) / res)),
                height=int(math.ceil((ymax - ymin) / res)))


def raster_struct(raster):
    r = raster if isinstance(raster, dict) else dict(zip(("x0", "y0", "res", "width", "height"), raster))
    return _lib.OrthoRaster(float(r["x0"]), float(r["y0"]), float(r["res"]), int(r["width"]), int(r["height"]))


def opts_struct(max_range=0.0, sampling="bilinear", fill=(255, 255, 255)):
    if sampling not in SAMPLING:
        raise ValueError("sampling is 'bilinear' or 'nearest'")
    f = [int(v) for v in fill]
    if len(f) != 3 or min(f) < 0 or max(f) > 255:
        raise ValueError("fill is three values in 0 .. 255")
    return _lib.OrthoOpts(float(max_range), SAMPLING[sampling], (C.c_uint8 * 3)(*f))


def world_file(raster):
    """The six lines of the ESRI world file of a raster: res, 0, 0, -res, x0, y0 -- repr's digits, which parse back to
    the same doubles."""
    r = raster_struct(raster)
    return "".join("%s\n" % repr(float(v)) for v in (r.res, 0.0, 0.0, -r.res, r.x0, r.y0))


def read_world_file(text):
    """(x0, y0, res) of a north-up world file `world_file` wrote."""
    a, d, b, e, c, f = (float(v) for v in text.split())
    if d != 0 or b != 0 or e != -a:
        raise ValueError("not a north-up world file with square cells")
    return c, f, a


def _source_array(source):
    """A source given as pixels -> a C-contiguous (h, w) or (h, w, 3) uint8 array, else None."""
    if isinstance(source, np.ndarray):
        a = np.ascontiguousarray(source, dtype=np.uint8)
        if a.ndim == 3 and a.shape[2] == 1:
            a = np.ascontiguousarray(a[:, :, 0])
        if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
            raise ValueError("a source array is (h, w) or (h, w, 3) uint8")
        return a
    return None


def _source_bytes(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if isinstance(source, (str, os.PathLike)):
        with open(source, "rb") as f:
            return f.read()
    return None


def decode_with_pillow(data):
    """A JPEG the device refuses, opened with PIL as the folder driver does: gray stays gray, everything else is R G B."""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.asarray(im if im.mode == "L" else im.convert("RGB"))


def ortho_coords_host(camera, raster, size, max_range=0.0):
    """dict(xs, ys, d2: (height, width) float64, seen: (height, width) bool) of every raster pixel for a camera whose
    source is size = (sw, sh) samples (icelk_ortho_coords_host): the cropped frame's coordinates, bit for bit the
    reference's `utm_to_photo` + `photocords_uncropped_to_cropped`."""
    r = raster_struct(raster)
    cam = camera.struct()
    shape = (max(r.height, 0), max(r.width, 0))
    xs, ys, d2 = (np.zeros(shape, np.float64) for _ in range(3))
    seen = np.zeros(shape, np.uint8)
    rc = _lib.load().icelk_ortho_coords_host(C.byref(cam), C.byref(r), int(size[0]), int(size[1]), float(max_range),
                                             xs.ctypes.data_as(_lib.f64p), ys.ctypes.data_as(_lib.f64p),
                                             d2.ctypes.data_as(_lib.f64p), seen.ctypes.data_as(_lib.u8p))
    if rc != _lib.OK:
        raise ValueError("a raster with res <= 0, a non-finite number, or a source outside 1 .. 65535 a side")
    return dict(xs=xs, ys=ys, d2=d2, seen=seen.astype(bool))


def orthophoto_host(views, raster, max_range=0.0, sampling="bilinear", fill=(255, 255, 255)):
    """The host statement (icelk_ortho_begin_host / icelk_ortho_add_host): `views` is [(CameraModel, pixels)], pixels an
    (h, w) or (h, w, 3) uint8 array.  dict(rgb (height, width, 3) uint8, cover (height, width) uint8, best (height, width)
    float64)."""
    L = _lib.load()
    r, o = raster_struct(raster), opts_struct(max_range, sampling, fill)
    shape = (max(r.height, 1), max(r.width, 1))
    rgb, cover, best = np.empty(shape + (3,), np.uint8), np.empty(shape, np.uint8), np.empty(shape, np.float64)
    u8, f64 = _lib.u8p, _lib.f64p
    if L.icelk_ortho_begin_host(C.byref(r), C.byref(o), rgb.ctypes.data_as(u8), rgb.strides[0], cover.ctypes.data_as(u8),
                                cover.strides[0], best.ctypes.data_as(f64)) != _lib.OK:
        raise ValueError("a raster with res <= 0, a non-finite number or a side below 1")
    for index, (camera, pixels) in enumerate(views):
        a = _source_array(pixels)
        if a is None:
            raise ValueError("the host statement takes pixels")
        cam = camera.struct()
        rc = L.icelk_ortho_add_host(C.byref(r), C.byref(o), C.byref(cam), index, a.ctypes.data, a.shape[1], a.shape[0],
                                    1 if a.ndim == 2 else 3, a.strides[0], rgb.ctypes.data_as(u8), rgb.strides[0],
                                    cover.ctypes.data_as(u8), cover.strides[0], best.ctypes.data_as(f64))
        if rc != _lib.OK:
            raise ValueError("more than 255 cameras, a non-finite camera or a source outside 1 .. 65535 a side")
    return dict(rgb=rgb, cover=cover, best=best)


def orthophoto(ctx, views, raster, max_range=0.0, sampling="bilinear", fill=(255, 255, 255), format=None, quality=90):
    """The mosaic of `views` = [(CameraModel, source)] on `raster`, on the device.  A source is the bytes of a JPEG file, a
    path to one, an (h, w) or (h, w, 3) uint8 array, or ("slot", k): the frame slot k holds.  View i is camera index i: of
    the cameras that see a pixel the nearest gives it its colour.  A JPEG the device decoder refuses (`UnsupportedJpeg`) is
    opened with PIL and added as pixels.  format: None, "png" or "jpeg" (at `quality`).  Returns dict(rgb (height, width, 3)
    uint8, cover (height, width) uint8: 0 or 1 + the index of the camera, file: bytes or None)."""
    ctx.ortho_begin(raster, max_range, sampling, fill)
    for index, (camera, source) in enumerate(views):
        try:
            ctx.ortho_add(camera, index, source)
        except UnsupportedJpeg:
            ctx.ortho_add(camera, index, decode_with_pillow(_source_bytes(source)))
    return ctx.ortho_write(format, quality)


def ortho_movie_name(res):
    """'ortho_<res>m.avi'"""
    return "ortho_{:g}m.avi".format(float(res))


def orthophoto_sequence(frames, target_dir, raster, max_range=0.0, sampling="bilinear", fill=(255, 255, 255), format="png",
                        quality=90, movie=False, ctx=None):
    """`frames` yields (name, views): every mosaic is written to target_dir as <name>_ortho.png | .jpg with its world file
    (.pgw | .jgw) beside it and, with movie=True, becomes a frame of ortho_<res>m.avi (`MovieWriter.add_picture`: the
    frame is made of the pixels still on the device).  `ctx`: the Context to run on -- the one whose slots ("slot", k)
    sources name; without one a small Context is made for the call.  Returns the paths of the pictures (and of the movie,
    last)."""
    from .context import Context
    from .movie import MovieWriter
    if format not in _EXT:
        raise ValueError("format is 'png' or 'jpeg'")
    ext, wext = _EXT[format]
    world = world_file(raster)
    res = raster_struct(raster).res
    written = []
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1024)
    writer = MovieWriter(os.path.join(target_dir, ortho_movie_name(res))) if movie else None
    try:
        for name, views in frames:
            out = orthophoto(ctx, views, raster, max_range, sampling, fill, format, quality)
            path = os.path.join(target_dir, "%s_ortho.%s" % (name, ext))
            with open(path, "wb") as f:
                f.write(out["file"])
            with open(os.path.join(target_dir, "%s_ortho.%s" % (name, wext)), "w") as f:
                f.write(world)
            written.append(path)
            if writer is not None:
                writer.add_picture(ctx)
    finally:
        if writer is not None:
            writer.close()
        if own:
            ctx.close()
    if writer is not None and writer.frames:
        written.append(writer.path)
    return written

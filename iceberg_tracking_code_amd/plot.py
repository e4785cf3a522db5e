"""The picture the reference draws of every saved segment (s1_lucaskanade_tracking.py:397-434, plot_switch = 1): the
segment's last gray frame 1200 pixels wide, every surviving track as a red line, its end point as a red dot, the frame's
time in a corner.  The device rasterises it and writes it as a JPEG file (`Context.plot_tracks`, `Context.seg_plot`,
`SegmentTracker.plot_closed`, `track_image_sequence(plots=...)`); here are the host-only parts: the size, the font, the
host statement of the rasteriser (csrc/plot_raster.h on the CPU) and the reference's file name.  DESIGN.md 7.6 has the
rules and what differs from the reference's PNG.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

PLOT_WIDTH = 1200            # the reference's 15 in x 80 dpi (s1:407,432)
PLOT_QUALITY = 90
STAMP_CHARACTERS = "0123456789-:./ "
STAMP_MAX = 48


def _stamp_arg(stamp):
    """The stamp as the C calls take it.  What they would refuse is left to them, apart from what bytes cannot carry."""
    if stamp is None:
        return b""
    if isinstance(stamp, str):
        try:
            stamp = stamp.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("stamp has characters outside %r" % STAMP_CHARACTERS)
    stamp = bytes(stamp)
    if b"\0" in stamp:
        raise ValueError("stamp has characters outside %r" % STAMP_CHARACTERS)
    return stamp


def plot_size(w, h, width=PLOT_WIDTH):
    """(Wo, Ho) of the picture of a w x h frame asked for at `width` (icelk_plot_size)."""
    ow, oh = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().icelk_plot_size(int(w), int(h), int(width), C.byref(ow), C.byref(oh)))
    return ow.value, oh.value


def plot_glyph(ch):
    """The 7 rows of a stamp character's glyph as strings of '#' and '.' (icelk_plot_glyph)."""
    rows = (C.c_uint8 * 7)()
    _lib.check(_lib.load().icelk_plot_glyph(ord(ch), rows))
    return ["".join("#" if (r >> (4 - k)) & 1 else "." for k in range(5)) for r in rows]


def _tracks3(tracks):
    t = np.ascontiguousarray(tracks, dtype=np.float32)
    if t.size == 0:
        return t.reshape(0, 1, 2)
    if t.ndim != 3 or t.shape[2] != 2:
        raise ValueError("tracks must have shape (n, vertices, 2)")
    return t


def plot_overlay_host(gray, tracks, width=PLOT_WIDTH, stamp=""):
    """The picture's R G B (Ho, Wo, 3) uint8 by the host statement of the rasteriser (icelk_plot_overlay_host): what
    `Context.plot_tracks(..., want_rgb=True)` returns for the same frame, byte for byte.  No GPU is needed."""
    g = np.asarray(gray)
    if g.dtype != np.uint8 or g.ndim != 2:
        raise ValueError("gray must be a 2-D uint8 array")
    g = np.ascontiguousarray(g)
    t = _tracks3(tracks)
    ow, oh = plot_size(g.shape[1], g.shape[0], width)
    rgb = np.empty((oh, ow, 3), np.uint8)
    _lib.check(_lib.load().icelk_plot_overlay_host(g.ctypes.data_as(_lib.u8p), g.shape[1], g.shape[0], g.strides[0],
                                                   t.ctypes.data_as(_lib.f32p), t.shape[0], t.shape[1], int(width), _stamp_arg(stamp),
                                                   rgb.ctypes.data_as(_lib.u8p), rgb.strides[0]))
    return rgb


def plot_name(plot_dir, last_image_path, track_len, track_len_sec):
    """'<plots>/<basename of the segment's last photo>_<track_len * track_len_sec>sec.jpg': the reference's name
    (s1:429-430) with .jpg for .png."""
    base = os.path.splitext(os.path.basename(str(last_image_path)))[0]
    return os.path.join(str(plot_dir), "{}_{}sec.jpg".format(base, track_len * track_len_sec))


def plot_stamp(last_image_path, track_len, track_len_sec):
    """'<basename> <track_len * track_len_sec>/<track_len_sec>': the two lines the reference annotates (s1:426-427), in the
    characters the bitmap font has."""
    base = os.path.splitext(os.path.basename(str(last_image_path)))[0]
    return "{} {}/{}".format(base, track_len * track_len_sec, track_len_sec)

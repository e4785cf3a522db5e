"""The map the reference draws of every gridded time window (s3_utm_to_gridded_utm.py:449-465; plot_switch 1:
plot_velocities_one_map, s3:471-641; plot_switch 2: plot_velocities_two_maps, s3:644-844): the grid with its unmeasured
cells filled, one arrow per measured cell coloured by speed, with switch 2 a second panel with every velocity vector of the
window, the fjord's outline, the cameras, four strings and a colour bar.  The device rasterises it and writes it as a JPEG
file or, with format="png", as a PNG file with exactly the rasterised pixels (`Context.map_draw`, `utm_to_gridded_utm(plots=...)`); here are the host-only parts: the reference's limits, the
layout of the picture in integers, the colour table, the arrow scaling, the strings, the file name, and the host statement
of the rasteriser (csrc/map_raster.h on the CPU).  DESIGN.md 7.7 has the rules and what differs from the reference's PNG.

A picture is described by a dict:
    width, height, quality, table (256, 3) uint8, texts [(px, py, str)],
    panels [dict(view=(x0, y0, w, h), bar=(bar_x0, bar_w), limits=(xmin, xmax, ymin, ymax), cells (n, 3) left top size,
                 measured (n,), outline (n, 2), arrows (n, 5) x y dx dy speed | resident=True with group=int or -1,
                 pivot 'tail' | 'mid', width, alpha, vmax, cameras (n, 2))]
and, for the cameras' inset photographs (`map_insets` places them),
    insets [dict(index = which resident thumbnail of `Context.map_inset_set`, at=(x0, y0), label=(px, py, text) | None;
                 for `map_overlay_host`: pixels = the thumbnail (h, w, 3) uint8)]
"""
import ctypes as C
import os

import numpy as np

from . import _lib

MAP_WIDTH = 1400             # the reference's 14 in x 100 dpi (s3:481,639)
MAP_QUALITY = 90
MAP_CHARACTERS = "0123456789-:./ ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz,()"
MAP_TEXT_MAX = 48
MAP_TEXTS_MAX = 16
MAP_CAMERAS_MAX = 8

# matplotlib's 'gist_rainbow' (lib/matplotlib/_cm.py, _gist_rainbow_data): position, (r, g, b)
GIST_RAINBOW = ((0.000, (1.00, 0.00, 0.16)), (0.030, (1.00, 0.00, 0.00)), (0.215, (1.00, 1.00, 0.00)), (0.400, (0.00, 1.00, 0.00)),
                (0.586, (0.00, 1.00, 1.00)), (0.770, (0.00, 0.00, 1.00)), (0.954, (1.00, 0.00, 1.00)), (1.000, (1.00, 0.00, 0.75)))


def gist_rainbow_table():
    """(256, 3) uint8: matplotlib.cm.gist_rainbow(np.arange(256), bytes=True)[:, :3], from the colour map's eight break
    points by the steps of matplotlib's lookup table (colors._create_lookup_table: the break points scaled to 0 .. 255,
    linear between neighbours; bytes are the values times 255, truncated).  matplotlib is not imported."""
    n = 256
    x = np.array([p for p, _ in GIST_RAINBOW], float) * (n - 1)
    xind = np.linspace(0, n - 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    out = np.empty((n, 3), np.uint8)
    for c in range(3):
        y = np.array([rgb[c] for _, rgb in GIST_RAINBOW], float)
        lut = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
        out[:, c] = (np.clip(lut, 0.0, 1.0) * 255).astype(np.uint8)
    return out


def scaled_arrows(u, v, exponent=0.5, factor=250):
    """trm.scale_arrows (imports/tracking_misc.py:61-74) with its quirk: `exponent` is ignored, the exponent is 0.5."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    angles = np.arctan2(v, u)
    speed = np.hypot(u, v)
    speed_scaled = (speed ** 0.5) * factor
    return [np.cos(angles) * speed_scaled, np.sin(angles) * speed_scaled]


def map_view(fjord, plot_switch=1):
    """(xmin, xmax, ymin, ymax), the reference's axis limits (s3:488-489; the two-map figure s3:662-663)."""
    fx, fy = np.asarray(fjord["x"]), np.asarray(fjord["y"])
    pad = 3000 if plot_switch == 2 else 500
    return int(np.min(fx) - pad), int(np.max(fx) + 300), int(np.min(fy) - 300), int(np.max(fy) + 300)


def map_layout(limits, out_width=MAP_WIDTH, panels=1):
    """The picture's geometry in integers: dict(width, height, scale, views=[dict(x0, y0, w, h, bar_x0, bar_w, right)]).
    A margin m = max(2, W / 100) around and between the panels; a panel is a view, a gap g = max(1, W / 200), a colour bar
    max(3, W / 70) wide and 19 k + g pixels for its labels (k = max(1, W / 400), the text scale); above the views 9 k
    pixels for the bar's title.  The scale is the same on both axes: vh = max(1, (2 vw dy + dx) / (2 dx))."""
    xmin, xmax, ymin, ymax = (int(v) for v in limits)
    W = int(out_width)
    if W < 64 or panels not in (1, 2) or xmax <= xmin or ymax <= ymin:
        raise ValueError("a picture less than 64 pixels wide, panels other than 1 and 2, or empty limits")
    k, m, bw, g = max(1, W // 400), max(2, W // 100), max(3, W // 70), max(1, W // 200)
    pw = (W - m * (panels + 1)) // panels
    vw = pw - g - bw - (19 * k + g)
    if vw < 1:
        raise ValueError("no room for a view")
    vh = max(1, (2 * vw * (ymax - ymin) + (xmax - xmin)) // (2 * (xmax - xmin)))
    top = m + 9 * k
    views = [dict(x0=m + i * (pw + m), y0=top, w=vw, h=vh, bar_x0=m + i * (pw + m) + vw + g, bar_w=bw, right=m + i * (pw + m) + pw)
             for i in range(panels)]
    return dict(width=W, height=top + vh + m, scale=k, gap=g, views=views)


def map_strings(day, start, end, cam_with_tracks, grid_size, time_window=None, min_time=None, max_time=None):
    """[datestring, timestring, camstring, gridstring] of s3:522-536 (the reference's typographic minus is '-')."""
    a, b = (min_time, max_time) if time_window == 24.0 else (start, end)
    cams = str(list(cam_with_tracks))[1:-1].replace("'", "")
    return ["Date: {}".format(day.strftime("%Y-%m-%d")), "Time: " + a.strftime("%H:%M") + "-" + b.strftime("%H:%M") + " UTC",
            ("Camera: {}" if len(cam_with_tracks) == 1 else "Cameras: {}").format(cams), "Grid spacing: {} m".format(grid_size)]


def map_name(plot_dir, start, end, time_window=None, min_time=None, max_time=None, ext=".jpg"):
    """'<plots>/%Y%m%d_%H%M-%H%M.jpg' of the window (s3:630-637, .jpg for .png; ext=".png" gives the reference's name); the
    full day (time_window 24.0) from the rounded first and last selected times."""
    a, b = (min_time, max_time) if time_window == 24.0 else (start, end)
    return os.path.join(str(plot_dir), "{}-{}{}".format(a.strftime("%Y%m%d_%H%M"), b.strftime("%H%M"), ext))


def map_corner_right(xcord, ycord, limits):
    """The reference's test for writing the strings in the right corner (s3:562, s3:778), as it stands: the second term
    compares the northing with the largest easting."""
    return bool(xcord - limits[0] <= 500 and limits[1] - ycord <= 500)


def map_text(s):
    """A string as the picture can carry it: characters without a glyph become spaces, at most 48 are kept."""
    return "".join(ch if ch in MAP_CHARACTERS else " " for ch in str(s))[:MAP_TEXT_MAX]


def _pixel(view, limits, x, y):
    """the pixel (in the picture) of a world position by the coordinate rule, or None"""
    xmin, xmax, ymin, ymax = (float(v) for v in limits)
    with np.errstate(all="ignore"):
        cx = ((np.float64(x) - xmin) * view["w"]) / (xmax - xmin)
        cy = ((ymax - np.float64(y)) * view["h"]) / (ymax - ymin)
    if not (abs(cx) < 2.0 ** 20 and abs(cy) < 2.0 ** 20):
        return None
    return view["x0"] + (int(np.floor(cx * 256)) >> 8), view["y0"] + (int(np.floor(cy * 256)) >> 8)


def map_texts(layout, limits, strings, cameras, label, vmax, plot_switch=1):
    """[(px, py, text)] of a picture: per view the four strings in the corner the reference's test picks (one map: every
    camera picks, at 0.98 of the height from the right or at 0.8 from the left; two maps: the last camera picks, at 0.98),
    `label` = (x, y, 'Camera' | 'Cameras') or None: the word beside the first camera (s3:557-559: at (x - 120, y + 50), the
    text's bottom-left corner), and on
    the colour bar vmax at its top, 0.0 at its bottom and 'Speed (m/s)' above it.  Lines are 9 k pixels apart."""
    k, g = layout["scale"], layout["gap"]
    out = []
    cameras = [tuple(c) for c in cameras]
    for view in layout["views"]:
        picks = [map_corner_right(x, y, limits) for x, y in cameras]
        if plot_switch == 2:
            picks = picks[-1:] if picks else [False]
        for right in sorted(set(picks)):
            top = view["y0"] + ((2 if right or plot_switch == 2 else 20) * view["h"]) // 100
            for n, s in enumerate(map_text(t) for t in strings):
                px = view["x0"] + view["w"] - (2 * view["w"]) // 100 - 6 * k * len(s) if right else view["x0"] + (2 * view["w"]) // 100
                out.append((px, top + 9 * k * n, s))
        if label is not None:
            at = _pixel(view, limits, label[0] - 120, label[1] + 50)
            if at is not None:
                out.append((at[0], at[1] - 7 * k, label[2]))
        lx = view["bar_x0"] + view["bar_w"] + g
        out.append((lx, view["y0"], map_text(repr(float(vmax)))))
        out.append((lx, view["y0"] + view["h"] - 7 * k, "0.0"))
        out.append((max(0, view["right"] - 66 * k), view["y0"] - 8 * k, "Speed (m/s)"))
    return out[:MAP_TEXTS_MAX]


def map_picture(fjord, grid_size, polygons_measured, polygons_not_measured, x, y, u, v, speed, strings, cameras=(), label=None,
                n_camnames=1, plot_switch=1, vectors=None, group=-1, speedthreshold_cbar=0.5, out_width=MAP_WIDTH, quality=MAP_QUALITY, table=None):
    """The picture dict of one window from what s3 hands its plotting functions: the saved polygons, the gridded x, y, u,
    v, speed, the four strings, the cameras' (easting, northing), `label` = the position of the first camera name's camera
    (None: it has none) and how many names there are.  plot_switch 2 adds the all-vectors panel on the left:
    `vectors` = (n, 5) x, y, u * interval, v * interval, speed, or None for the resident arrows of `group`."""
    limits = map_view(fjord, plot_switch)
    panels = 2 if plot_switch == 2 else 1
    layout = map_layout(limits, out_width, panels)
    cells = [np.asarray(p, np.float64).reshape(-1, 4, 2) for p in (polygons_measured, polygons_not_measured)]
    left_top = np.concatenate([c[:, 0, :] for c in cells])
    cell3 = np.column_stack([left_top, np.full(len(left_top), float(grid_size))])
    measured = np.concatenate([np.ones(len(cells[0]), np.uint8), np.zeros(len(cells[1]), np.uint8)])
    outline = np.column_stack([np.asarray(fjord["x"], np.float64), np.asarray(fjord["y"], np.float64)])
    du, dv = scaled_arrows(u, v, exponent=0.2, factor=100) if plot_switch != 2 else scaled_arrows(u, v)
    arrows = np.column_stack([np.asarray(a, np.float64).ravel() for a in (x, y, du, dv, speed)]).reshape(-1, 5)
    cams = np.asarray([tuple(c) for c in cameras][:MAP_CAMERAS_MAX], np.float64).reshape(-1, 2)
    common = dict(limits=limits, outline=outline, vmax=float(speedthreshold_cbar), cameras=cams)
    gridded = dict(common, cells=cell3, measured=measured, arrows=arrows, pivot="mid", width=8.0 if plot_switch == 2 else 4.0, alpha=1.0)
    out = []
    if plot_switch == 2:
        every = dict(common, pivot="tail", width=3.5, alpha=0.75)
        if vectors is None:
            every.update(resident=True, group=int(group))
        else:
            every.update(arrows=np.asarray(vectors, np.float64).reshape(-1, 5))
        out.append(every)
    out.append(gridded)
    for panel, view in zip(out, layout["views"]):
        panel.update(view=(view["x0"], view["y0"], view["w"], view["h"]), bar=(view["bar_x0"], view["bar_w"]))
    return dict(width=layout["width"], height=layout["height"], quality=int(quality),
                table=gist_rainbow_table() if table is None else table,
                texts=map_texts(layout, limits, strings, cams, None if label is None else (label[0], label[1], "Cameras" if n_camnames > 1 else "Camera"),
                                speedthreshold_cbar, plot_switch), panels=out)


def map_insets(layout, plot_switch, sizes):
    """Where the cameras' photographs go in a picture of `layout`, in integers from the reference's figure fractions
    (s3:614 one map: one box [0.06, 0.06, 0.2, 0.2]; s3:791-796 two maps: four boxes [0.03, 0.06 + 0.2 k, 0.18, 0.18]; left,
    bottom, width, height with the origin at the figure's bottom-left).  `sizes`: per inset the photo's (width, height), or
    None for none.  Returns per inset None or dict(box=(bw, bh), size=(tw, th) the thumbnail's by icelk_thumb_size,
    at=(x0, y0) its top-left corner -- it sits in the bottom-left corner of its box (anchor='SW') --, label_at=(px, py) the
    top-left corner of the camera's name, whose bottom-left corner is 5 % of the thumbnail's width from its left edge and
    15 % of its height below its top (annotatefun(axins, [name], 0.05, 0.85)).  One map: every inset has the one box; two
    maps: inset k has box k, more than four raise ValueError where the reference asserts."""
    from .jpeg import thumbnail_size
    W, H, k = layout["width"], layout["height"], layout["scale"]
    sizes = list(sizes)
    if plot_switch == 2 and len(sizes) > 4:
        raise ValueError("the two-map figure has room for four cameras' photographs")
    out = []
    for n, size in enumerate(sizes):
        if size is None:
            out.append(None)
            continue
        if plot_switch == 2:
            x, bw, bh, bottom = (3 * W) // 100, (18 * W) // 100, (18 * H) // 100, H - ((6 + 20 * n) * H) // 100
        else:
            x, bw, bh, bottom = (6 * W) // 100, (20 * W) // 100, (20 * H) // 100, H - (6 * H) // 100
        tw, th = thumbnail_size(size[0], size[1], (max(bw, 1), max(bh, 1)))
        y0 = bottom - th
        out.append(dict(box=(max(bw, 1), max(bh, 1)), size=(tw, th), at=(x, y0), label_at=(x + (5 * tw) // 100, y0 + (15 * th) // 100 - 7 * k)))
    return out


def map_inset_array(insets):
    """(array of icelk_map_inset_t, its length) of a picture's insets"""
    insets = list(insets)
    if len(insets) > _lib.MAP_INSETS_MAX:
        raise ValueError("more than 8 insets")
    a = (_lib.MapInset * max(len(insets), 1))()
    for t, q in zip(a, insets):
        t.x0, t.y0 = (int(v) for v in q["at"])
        t.index = int(q["index"])
        if q.get("label") is not None:
            px, py, s = q["label"]
            t.label_px, t.label_py, t.label = int(px), int(py), _text_bytes(s)
    return a, len(insets)


def _text_bytes(s):
    if isinstance(s, str):
        try:
            s = s.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("text has characters outside %r" % MAP_CHARACTERS)
    s = bytes(s)
    if b"\0" in s or len(s) > 55:
        raise ValueError("a text of more than 48 characters, or with characters outside %r" % MAP_CHARACTERS)
    return s


def map_descriptor(picture):
    """(icelk_map_desc_t, the arrays it points into) of a picture dict.  What the library would refuse is left to it, apart
    from what the struct cannot carry."""
    d, keep = _lib.MapDesc(), []

    def arr(a, dtype, cols):
        a = np.ascontiguousarray(a, dtype=dtype)
        a = a.reshape(-1, cols) if cols else a.ravel()
        keep.append(a)
        return a

    panels, texts = list(picture["panels"]), list(picture.get("texts", ()))
    if len(panels) > 2 or len(texts) > MAP_TEXTS_MAX:
        raise ValueError("more than 2 panels or more than 16 texts")
    d.width, d.height, d.quality = int(picture["width"]), int(picture["height"]), int(picture.get("quality", MAP_QUALITY))
    d.n_panels, d.n_texts = len(panels), len(texts)
    table = arr(picture["table"], np.uint8, 3)
    if table.shape != (256, 3):
        raise ValueError("the colour table must be (256, 3) uint8")
    d.table = table.ctypes.data
    for p, q in zip(d.panel, panels):
        p.x0, p.y0, p.w, p.h = (int(v) for v in q["view"])
        p.bar_x0, p.bar_w = (int(v) for v in q.get("bar", (0, 0)))
        p.xmin, p.xmax, p.ymin, p.ymax = (float(v) for v in q["limits"])
        cells, measured = arr(q.get("cells", ()), np.float64, 3), arr(q.get("measured", ()), np.uint8, 0)
        if len(cells) != len(measured):
            raise ValueError("cells and measured differ in length")
        outline, cams = arr(q.get("outline", ()), np.float64, 2), arr(q.get("cameras", ()), np.float64, 2)
        p.cells, p.measured, p.n_cells = cells.ctypes.data, measured.ctypes.data, len(cells)
        p.outline, p.n_outline = outline.ctypes.data, len(outline)
        p.cameras, p.n_cameras = cams.ctypes.data, len(cams)
        p.resident, p.group = int(bool(q.get("resident", False))), int(q.get("group", -1))
        if not p.resident:
            arrows = arr(q.get("arrows", ()), np.float64, 5)
            p.arrows, p.n_arrows = arrows.ctypes.data, len(arrows)
        pivot = q.get("pivot", "tail")
        p.pivot = {"tail": 0, "mid": 1, "middle": 1}.get(pivot, pivot)
        p.width, p.alpha, p.vmax = float(q.get("width", 4.0)), float(q.get("alpha", 1.0)), float(q.get("vmax", 0.5))
    for t, (px, py, s) in zip(d.text, texts):
        t.px, t.py, t.text = int(px), int(py), _text_bytes(s)
    return d, keep


def _resident_args(resident, group):
    if resident is None:
        return None, None, None, 0
    a = np.ascontiguousarray(resident, dtype=np.float64).reshape(-1, 5)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32).ravel()
    if g is not None and len(g) != len(a):
        raise ValueError("one group per arrow")
    return a, g, (a, g), len(a)


def map_glyph(ch):
    """The 7 rows of the glyph of a map text's character as strings of '#' and '.' (icelk_map_glyph)."""
    rows = (C.c_uint8 * 7)()
    _lib.check(_lib.load().icelk_map_glyph(ord(ch), rows))
    return ["".join("#" if (r >> (4 - k)) & 1 else "." for k in range(5)) for r in rows]


def map_overlay_host(picture, resident=None, group=None):
    """The picture's R G B (height, width, 3) uint8 by the host statement of the rasteriser (icelk_map_overlay_host): what
    `Context.map_draw(picture, want_rgb=True)` returns, byte for byte.  `resident`, `group`: what `Context.map_arrows_set`
    was given, for panels that draw the resident arrows.  picture["insets"]: each with pixels= the thumbnail its index
    stands for (icelk_map_overlay_insets_host); an index given pixels twice keeps the last.  No GPU is needed."""
    d, keep = map_descriptor(picture)
    a, g, _, n = _resident_args(resident, group)
    rgb = np.empty((max(d.height, 1), max(d.width, 1), 3), np.uint8)
    args = (C.byref(d), None if a is None else a.ctypes.data_as(_lib.f64p), None if g is None else g.ctypes.data_as(_lib.i32p), n)
    if picture.get("insets"):
        insets, n_insets = map_inset_array(picture["insets"])
        have = (_lib.MapInsetPixels * _lib.MAP_INSETS_MAX)()
        for q in picture["insets"]:
            if q.get("pixels") is not None and 0 <= int(q["index"]) < _lib.MAP_INSETS_MAX:
                px = np.ascontiguousarray(q["pixels"], dtype=np.uint8)
                if px.ndim != 3 or px.shape[2] != 3:
                    raise ValueError("an inset's pixels must be (h, w, 3) uint8")
                keep.append(px)
                t = have[int(q["index"])]
                t.rgb, t.w, t.h, t.stride = px.ctypes.data, px.shape[1], px.shape[0], px.strides[0]
        rc = _lib.load().icelk_map_overlay_insets_host(*args, insets, n_insets, have, rgb.ctypes.data_as(_lib.u8p), rgb.strides[0])
    else:
        rc = _lib.load().icelk_map_overlay_host(*args, rgb.ctypes.data_as(_lib.u8p), rgb.strides[0])
    if rc == _lib.EARG:
        raise ValueError("icelk_map_overlay_host: a bad argument (include/icelk.h lists what a picture may hold)")
    if rc == _lib.ESTATE:
        raise _lib.IcelkError("icelk_map_overlay_host: a panel draws the resident arrows, or an inset a thumbnail, and none were given")
    _lib.check(rc)
    return rgb

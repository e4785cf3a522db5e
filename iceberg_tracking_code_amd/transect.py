"""Velocities binned into the boxes of a transect or around a mooring -- the box geometry of imports/tracking_misc.py:76-185
(`azimuth_transect`, `locate_points_along_transect`, `create_squares_rot`, `create_squares_along_transect`,
`create_squares_around_mooring`, with the reference's names, argument orders and return shapes) and the loop a user of the
reference runs over them: matplotlib.path.Path(poly).contains_points over all points, per box and per time window, then
np.sum(u_sel) / n, np.hypot.  The geometry of a few dozen boxes stays on the host; every point-in-box test, the sums in
numpy's order, the speeds and, asked for, the statistics of gridding.STATS_KEYS run on the device (`icelk_boxes_bin`,
`icelk_boxes_bin_windows`; k_boxes_assign / k_boxes_day_assign in csrc/k_grid.hip, then the gridder's sort and reduce).
The boxes meet along edges that are no grid lines: a point lies in none, one or two of them, where contains_points says so.
No CPU fallback.  DESIGN.md 7.3a.

A rotation is written out as products and sums in a fixed order, vertex offset = (a c + b (-s), a s + b c) for the half
extents (a, b): np.dot, which the reference uses, goes through BLAS, whose rounding differs from machine to machine.

`frame="transect"` turns every velocity into the boxes' frame before it is added: u is then the component along the
azimuth (along the transect), v the one across it, to the left of the azimuth.
"""
import ctypes as C
import datetime as dt
import os

import numpy as np

from . import _lib
from .context import Context
from .day_grid import epoch_seconds, load_day, plan_day
from .gridding import STATS_KEYS, _STATS_OF_KEY, CellStats, hypot_of_medians

FRAMES = ("map", "transect")


def azimuth_transect(p1, p2):
    """Direction from p1 to p2 in radians, counter-clockwise from east (tracking_misc.py:76-83)."""
    return np.arctan2(p2[1] - p1[1], p2[0] - p1[0])


def locate_points_along_transect(p1, p2, dist):
    """[pointlist, distancelist]: points every `dist` from p1 towards p2, np.ceil((length + 0.3 * dist) / dist) of them
    (tracking_misc.py:85-107)."""
    u, v = p2[0] - p1[0], p2[1] - p1[1]
    profile_len = np.hypot(u, v)
    azimuth = np.arctan2(v, u)
    u_scaled, v_scaled = np.cos(azimuth) * dist, np.sin(azimuth) * dist
    pointlist, distancelist = [], []
    for c in np.arange(0, np.ceil((profile_len + 0.3 * dist) / dist)):
        pointlist.append([p1[0] + c * u_scaled, p1[1] + c * v_scaled])
        distancelist.append(c * dist)
    return [pointlist, distancelist]


def create_squares_rot(center, height, width, rotation):
    """The four corners of a box of `height` along the direction `rotation` (radians) and `width` across it, around
    `center`, as tuples in the reference's order (tracking_misc.py:109-131).  Products and sums in a fixed order, no BLAS."""
    x, y = center[0], center[1]
    c, s = np.cos(rotation), np.sin(rotation)
    ms = -s
    poly = []
    for a, b in ((0.5 * height, 0.5 * width), (0.5 * height, -0.5 * width), (-0.5 * height, -0.5 * width),
                 (-0.5 * height, 0.5 * width)):
        poly.append((x + (a * c + b * ms), y + (a * s + b * c)))
    return poly


def create_squares_along_transect(profile, pointspacing, width):
    """[polylist, points, distances]: boxes of `pointspacing` along and `width` across the line from the first to the last
    point of `profile` ('x' and 'y' arrays), one around every point of `locate_points_along_transect`
    (tracking_misc.py:133-149)."""
    p1 = np.array((profile["x"][0], profile["y"][0]))
    p2 = np.array((profile["x"][-1], profile["y"][-1]))
    points, distances = locate_points_along_transect(p1, p2, pointspacing)
    azimuth = azimuth_transect(p1, p2)
    polylist = [create_squares_rot([point[0], point[1]], pointspacing, width, azimuth) for point in points]
    return [polylist, points, distances]


def create_squares_around_mooring(coord_mooring, azimuth=-45, width=100, nr=7):
    """[polygons, centerpoints, distancelist]: a lattice of square boxes of `width`, turned by `azimuth` degrees, with
    np.floor(nr / 2.0) boxes on each side of the mooring in both directions -- nr = 4 gives 5 x 5
    (tracking_misc.py:151-185)."""
    polygons, centerpoints, distancelist = [], [], []
    nr_side = np.floor(nr / 2.0)
    distances1 = np.arange(-1 * nr_side * width, nr_side * width + 1, width)
    distances2 = np.arange(-1 * nr_side * width, nr_side * width + 1, width)
    azimuth = np.radians(azimuth)
    for dist1 in distances1:
        for dist2 in distances2:
            u1, v1 = np.cos(azimuth) * dist1, np.sin(azimuth) * dist1
            u2, v2 = np.cos(azimuth + np.radians(90)) * dist2, np.sin(azimuth + np.radians(90)) * dist2
            point = [coord_mooring[0] + u1 + u2, coord_mooring[1] + v1 + v2]
            centerpoints.append(point)
            polygons.append(create_squares_rot([point[0], point[1]], width, width, azimuth))
            distancelist.append([dist1, dist2])
    return [polygons, centerpoints, distancelist]


class BoxSet:
    """A list of boxes to bin into: `polygons` (each a sequence of three or more (x, y)), their `centers`, `distances`
    (along the transect, or the (d1, d2) pairs of a mooring lattice), the `azimuth` of their frame in radians and a
    `name` for file names."""

    def __init__(self, polygons, centers=None, distances=None, azimuth=0.0, name="boxes"):
        self.polygons = [np.asarray(p, np.float64).reshape(-1, 2) for p in polygons]
        self.centers = np.asarray(centers if centers is not None else [p.mean(0) for p in self.polygons], np.float64)
        self.distances = np.asarray(distances if distances is not None else np.arange(len(self.polygons)), np.float64)
        self.azimuth, self.name = float(azimuth), str(name)

    def __len__(self):
        return len(self.polygons)

    @classmethod
    def along_transect(cls, profile, pointspacing, width, name="transect"):
        polys, points, distances = create_squares_along_transect(profile, pointspacing, width)
        return cls(polys, points, distances, azimuth_transect((profile["x"][0], profile["y"][0]),
                                                              (profile["x"][-1], profile["y"][-1])), name)

    @classmethod
    def around_mooring(cls, coord_mooring, azimuth=-45, width=100, nr=7, name="mooring"):
        polys, centers, distances = create_squares_around_mooring(coord_mooring, azimuth, width, nr)
        return cls(polys, centers, distances, np.radians(azimuth), name)

    def packed(self):
        """(xy, offset): the vertex array and the offsets icelk_boxes_t takes"""
        offset = np.zeros(len(self.polygons) + 1, np.int32)
        offset[1:] = np.cumsum([len(p) for p in self.polygons])
        xy = np.ascontiguousarray(np.concatenate(self.polygons) if self.polygons else np.zeros((0, 2)), np.float64)
        return xy, offset

    def polygon_array(self):
        """(boxes, vertices, 2) when every box has as many vertices as the others, else the (vertices in all, 2) array"""
        if len({len(p) for p in self.polygons}) == 1:
            return np.stack(self.polygons)
        return self.packed()[0]


def _as_boxes(boxes):
    if isinstance(boxes, BoxSet):
        return boxes
    if isinstance(boxes, dict):
        return BoxSet(boxes["polygons"], boxes.get("centers"), boxes.get("distances"), boxes.get("azimuth", 0.0),
                      boxes.get("name", "boxes"))
    return BoxSet(boxes)


class _BoxArgs:
    """the icelk_boxes_t of a BoxSet and the rotation of a frame, with the arrays they point into kept alive"""

    def __init__(self, boxes, frame):
        if frame not in FRAMES:
            raise ValueError("frame is 'map' or 'transect'")
        self.xy, self.offset = boxes.packed()
        self.struct = _lib.Boxes(self.xy.ctypes.data_as(_lib.f64p), self.offset.ctypes.data_as(_lib.i32p), len(boxes))
        self.rot = np.array([np.cos(boxes.azimuth), np.sin(boxes.azimuth)], np.float64) if frame == "transect" else None

    def rot_p(self):
        return None if self.rot is None else self.rot.ctypes.data_as(_lib.f64p)


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def _i32(a):
    return a.ctypes.data_as(_lib.i32p)


def _i64(a):
    return a.ctypes.data_as(_lib.i64p)


def _pack(cnt, mu, mv, sp, observation_threshold, stats=None):
    """per-box (or windows x boxes) arrays -> the dict bin_boxes returns: NaN where count <= observation_threshold"""
    measured = cnt > observation_threshold
    out = dict(count=cnt.astype(np.int64))
    for key, a in (("u", mu), ("v", mv), ("speed", sp)):
        out[key] = np.where(measured, a, np.nan)
    if stats is not None:
        for key in STATS_KEYS:
            a = hypot_of_medians(stats["median_u"], stats["median_v"]) if key == "speed_median" else stats[_STATS_OF_KEY[key]]
            out[key] = np.where(measured, a.reshape(cnt.shape), np.nan)
    return out


def bin_boxes(ctx, x, y, u, v, boxes, observation_threshold, frame="map", stats=False):
    """One set of velocities binned into `boxes` (a BoxSet, a dict with 'polygons' and, for the transect frame, 'azimuth',
    or a list of polygons): per box what Path(poly).contains_points selects, count, and np.sum(u_sel) / count, likewise v,
    np.hypot of the two -- NaN where count <= observation_threshold.  Returns a dict of per-box arrays count, u, v, speed;
    with `stats` also gridding.STATS_KEYS.  frame="transect": u is the component along boxes.azimuth, v the one across,
    u c + v s and v c - u s with c, s = np.cos(azimuth), np.sin(azimuth), every operation rounded once."""
    boxes = _as_boxes(boxes)
    b = _BoxArgs(boxes, frame)
    a = [np.ascontiguousarray(q, dtype=np.float64).ravel() for q in (x, y, u, v)]
    n, nb = len(a[0]), len(boxes)
    cnt = np.zeros(nb, np.int32)
    mu, mv, sp = (np.zeros(nb, np.float64) for _ in range(3))
    cs = CellStats(nb) if stats else None
    ctx._ck(ctx._lib.icelk_boxes_bin(ctx._h, _f64(a[0]), _f64(a[1]), _f64(a[2]), _f64(a[3]), n, C.byref(b.struct), b.rot_p(),
                                     _i32(cnt), _f64(mu), _f64(mv), _f64(sp), C.byref(cs.struct) if stats else None))
    return _pack(cnt, mu, mv, sp, observation_threshold, cs.arrays if stats else None)


def boxes_name(day, boxes, time_window):
    """'<%Y%m%d>_<name>_<minutes>min_boxes.npz'"""
    return "{}_{}_{}min_boxes.npz".format(day.strftime("%Y%m%d"), boxes.name, int(time_window * 60.0))


def _transect_day(ctx, plan, boxes, observation_threshold, frame, stats, timing=None):
    """The plan's files through one device pass (`icelk_boxes_bin_windows`) -> the arrays of the day's file, or None when
    the files hold no point."""
    day = load_day(plan)
    if day is None:
        return None
    b = _BoxArgs(boxes, frame)
    ncam, nw = day["lo"].shape
    nb = len(boxes)
    cnt = np.zeros(nw * nb, np.int32)
    mu, mv, sp = (np.zeros(nw * nb, np.float64) for _ in range(3))
    sel = np.zeros(nw * ncam, np.int32)
    tmin, tmax = np.zeros(nw * ncam, np.float64), np.zeros(nw * ncam, np.float64)
    tables = _lib.DayTables(_i64(day["off"]), _i32(day["fcam"]), _i32(day["wf0"]), _i32(day["wf1"]), len(day["fcam"]),
                            _i64(day["lo"]), _i64(day["hi"]), ncam, nw)
    cs = CellStats(nw * nb) if stats else None
    device_ms = C.c_double(0.0)
    ctx._ck(ctx._lib.icelk_boxes_bin_windows(ctx._h, _f64(day["x"]), _f64(day["y"]), _f64(day["u"]), _f64(day["v"]), _f64(day["t"]),
                                             len(day["x"]), C.byref(tables), C.byref(b.struct), b.rot_p(), _i32(cnt), _f64(mu),
                                             _f64(mv), _f64(sp), C.byref(cs.struct) if stats else None, _i32(sel), _f64(tmin),
                                             _f64(tmax), C.byref(device_ms) if timing is not None else None))
    if timing is not None:
        timing.update(points=len(day["x"]), kernels_ms=device_ms.value)
    keep = np.flatnonzero(sel.reshape(nw, ncam).any(1))                       # a window counts iff some camera selected a point
    shape = (nw, nb)
    out = _pack(cnt.reshape(shape), mu.reshape(shape), mv.reshape(shape), sp.reshape(shape), observation_threshold,
                cs.arrays if stats else None)
    arrays = dict(polygons=boxes.polygon_array(), centers=boxes.centers, distance=boxes.distances,
                  azimuth=np.float64(boxes.azimuth), frame=np.asarray(frame),
                  window_start=np.array([epoch_seconds(plan.windows[w][0]) for w in keep], np.int64),
                  window_end=np.array([epoch_seconds(plan.windows[w][1]) for w in keep], np.int64))
    if arrays["polygons"].ndim == 2:
        arrays["polygon_offset"] = boxes.packed()[1]
    arrays.update({k: a[keep] for k, a in out.items()})
    return arrays


def utm_to_transect(camnames, source_path_head, source_path_tail, target_path, schedule, clock_drifts, day, time_window,
                    boxes, observation_threshold, ctx=None, save=True, frame="map", stats=False):
    """One day of hourly velocity files binned into `boxes`, every time window in one device pass: the day driver of
    day_grid.utm_to_gridded_utm (schedule, windows, clock drift, selection from the hourly files -- `plan_day`) with the
    boxes of a transect or a mooring in place of the fjord grid.

    Returns (file name, dict of arrays), or None when the day has no files or no points; with `save` the arrays are
    written to target_path/'<%Y%m%d>_<name>_<minutes>min_boxes.npz'.  Keys: polygons, centers, distance, azimuth
    (radians), frame; window_start, window_end (epoch seconds of the windows in which some camera selected a point, one
    row of the following per such window); count (windows x boxes), u, v, speed (NaN where count <=
    observation_threshold), and with `stats` gridding.STATS_KEYS.  Boxes that do not all have the same number of vertices
    are stored as one (vertices, 2) array with `polygon_offset` beside it."""
    boxes = _as_boxes(boxes)
    if frame not in FRAMES:
        raise ValueError("frame is 'map' or 'transect'")
    plan = plan_day(camnames, source_path_head, source_path_tail, schedule, clock_drifts, day, time_window, 0)
    if not plan.files:
        return None
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    try:
        arrays = _transect_day(ctx, plan, boxes, observation_threshold, frame, stats)
    finally:
        if own:
            ctx.close()
    if arrays is None:
        return None
    name = boxes_name(day, boxes, time_window)
    if save:
        np.savez(os.path.join(target_path, name), **arrays)
    return name, arrays


def utm_to_transect_days(days, camnames, source_path_head, source_path_tail, target_path, schedule, clock_drifts,
                         time_window, boxes, observation_threshold, ctx=None, save=True, frame="map", stats=False):
    """`utm_to_transect` over a list of days on one context: [(file name, dict of arrays)] of the days that have points."""
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    try:
        out = []
        for day in days:
            r = utm_to_transect(camnames, source_path_head, source_path_tail, target_path, schedule, clock_drifts, day,
                                time_window, boxes, observation_threshold, ctx=ctx, save=save, frame=frame, stats=stats)
            if r is not None:
                out.append(r)
        return out
    finally:
        if own:
            ctx.close()

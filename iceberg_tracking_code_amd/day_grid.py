"""The day driver of step s3: `utm_to_gridded_utm` of s3_utm_to_gridded_utm.py:222-446 (plot_switch 0) -- camera
schedule, time windows, clock drift, selection of each window's velocities out of every camera's hourly files, one
gridded `.npz` per window -- with every window of the day binned in one device pass (`icelk_grid_bin_windows`,
csrc/k_grid.hip).  The host plans a few dozen windows with plain `datetime`; the points cross PCIe once.

What the reference does, and this module reproduces:
- schedule: a camera counts only if exactly one row has camera == name and start_day <= day <= end_day; its hours
  run from start_time ('%H:%M') to start + tracking_duration;
- windows: np.arange(min start, max end + 0.001, time_window), starts [:-1], ends [1:]; time_window == 24.0 is the one
  window [min start, max end]; datetimes are day + timedelta(hours=float), microseconds included;
- drift (trm.correct_time_drift): the first row with cam == name, start_date < day <= end_date; numpy's
  round(drift_start_sec + days * drift_pday_sec, 1) (the workbook's columns are numpy scalars); anything that fails
  means 0.  Windows shift by -drift; epoch bounds are int(total_seconds) of the shifted datetimes (truncation);
- selection: time >= start & time < end per hour file, float64;
- hour files: the hours start.replace(minute=0, second=0) + k h up to end.replace(minute=0, second=0) (the hours
  pandas.date_range(..., freq='H') lists, microseconds kept: when the end's microseconds are below the start's, the
  end's hour drops out); each hour's file is the first of '%Y%m%d_%H00*.npz' in the camera workspace -- the reference
  takes glob's first, in directory order; here the sorted first.  A file that cannot be read, or lacks one of x, y,
  u, v, speed, time, counts as missing, as the reference's `except: pass` has it.  A camera without a
  day_str + '*utm.npz' file is skipped.  A point in a file its window does not load belongs to no window;
- a window gets a file iff some camera selected a point in it; the points of a window are concatenated camera by
  camera, hour by hour -- the order of numpy's pairwise per-cell sums;
- names: '%Y%m%d_%H%M-%H%M_{time_diff}min_{grid_size}m.npz' with time_diff = int(minutes); the full day is named from
  the first / last selected time (+ drift) rounded to 30 minutes (trm.round_time).
Times are taken as float64: s2 writes int64 epoch seconds, which float64 holds exactly.
With `plots=directory` every window that writes an `.npz` also writes its map (plot_switch 1 and 2, s3:449-465), drawn on
the device as a JPEG file (velocity_map.py) or, with plot_format="png", as the PNG file the reference
writes, with its name and exactly the rasterised pixels; with plot_switch 2 the day's selected vectors are uploaded once
and each window's picture draws its group of them.  With `photos=directory` as well, the picture carries the cameras'
photographs from the middle of the window (s3:593-626, s3:788-829): `closest_image` picks the file, the device decodes it
and reduces it to a thumbnail that is pasted into the map with the camera's name.
With `movie=` as well, every map drawn also becomes a frame of the movie the reference makes of them (s3:194-215), scaled
and coded on the device from the pixels the map left there: a Motion-JPEG AVI, 8 frames per second, 2000 pixels wide
(movie.py); `utm_to_gridded_utm_days` writes one movie over all its days, as s3's main does.
Not built: the reference's movie codec (msmpeg4v2), PNG files with dynamic Huffman codes (the PNG is one fixed-Huffman block), the xlsx readers (pass the rows pd.read_excel gives),
s3:main's process pool.
"""
import ctypes as C
import datetime as dt
import glob
import os
import time

import numpy as np

from . import _lib
from .context import Context
from .gridding import STATS_KEYS, CellStats, cell_table, create_grid_across_fjord, pack_cells
from .jpeg import UnsupportedJpeg, describe_jpeg
from .movie import open_movie, velocities_movie_name
from .validate import lattice_struct, params_struct, validate_options, validation_array, validation_lattice
from .velocity_map import MAP_QUALITY, MAP_WIDTH, map_insets, map_layout, map_name, map_picture, map_strings, map_text, map_view

EPOCH = dt.datetime(1970, 1, 1)
HOUR_KEYS = ("x", "y", "u", "v", "speed", "time")
SAVED_KEYS = ("grid_size", "topleft", "rows", "cols", "grid_id", "i", "j", "x", "y", "u", "v", "speed", "count",
              "measured", "not_measured")


def _records(table):
    """A workbook table as a list of row dicts: a list of dicts, or anything with .to_dict('records')."""
    return table.to_dict("records") if hasattr(table, "to_dict") else list(table)


def epoch_seconds(t):
    """trm.datetime_to_epoch: whole seconds since 1970, truncated toward zero."""
    return int((t - EPOCH).total_seconds())


def round_half_hour(t):
    """trm.round_time(t, 1800): to the nearest half hour of the day (a tie goes up), microseconds dropped."""
    s = t.hour * 3600 + t.minute * 60 + t.second
    r = (s + 900.0) // 1800 * 1800
    return t.replace(microsecond=0) + dt.timedelta(seconds=r - s)


def scheduled_cameras(camnames, schedule, day):
    """s3:239-262 -> [(name, start hour, end hour)] in camnames order."""
    d = int(day.strftime("%Y%m%d"))
    rows = _records(schedule)
    out = []
    for name in camnames:
        match = [r for r in rows if r["camera"] == name and r["start_day"] <= d and r["end_day"] >= d]
        if len(match) == 1:
            t = dt.datetime.strptime(match[0]["start_time"], "%H:%M")
            start = t.hour + t.minute / 60.0
            out.append((name, start, start + match[0]["tracking_duration"]))
    return out


def time_correction(camname, day, clock_drifts):
    """trm.correct_time_drift for one camera and day, in seconds; 0 when no row applies or anything fails."""
    d = int(day.strftime("%Y%m%d"))
    try:
        row = [r for r in _records(clock_drifts) if r["cam"] == camname and r["start_date"] < d
               and r["end_date"] >= d][0]
        days = (dt.datetime.strptime(str(d), "%Y%m%d") - dt.datetime.strptime(str(row["start_date"]), "%Y%m%d")).days
        return float(np.round(np.float64(row["drift_start_sec"]) + days * np.float64(row["drift_pday_sec"]), 1))
    except Exception:
        return 0


def time_windows(starts, ends, time_window):
    """s3:268-274 -> [(start hour, end hour)]."""
    edges = list(np.arange(min(starts), max(ends) + 0.001, time_window))
    if time_window == 24.0:
        return [(min(starts), max(ends))]
    return list(zip(edges[:-1], edges[1:]))


def hours_between(start, end):
    """The hours return_velocities_by_time loads for [start, end): start and end with minutes and seconds zeroed
    (microseconds kept), then start + k hours while <= end."""
    h, last = start.replace(minute=0, second=0), end.replace(minute=0, second=0)
    out = []
    while h <= last:
        out.append(h)
        h += dt.timedelta(hours=1)
    return out


class DayPlan:
    """Everything about a day that does not need the velocities.

    windows[w] = (start, end) datetimes; cameras[c] = dict(name, correction, workspace, has_files, lo, hi, hours, f0,
    f1): lo / hi the int64 epoch bounds of each window, hours[w] the hour datetimes window w loads, f0[w] .. f1[w] the
    files it loads (none: f0 > f1); files = the hour files in concatenation order (camera, then hour), dict(cam, hour
    ('%Y%m%d_%H00'), path)."""

    def __init__(self, day, time_window, grid_size, windows, cameras, files):
        self.day, self.time_window, self.grid_size = day, time_window, grid_size
        self.windows, self.cameras, self.files = windows, cameras, files

    def name(self, w, t_min=None, t_max=None):
        """File name of window w (s3:427-437).  The full day (time_window 24.0) needs t_min / t_max: per camera
        the smallest / largest selected epoch time, None for a camera that selected nothing."""
        start, end = self.windows[w]
        if self.time_window == 24.0:
            lo = [EPOCH + dt.timedelta(seconds=t) + dt.timedelta(seconds=cam["correction"])
                  for t, cam in zip(t_min, self.cameras) if t is not None]
            hi = [EPOCH + dt.timedelta(seconds=t) + dt.timedelta(seconds=cam["correction"])
                  for t, cam in zip(t_max, self.cameras) if t is not None]
            return "{}-{}_full_day_{}m.npz".format(round_half_hour(min(lo)).strftime("%Y%m%d_%H%M"),
                                                   round_half_hour(max(hi)).strftime("%H%M"), self.grid_size)
        time_diff = int((end - start).total_seconds() / 60.0)
        return "{}-{}_{}min_{}m.npz".format(start.strftime("%Y%m%d_%H%M"), end.strftime("%H%M"), time_diff,
                                            self.grid_size)


def plan_day(camnames, source_path_head, source_path_tail, schedule, clock_drifts, day, time_window, grid_size):
    """The bookkeeping of s3:228-322 for one day, from the schedule, the drift table and the file names alone."""
    day_str = day.strftime("%Y%m%d")
    cams = scheduled_cameras(camnames, schedule, day)
    if not cams:
        return DayPlan(day, time_window, grid_size, [], [], [])
    windows = [(day + dt.timedelta(hours=a), day + dt.timedelta(hours=b))
               for a, b in time_windows([c[1] for c in cams], [c[2] for c in cams], time_window)]
    cameras, files = [], []
    for ci, (name, _, _) in enumerate(cams):
        corr = time_correction(name, day, clock_drifts)
        ws = os.path.join(source_path_head, name, source_path_tail)
        shift = dt.timedelta(seconds=corr)
        bounds = [(s - shift, e - shift) for s, e in windows]
        cam = dict(name=name, correction=corr, workspace=ws,
                   has_files=len(glob.glob(os.path.join(ws, day_str + "*utm.npz"))) > 0,
                   lo=[epoch_seconds(s) for s, _ in bounds], hi=[epoch_seconds(e) for _, e in bounds],
                   hours=[hours_between(s, e) for s, e in bounds], f0=[], f1=[])
        cameras.append(cam)
        if not cam["has_files"]:
            cam["f0"], cam["f1"] = [0] * len(windows), [-1] * len(windows)
            continue
        # a window loads consecutive hours, so a contiguous run of the camera's files; the windows loading one file
        # need not be consecutive (a window inside one hour whose end microseconds lie below its start's loads none)
        prefixes = sorted({h.strftime("%Y%m%d_%H00") for hours in cam["hours"] for h in hours})
        index = {}
        for prefix in prefixes:
            match = sorted(glob.glob(os.path.join(ws, prefix + "*.npz")))
            if match:
                index[prefix] = len(files)
                files.append(dict(cam=ci, hour=prefix, path=match[0]))
        for hours in cam["hours"]:
            got = [index[p] for p in (h.strftime("%Y%m%d_%H00") for h in hours) if p in index]
            assert got == list(range(got[0], got[-1] + 1)) if got else True
            cam["f0"].append(got[0] if got else 0)
            cam["f1"].append(got[-1] if got else -1)
    return DayPlan(day, time_window, grid_size, windows, cameras, files)


def _load_hour_file(path, with_speed=False):
    """x, y, u, v, t (and, asked for, speed) of an hourly velocity file as float64, or None where the reference's
    `except: pass` would skip the file."""
    try:
        with np.load(path) as z:
            a = [np.asarray(z[k]) for k in HOUR_KEYS]
    except Exception:
        return None
    x, y, u, v, speed, t = (np.ascontiguousarray(q, dtype=np.float64).ravel() for q in a)
    if not len(x) == len(y) == len(u) == len(v) == len(t):
        return None
    if with_speed:
        return (x, y, u, v, t, speed) if len(speed) == len(x) else None
    return x, y, u, v, t


def load_day(plan, with_speed=False):
    """The plan's hour files as the device passes take them (`icelk_grid_bin_windows`, `icelk_boxes_bin_windows`): x, y, u,
    v, t concatenated camera by camera, hour by hour; off (file f holds points off[f] .. off[f + 1]), fcam (its camera);
    lo, hi (cameras x windows, the int64 epoch bounds), wf0, wf1 (the files each window loads); parts, the files'
    own arrays (with their speed when asked for).  An unreadable file holds no point.  None when no file holds one."""
    empty = (np.zeros(0),) * (6 if with_speed else 5)
    parts = [_load_hour_file(f["path"], with_speed) or empty for f in plan.files]
    if sum(len(p[0]) for p in parts) == 0:
        return None
    out = {k: np.concatenate([p[i] for p in parts]) for i, k in enumerate(("x", "y", "u", "v", "t"))}
    out["off"] = np.zeros(len(parts) + 1, np.int64)
    out["off"][1:] = np.cumsum([len(p[0]) for p in parts])
    out["fcam"] = np.array([f["cam"] for f in plan.files], np.int32)
    out["lo"], out["hi"] = (np.array([c[k] for c in plan.cameras], np.int64) for k in ("lo", "hi"))
    out["wf0"], out["wf1"] = (np.array([c[k] for c in plan.cameras], np.int32) for k in ("f0", "f1"))
    out["parts"] = parts
    return out


def tracking_interval(workspace, day_str):
    """The camera's tracking interval in seconds, from the name of its first file of the day (s3:318,340)."""
    npzs = sorted(glob.glob(os.path.join(workspace, day_str + "*utm.npz")))
    return float(os.path.basename(npzs[0]).split("_")[2].split("s")[0])


def window_of_points(t, off, fcam, lo, hi, wf0, wf1):
    """The window of every point of the concatenated hour files, -1 for none, by the rule of the device pass
    (k_grid_day_assign): the last window of the point's camera that starts at or before its time, if the window loads the
    point's file and ends after the time."""
    group = np.full(len(t), -1, np.int32)
    for f in range(len(off) - 1):
        a, b, c = int(off[f]), int(off[f + 1]), int(fcam[f])
        if b == a:
            continue
        tp = t[a:b]
        w = np.searchsorted(lo[c].astype(np.float64), tp, side="right") - 1
        wc = np.maximum(w, 0)
        ok = (w >= 0) & (wf0[c][wc] <= f) & (f <= wf1[c][wc]) & (tp < hi[c][wc].astype(np.float64))
        group[a:b] = np.where(ok, w, -1)
    return group


def camera_positions(camnames, cameras, day):
    """[(easting, northing)] of the cameras with exactly one row for the day, in camnames order, and the position the
    'Camera(s)' label goes beside (the first name's, s3:538-559), or None."""
    d = int(day.strftime("%Y%m%d"))
    rows = _records(cameras) if cameras is not None else []
    out, label = [], None
    for name in camnames:
        match = [r for r in rows if r["camera"] == name and r["start_day"] <= d and r["end_day"] >= d and "easting" in r and "northing" in r]
        if len(match) == 1:
            out.append((float(match[0]["easting"]), float(match[0]["northing"])))
            if name == camnames[0]:
                label = out[-1]
    return out, label


def closest_image(workspace, target_time, max_timediff=300):
    """trm.return_closest_image (imports/tracking_misc.py:295-315): the photo of `workspace` nearest in time to
    `target_time` (UTC), or None.  The folder is (target_time - 8 h).strftime('%Y%m%d') -- the cameras' folders are named in
    Alaska time --, the files are '%Y%m%d-%H%M%S.jpg', and the nearest one counts only if it is less than `max_timediff`
    seconds away, strictly.  Where the reference raises or leaves it to chance: a missing or empty folder gives None, names
    that do not parse are skipped, a tie goes to the earlier photo."""
    folder = os.path.join(str(workspace), (target_time - dt.timedelta(hours=8)).strftime("%Y%m%d"))
    times = []
    for path in sorted(glob.glob(os.path.join(folder, "*.jpg"))):
        try:
            times.append((dt.datetime.strptime(os.path.basename(path), "%Y%m%d-%H%M%S.jpg"), path))
        except ValueError:
            continue
    if not times:
        return None
    when, path = min(sorted(times), key=lambda tp: abs(tp[0] - target_time))
    return path if abs((target_time - when).total_seconds()) < max_timediff else None


def photo_time(plan, w, plot_switch, min_time=None, max_time=None):
    """The time whose photographs a window's picture shows.  One map (s3:600-603): the last scheduled camera's corrected
    window start plus half the window -- the reference's variable is left over from its loop over the cameras (s3:304-314),
    so it is that camera's whether or not it has files --, for the full day min_time + (max_time - min_time) / 2.  Two
    maps (s3:807): always the corrected start plus half the window."""
    if plot_switch != 2 and plan.time_window == 24.0:
        return min_time + (max_time - min_time) / 2
    start = plan.windows[w][0] - dt.timedelta(seconds=plan.cameras[-1]["correction"])
    return start + dt.timedelta(hours=plan.time_window / 2.0)


def _photo_size(data):
    """(width, height) of a photo's file: from its header, by Pillow for a file the device decoder does not take"""
    try:
        info = describe_jpeg(data)
        return info.width, info.height
    except UnsupportedJpeg:
        import io
        from PIL import Image
        return Image.open(io.BytesIO(data)).size


def window_insets(ctx, photos, names, when, plot_switch, fjord, out_width):
    """The insets of one window's picture: for each camera with tracks the photo of <photos>/<camera>/ closest to `when`,
    made resident on `ctx` (`Context.map_inset_set`) and placed by `velocity_map.map_insets`.  One map: the reference stacks
    every camera's photo in the one box; only the last camera that has one is drawn (inset 0).  Two maps: camera k goes to
    box k, a camera without a photo leaves its box empty."""
    paths = [closest_image(os.path.join(photos, name), when) for name in names]
    if plot_switch == 2 and len(names) > 4:
        raise ValueError("the two-map figure has room for four cameras' photographs")
    if plot_switch != 2:
        last = [k for k, p in enumerate(paths) if p is not None][-1:]
        names, paths = [names[k] for k in last], [paths[k] for k in last]
    files = []
    for path in paths:
        if path is None:
            files.append(None)
            continue
        with open(path, "rb") as f:
            files.append(f.read())
    layout = map_layout(map_view(fjord, plot_switch), out_width, 2 if plot_switch == 2 else 1)
    places = map_insets(layout, plot_switch, [None if d is None else _photo_size(d) for d in files])
    out = []
    for k, (name, data, place) in enumerate(zip(names, files, places)):
        if place is None:
            continue
        size = ctx.map_inset_set(k, data, place["box"])
        assert tuple(size) == tuple(place["size"])
        out.append(dict(index=k, at=place["at"], label=(place["label_at"][0], place["label_at"][1], map_text(name))))
    return out


def _grid_day(ctx, plan, fjord, grid_size, observation_threshold, timing=None, maps=None, stats=False, validate=None):
    """Loads the plan's files, runs the device pass, and packs every window that selected a point.  `timing`: a dict
    that receives the seconds of each stage and the kernels' milliseconds (tools/grid_day_bench.py).  `maps`: None, or
    what the windows' pictures need (utm_to_gridded_utm's plot keywords); the written list then carries each picture's
    name and bytes as a third and fourth entry.  `stats`: every window's arrays also carry gridding.STATS_KEYS, from
    `icelk_grid_bin_windows_stats`; without it that entry point is not called.  `validate`: None, or what
    validate.validate_options returns: the pass is `icelk_grid_bin_windows_validated`, every window's arrays also carry
    `rejected` and `validation`, and `timing` receives the per-point `status`."""
    clock = time.perf_counter
    t0 = clock()
    vectors = maps is not None and maps["plot_switch"] == 2
    loaded = load_day(plan, vectors)
    if loaded is None:
        return []
    x, y, u, v, t, off, fcam, lo, hi, wf0, wf1, parts = (loaded[k] for k in ("x", "y", "u", "v", "t", "off", "fcam", "lo", "hi",
                                                                             "wf0", "wf1", "parts"))
    n = len(x)
    ncam, nw = lo.shape
    grid = create_grid_across_fjord(ctx, fjord, grid_size)
    topleft, rows, cols = grid[3], grid[4], grid[5]
    left, top, on, idx = cell_table(grid, fjord)
    ncells = rows * cols
    t1 = clock()
    cnt = np.zeros(nw * ncells, np.int32)
    mu, mv, sp = (np.zeros(nw * ncells, np.float64) for _ in range(3))
    sel = np.zeros(nw * ncam, np.int32)
    tmin, tmax = np.zeros(nw * ncam, np.float64), np.zeros(nw * ncam, np.float64)
    f64 = lambda a: a.ctypes.data_as(_lib.f64p)               # noqa: E731
    i32 = lambda a: a.ctypes.data_as(_lib.i32p)               # noqa: E731
    i64 = lambda a: a.ctypes.data_as(_lib.i64p)               # noqa: E731
    device_ms = C.c_double(0.0)
    args = (ctx._h, f64(x), f64(y), f64(u), f64(v), f64(t), n, i64(off), i32(fcam), i32(wf0), i32(wf1), len(parts),
            i64(lo), i64(hi), ncam, nw, left, top, float(grid_size), cols, rows, on.ctypes.data_as(_lib.u8p), i32(cnt),
            f64(mu), f64(mv), f64(sp), i32(sel), f64(tmin), f64(tmax), C.byref(device_ms) if timing is not None else None)
    cs = CellStats(nw * ncells) if stats else None
    if validate is not None:
        lattice = lattice_struct(validation_lattice(fjord, validate["side"]))
        params = params_struct(validate["threshold"], validate["eps"], validate["min_neighbours"])
        status, rejected = np.zeros(n, np.uint8), np.zeros(nw, np.int32)
        ctx._ck(ctx._lib.icelk_grid_bin_windows_validated(*args, C.byref(cs.struct) if stats else None, C.byref(lattice), C.byref(params),
                                                          status.ctypes.data_as(_lib.u8p), i32(rejected)))
    elif stats:
        ctx._ck(ctx._lib.icelk_grid_bin_windows_stats(*args, C.byref(cs.struct)))
    else:
        ctx._ck(ctx._lib.icelk_grid_bin_windows(*args))
    t2 = clock()
    sel, tmin, tmax = sel.reshape(nw, ncam), tmin.reshape(nw, ncam), tmax.reshape(nw, ncam)
    if maps is not None:
        day_str = plan.day.strftime("%Y%m%d")
        names = [c["name"] for c in plan.cameras]
        positions, label = camera_positions(names, maps["cameras"], plan.day)
        if vectors:            # the day's vectors go to the device once; every window's picture draws its group
            speed = np.concatenate([p[5] for p in parts])
            seconds = np.zeros(n)
            for f, c in enumerate(fcam):
                if off[f + 1] > off[f]:
                    seconds[off[f]:off[f + 1]] = tracking_interval(plan.cameras[c]["workspace"], day_str)
            ctx.map_arrows_set(np.column_stack([x, y, u * seconds, v * seconds, speed]), window_of_points(t, off, fcam, lo, hi, wf0, wf1))
    written = []
    for w in range(nw):
        if not sel[w].any():
            continue
        s = slice(w * ncells, (w + 1) * ncells)
        r = pack_cells(grid, idx, cnt[s], mu[s], mv[s], sp[s], observation_threshold, stats=cs.window(s) if stats else None)
        r.update(grid_size=grid_size, topleft=topleft, rows=rows, cols=cols)
        arrays = {k: np.asanyarray(r[k]) for k in SAVED_KEYS + (STATS_KEYS if stats else ())}   # what np.savez makes of s3's lists
        if validate is not None:
            arrays.update(rejected=np.asanyarray(int(rejected[w])), validation=validation_array(validate))
        name = plan.name(w, [float(a) if k else None for a, k in zip(tmin[w], sel[w])],
                         [float(a) if k else None for a, k in zip(tmax[w], sel[w])])
        if maps is None:
            written.append((name, arrays))
            continue
        lo_t = [EPOCH + dt.timedelta(seconds=float(a)) + dt.timedelta(seconds=cam["correction"]) for a, k, cam in zip(tmin[w], sel[w], plan.cameras) if k]
        hi_t = [EPOCH + dt.timedelta(seconds=float(a)) + dt.timedelta(seconds=cam["correction"]) for a, k, cam in zip(tmax[w], sel[w], plan.cameras) if k]
        when = dict(time_window=plan.time_window, min_time=round_half_hour(min(lo_t)), max_time=round_half_hour(max(hi_t)))
        start, end = plan.windows[w]
        strings = map_strings(plan.day, start, end, [nm for nm, k in zip(names, sel[w]) if k], grid_size, **when)
        picture = map_picture(fjord, grid_size, r["measured"], r["not_measured"], r["x"], r["y"], r["u"], r["v"], r["speed"], strings,
                              cameras=positions, label=label, n_camnames=len(names), plot_switch=maps["plot_switch"], group=w,
                              speedthreshold_cbar=maps["speedthreshold_cbar"], out_width=maps["out_width"], quality=maps["quality"])
        if maps.get("photos") is not None:
            at = photo_time(plan, w, maps["plot_switch"], when["min_time"], when["max_time"])
            picture["insets"] = window_insets(ctx, maps["photos"], [nm for nm, k in zip(names, sel[w]) if k], at, maps["plot_switch"], fjord,
                                              maps["out_width"])
        as_png = maps.get("format", "jpeg") == "png"
        written.append((name, arrays, map_name(maps["dir"], start, end, ext=".png" if as_png else ".jpg", **when),
                        ctx.map_draw(picture, format="png" if as_png else "jpeg")))
        if maps.get("movie") is not None:
            maps["movie"].add_picture(ctx)
    if vectors:
        ctx.map_arrows_release()
    if maps is not None and maps.get("photos") is not None:
        ctx.map_inset_release()
    if timing is not None:
        timing.update(points=n, load_s=t1 - t0, device_call_s=t2 - t1, kernels_ms=device_ms.value,
                      pack_s=clock() - t2)
        if validate is not None:
            timing.update(status=status, rejected=rejected)
    return written


def utm_to_gridded_utm(camnames, source_path_head, source_path_tail, target_path, schedule, clock_drifts, fjord, day,
                       time_window, grid_size, observation_threshold, ctx=None, save=True, plots=None, plot_switch=1,
                       speedthreshold_cbar=0.5, cameras=None, out_width=MAP_WIDTH, quality=MAP_QUALITY, photos=None, plot_format="jpeg",
                       movie=None, stats=False, validate=None):
    """One day of hourly velocity files -> one gridded .npz per time window, as s3_utm_to_gridded_utm.utm_to_gridded_utm
    (s3:222-446) with plot_switch 0.

    `schedule`: the rows of the parameter workbook (camera, start_day, end_day, start_time, tracking_duration);
    `clock_drifts`: the rows of the clock-drift workbook (cam, start_date, end_date, drift_start_sec, drift_pday_sec)
    -- each a list of dicts or anything with .to_dict('records'), e.g. what pd.read_excel returns.  `fjord`: dict or
    npz with 'x' and 'y'.  `day`: datetime.  Returns [(file name, dict of arrays)] in writing order; with `save` the
    files are written to target_path with np.savez, keys and dtypes as the reference's.

    `plots`: a directory; every window that writes an .npz also gets its map there (s3:449-465), '%Y%m%d_%H%M-%H%M.jpg',
    drawn and coded on the device.  plot_switch 1: the gridded map; 2: the all-vectors panel beside it.
    `cameras`: the parameter workbook's rows with camera, start_day, end_day, easting, northing (None: `schedule`, whose
    rows may carry them); `speedthreshold_cbar`: the speed at the colour bar's end.  plots=None calls nothing of this.
    `plot_format`: "jpeg", or "png" for '%Y%m%d_%H%M-%H%M.png', the reference's name, a file that decodes to exactly the
    rasterised pixels (`quality` plays no part then).

    `photos`: the reference's source_path_photos, a directory with <camera>/<%Y%m%d>/<%Y%m%d-%H%M%S>.jpg; every picture then
    carries, for each camera with tracks in its window, the photograph closest to the middle of the window (less than
    300 s away, `closest_image`), reduced on the device and labelled with the camera's name.  It needs
    `plots`; photos=None calls nothing of this.

    `movie`: with `plots`, every map drawn also becomes a frame of a Motion-JPEG AVI (8 frames per second, 2000 pixels wide:
    `movie.MovieWriter`), in the order drawn, scaled and coded on the device whatever `plot_format` is.
    True: 'velocities_utm_<minutes>min.avi', the reference's name (s3:211), in `plots`; a path: that file; a `MovieWriter`:
    frames are added to it and it is left open.  The maps and the .npz files do not change.  movie=None calls nothing of this.

    `stats`: every window file also carries, over its measured cells, u_std, v_std (np.std(ddof=1) of the cell's velocities),
    u_median, v_median, speed_median (np.hypot of the two), u_mad, v_mad (the median absolute deviation) -- numpy's bits,
    selected on the device; every other key is what it is without.  The maps still draw the means.
    stats=False calls nothing of this.

    `validate`: None, True (threshold 2.0, eps 0.01 m/s, min_neighbours 8, a lattice side of 2 * grid_size -- policy, not
    measurements) or a dict of those four: the normalised median test (validate.py) runs on the device
    between the upload and the gridder, every window's points against the pools of that window, all cameras together.  A
    rejected vector is in no window: it is neither binned, counted nor part of a window's time range, so a window whose
    every vector is rejected writes no file.  Every window file carries two more keys, `rejected` (int, the window's
    count) and `validation` (threshold, eps, min_neighbours, side as float64); everything else is computed from the
    surviving points.  The all-vectors panel of plot_switch 2 keeps drawing every vector, the rejected ones too.
    validate=None calls nothing of this, and every file is what it was."""
    validate = validate_options(validate, grid_size)
    if movie is not None and plots is None:
        raise ValueError("movie needs plots: its frames are the windows' pictures")
    if plots is not None and plot_switch not in (1, 2):
        raise ValueError("plot_switch must be 1 or 2")
    if plot_format not in ("jpeg", "png"):
        raise ValueError("plot_format is 'jpeg' or 'png'")
    if photos is not None and plots is None:
        raise ValueError("photos needs plots: the photographs go into the windows' pictures")
    maps = None if plots is None else dict(dir=str(plots), plot_switch=plot_switch, speedthreshold_cbar=speedthreshold_cbar,
                                           cameras=schedule if cameras is None else cameras, out_width=out_width, quality=quality,
                                           photos=None if photos is None else str(photos), format=plot_format)
    plan = plan_day(camnames, source_path_head, source_path_tail, schedule, clock_drifts, day, time_window, grid_size)
    if not plan.files:
        return []
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    film_own = False
    if movie is not None:
        os.makedirs(maps["dir"], exist_ok=True)
        maps["movie"], film_own = open_movie(movie, maps["dir"], velocities_movie_name(time_window))
    try:
        written = _grid_day(ctx, plan, fjord, grid_size, observation_threshold, maps=maps, stats=stats, validate=validate)
    finally:
        if own:
            ctx.close()
        if film_own:
            maps["movie"].close()
    if maps is not None:
        os.makedirs(maps["dir"], exist_ok=True)
        for _, _, path, data in written:
            with open(path, "wb") as f:
                f.write(data)
        written = [(name, arrays) for name, arrays, _, _ in written]
    if save:
        for name, arrays in written:
            np.savez(os.path.join(target_path, name), **arrays)
    return written


def utm_to_gridded_utm_days(days, camnames, source_path_head, source_path_tail, target_path, schedule, clock_drifts,
                            fjord, time_window, grid_size, observation_threshold, ctx=None, save=True, plots=None,
                            plot_switch=1, speedthreshold_cbar=0.5, cameras=None, out_width=MAP_WIDTH, quality=MAP_QUALITY, photos=None,
                            plot_format="jpeg", movie=None, stats=False, validate=None):
    """s3:main's loop over days (without its process pool), on one context: the files of every day, in order.  The plot
    keywords, `stats` and `validate` are utm_to_gridded_utm's; `movie` gives ONE movie over all the days' maps, as s3's main makes one."""
    if movie is not None and plots is None:
        raise ValueError("movie needs plots: its frames are the windows' pictures")
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1 << 18)
    film, film_own = None, False
    if movie is not None:
        os.makedirs(str(plots), exist_ok=True)
        film, film_own = open_movie(movie, plots, velocities_movie_name(time_window))
    try:
        out = []
        for day in days:
            out += utm_to_gridded_utm(camnames, source_path_head, source_path_tail, target_path, schedule,
                                      clock_drifts, fjord, day, time_window, grid_size, observation_threshold,
                                      ctx=ctx, save=save, plots=plots, plot_switch=plot_switch,
                                      speedthreshold_cbar=speedthreshold_cbar, cameras=cameras, out_width=out_width,
                                      quality=quality, photos=photos, plot_format=plot_format, movie=film,
                                      stats=stats, validate=validate)
        return out
    finally:
        if own:
            ctx.close()
        if film_own:
            film.close()

"""Step s4: s4_postprocess_gridded_utm.py -- the gridded windows of a run stacked into one cube (`combine_npzs`,
s4:120-210), the daily / period mean velocity fields (`average_spatially_temporally`, `spatial_mean`, s4:264-343) and
the csv / mat exports (s4:212-256).

The cube is built on the host (one fancy-index scatter per window file; it needs no GPU).  The averages run on the
device: `VelocityCube` uploads u, v, count once, laid out [window][cell], and `average_periods` serves every period of
a request -- all days of a run, say -- with one launch chain (`icelk_cube_average`, csrc/k_cube.hip), where the
reference slices the cube and calls np.nanmean / np.nansum once per period.  Results are bit for bit numpy's (DESIGN.md
§7.4 for the order of additions found); only the sign of a NaN may differ.  No CPU fallback for the averages.

Reference quirks kept:
- x / y of the cube come from the last file read, rows / cols from the first; `i` / `j` are meshgrid(range(rows),
  range(cols), indexing='ij'), named against the raster's [j, i];
- `average_spatially_temporally` returns y, u, v flipped upside down for coarseness 1 (the reference flips them for its
  plot before it returns) and count not; for coarseness > 1 nothing is flipped; a period without data returns six
  NaN; a period that selects no window raises ValueError (the reference's .min() of an empty array);
- spatial_mean pads with zeros up to a multiple of coarseness, and the padded cells count in the mean.
One deliberate difference: `daily_averages` skips a day without windows or without data, where the loop of the
reference's __main__ stops with an exception.
Not built: the plots, s4:main's moving of figures and movies, `cleanup`.
"""
import ctypes as C
import datetime as dt
import glob
import os

import numpy as np

from . import _lib
from .context import Context
from .day_grid import EPOCH, epoch_seconds

STAMP = "%Y%m%d_%H%M"


def _nan(*shape):
    a = np.empty(shape)
    a[:] = np.nan
    return a


def datetime_to_matlab(t):
    """util.datetime2matlab: MATLAB's datenum of a datetime (ordinal + 366 days + the fraction of the day)."""
    midnight = dt.datetime(t.year, t.month, t.day, 0, 0, 0)
    day_fraction = (t - midnight).seconds / (24.0 * 60.0 * 60.0)
    micro_fraction = t.microsecond / (24.0 * 60.0 * 60.0 * 1000000.0)
    return (t + dt.timedelta(days=366)).toordinal() + day_fraction + micro_fraction


def epoch_to_datetime(seconds):
    return dt.timedelta(seconds=seconds) + EPOCH


def velocities_to_regular_grid(npz, extra=()):
    """One window file of s3 -> rasters (s4:120-168): [x_ras, y_ras, u_ras, v_ras, speed_ras, count_ras, xx, yy, ii,
    jj, cols, rows].  Raster index is [j, i]; cells the file does not list are NaN.  `extra`: names of further per-cell
    fields of the file (the statistics of day_grid's stats=True, say); their rasters follow as a thirteenth entry, a
    dict by name.  A file without one of them raises ValueError."""
    extra = tuple(extra)
    with np.load(npz) as z:
        missing = [k for k in extra if k not in z.files]
        if missing:
            raise ValueError("%s has no %s" % (npz, ", ".join(missing)))
        i, j = z["i"], z["j"]
        fields = [z[k] for k in ("x", "y", "u", "v", "speed", "count") + extra]
        grid_size, topleft, cols, rows = z["grid_size"], z["topleft"], z["cols"], z["rows"]
    rasters = [_nan(rows, cols) for _ in fields]
    if len(i):          # a window with points and no kept cell stores empty float64 i, j: nothing to place
        for ras, f in zip(rasters, fields):
            ras[j, i] = f
    x = np.arange(topleft[0], topleft[0] + cols * grid_size, grid_size)
    y = np.arange(topleft[1] - (rows - 1) * grid_size, topleft[1] + 1 * grid_size, grid_size)
    xx, yy = np.meshgrid(x, y, indexing="xy")
    yy = np.flipud(yy)
    ii, jj = np.meshgrid(range(0, rows), range(0, cols), indexing="ij")
    out = rasters[:6] + [xx, yy, ii, jj, cols, rows]
    return out + [dict(zip(extra, rasters[6:]))] if extra else out


def combine_npzs(folder, npz_workspace, npz_combined_name, save=True, extra=()):
    """The window files of `folder` (sorted) stacked into the run's cube (s4:170-210): a dict with x, y, i, j, u, v,
    speed, count (rows, cols, n_files), time (epoch seconds), time_matlab; written with np.savez when `save`.  Rows
    and cols are the first file's; a file of another shape raises ValueError.  `extra`: names of further per-cell fields
    of the window files, stacked like u into (rows, cols, n_files) NaN-filled arrays beside the cube's own; a file that
    lacks one raises ValueError.  They stay on the host: the averages of the device cube do not take them."""
    extra = tuple(extra)
    if set(extra) & {"x", "y", "i", "j", "u", "v", "speed", "count", "time", "time_matlab"}:
        raise ValueError("extra names a field the cube already has")
    npzs = sorted(glob.glob(os.path.join(folder, "*.npz")))
    first = velocities_to_regular_grid(npzs[0], extra)
    cols, rows = first[10], first[11]
    n = len(npzs)
    u, v, speed, count = (_nan(rows, cols, n) for _ in range(4))
    time, time_matlab = _nan(n), _nan(n)
    more = {name: _nan(rows, cols, n) for name in extra}
    for k, path in enumerate(npzs):
        _, _, u_ras, v_ras, speed_ras, count_ras, xx, yy, ii, jj, _, _, *extra_ras = velocities_to_regular_grid(path, extra)
        for name in extra:
            more[name][:, :, k] = extra_ras[0][name]
        u[:, :, k] = u_ras
        v[:, :, k] = v_ras
        speed[:, :, k] = speed_ras
        count[:, :, k] = count_ras
        stamp = dt.datetime.strptime(os.path.basename(path).split("-")[0], STAMP)
        time[k] = epoch_seconds(stamp)
        time_matlab[k] = datetime_to_matlab(stamp)
    cube = dict(x=xx, y=yy, i=ii, j=jj, u=u, v=v, speed=speed, count=count, time=time, time_matlab=time_matlab, **more)
    if save:
        np.savez(os.path.join(npz_workspace, npz_combined_name), **cube)
    return cube


# ---- exports (host) ---------------------------------------------------------------------------------------------

def npz_to_mat(np_file, targetfolder):
    """The cube as a .mat file of the same base name (s4:212-228); `time` is the MATLAB datenum."""
    import scipy.io                              # only this export needs scipy
    with np.load(np_file) as z:
        out = {k: z[k] for k in ("x", "y", "u", "v", "speed", "count")}
        out["time"] = z["time_matlab"]
    scipy.io.savemat(os.path.join(targetfolder, os.path.basename(np_file).replace(".npz", ".mat")), out)


def _csv(folder, name, a, fmt):
    np.savetxt(os.path.join(folder, name + ".csv"), a, fmt=fmt, delimiter=",")


def npz_to_csv(file_loaded, targetfolder, name_fjord):
    """Every window of the cube as u / v / count csv files plus easting and northing (s4:230-241)."""
    _csv(targetfolder, name_fjord + "_easting", file_loaded["x"], "%.2f")
    _csv(targetfolder, name_fjord + "_northing", file_loaded["y"], "%.2f")
    u, v, count, time = (file_loaded[k] for k in ("u", "v", "count", "time"))
    for k in range(u.shape[2]):
        stamp = epoch_to_datetime(time[k]).strftime("%Y%m%d%H%M%S")
        _csv(targetfolder, name_fjord + "_u_" + stamp, u[:, :, k], "%.4f")
        _csv(targetfolder, name_fjord + "_v_" + stamp, v[:, :, k], "%.4f")
        _csv(targetfolder, name_fjord + "_count_" + stamp, count[:, :, k], "%.0f")


def save_csv(x, y, u, v, count, time_str, targetfolder, name_fjord):
    """One averaged field as csv files (s4:244-256)."""
    _csv(targetfolder, name_fjord + "_easting", x, "%.2f")
    _csv(targetfolder, name_fjord + "_northing", y, "%.2f")
    _csv(targetfolder, name_fjord + "_u_" + time_str, u, "%.4f")
    _csv(targetfolder, name_fjord + "_v_" + time_str, v, "%.4f")
    _csv(targetfolder, name_fjord + "_count_" + time_str, count, "%.0f")


# ---- averages (device) ------------------------------------------------------------------------------------------

def spatial_mean_host(variable, coarseness):
    """spatial_mean(variable, coarseness, nanmean=0) of s4:264-287 on the host: used for the coordinate grids, which
    never reach the device."""
    rows, cols = variable.shape
    pr, pc = -(-rows // coarseness) * coarseness, -(-cols // coarseness) * coarseness
    padded = np.zeros((pr, pc))
    padded[:rows, :cols] = variable
    return np.mean(padded.reshape(pr // coarseness, coarseness, pc // coarseness, coarseness), axis=(1, 3))


def select_windows(time, periods):
    """Per period (start, end) the ascending indices of the windows with start <= time < end (int epoch bounds
    compared with the float64 times) as CSR (offsets int32 (n + 1), indices int32), and the periods' time_str
    ('%Y%m%d_%H%M' of the earliest selected time + '-%H%M' of the latest; None when nothing is selected)."""
    time = np.asarray(time, np.float64)
    offsets, chunks, names = [0], [], []
    for start, end in periods:
        mask = (time >= epoch_seconds(start)) & (time < epoch_seconds(end))
        idx = np.flatnonzero(mask)
        chunks.append(idx)
        offsets.append(offsets[-1] + len(idx))
        names.append(epoch_to_datetime(time[idx].min()).strftime(STAMP) + epoch_to_datetime(time[idx].max()).strftime("-%H%M")
                     if len(idx) else None)
    if offsets[-1] > 0x7fffffff:
        raise ValueError("more than 2^31 selected windows in one request")
    index = np.concatenate(chunks).astype(np.int32) if chunks else np.zeros(0, np.int32)
    return np.array(offsets, np.int32), index, names


class VelocityCube:
    """The cube of `combine_npzs` (its dict, an open npz or a path) with u, v, count resident on the device; x, y and
    time stay on the host.  A context holds one cube at a time (a second one on the same context raises until the first
    is closed); without `ctx` the cube makes and owns a context."""

    def __init__(self, npz_or_dict, ctx=None):
        z = np.load(npz_or_dict) if isinstance(npz_or_dict, (str, os.PathLike)) else npz_or_dict
        u, v, count = (np.asarray(z[k], np.float64) for k in ("u", "v", "count"))
        if u.ndim != 3 or v.shape != u.shape or count.shape != u.shape or u.size == 0:
            raise ValueError("u, v, count must be (rows, cols, windows) arrays of one shape")
        self.rows, self.cols, self.nt = u.shape
        self.x, self.y = np.asarray(z["x"]), np.asarray(z["y"])
        self.time = np.asarray(z["time"], np.float64)
        if hasattr(z, "close") and z is not npz_or_dict:
            z.close()
        if ctx is not None and getattr(ctx, "_cube", None) is not None:
            raise _lib.IcelkError("this context already holds a velocity cube: close that one first")
        self._own = ctx is None
        self.ctx = Context(64, 64, n_slots=1, max_pts=1024) if self._own else ctx
        self._set = False
        try:
            # the device wants the cell index fastest: (rows, cols, T) -> [window][row * cols + col], transposed here
            planes = [np.ascontiguousarray(np.moveaxis(a, 2, 0)) for a in (u, v, count)]
            f64 = lambda a: a.ctypes.data_as(_lib.f64p)               # noqa: E731
            self.ctx._ck(self.ctx._lib.icelk_cube_set(self.ctx._h, f64(planes[0]), f64(planes[1]), f64(planes[2]),
                                                      self.rows * self.cols, self.nt))
            self._set = True
            self.ctx._cube = self
        except Exception:
            self.close()
            raise

    def close(self):
        if self._set:
            if self.ctx._h.value:
                self.ctx._lib.icelk_cube_release(self.ctx._h)
            self.ctx._cube = None
        self._set = False
        if self._own:
            self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def average_periods(cube, periods, coarseness=1, timing=None):
    """Every period (start, end) of the list in one device pass.  Per period a dict: u, v, count (np.nanmean,
    np.nanmean, np.nansum over the period's windows, then spatial_mean for coarseness > 1), speed = np.hypot(u, v), x,
    y (coarsened likewise), none of them flipped; has_data (some cell has a speed) and time_str (None for a period
    that selects no window).  `timing`: a dict that receives the kernels' milliseconds."""
    coarseness = int(coarseness)
    offsets, index, names = select_windows(cube.time, periods)
    n = len(names)
    if n == 0:
        return []
    cr, cc = -(-cube.rows // max(coarseness, 1)), -(-cube.cols // max(coarseness, 1))
    u, v, speed, count = (np.zeros((n, cr, cc), np.float64) for _ in range(4))
    has = np.zeros(n, np.int32)
    f64 = lambda a: a.ctypes.data_as(_lib.f64p)               # noqa: E731
    i32 = lambda a: a.ctypes.data_as(_lib.i32p)               # noqa: E731
    device_ms = C.c_double(0.0)
    ctx = cube.ctx
    ctx._ck(ctx._lib.icelk_cube_average(ctx._h, i32(offsets), i32(index), n, cube.rows, cube.cols, coarseness, f64(u),
                                        f64(v), f64(speed), f64(count), i32(has),
                                        C.byref(device_ms) if timing is not None else None))
    if timing is not None:
        timing.update(kernels_ms=device_ms.value, selected=int(offsets[-1]))
    x, y = cube.x, cube.y
    if coarseness > 1:
        x, y = spatial_mean_host(x, coarseness), spatial_mean_host(y, coarseness)
    return [dict(x=x, y=y, u=u[p], v=v[p], speed=speed[p], count=count[p], has_data=bool(has[p]) and names[p] is not None,
                 time_str=names[p]) for p in range(n)]


def average_spatially_temporally(start_time, end_time, coarseness, npz_or_cube, ctx=None):
    """The reference's function without its plot (s4:289-479): [x, y, u, v, count, time_str] of the period
    [start_time, end_time) -- for coarseness 1 with y, u, v upside down, as the reference returns them -- or six NaN
    when no selected cell holds data.  Raises ValueError when the period selects no window."""
    own = not isinstance(npz_or_cube, VelocityCube)
    cube = VelocityCube(npz_or_cube, ctx) if own else npz_or_cube
    try:
        if select_windows(cube.time, [(start_time, end_time)])[2][0] is None:
            raise ValueError("no window of the cube lies in [%s, %s)" % (start_time, end_time))
        r = average_periods(cube, [(start_time, end_time)], coarseness)[0]
    finally:
        if own:
            cube.close()
    if not r["has_data"]:
        return [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]
    if coarseness == 1:
        return [r["x"], np.flipud(r["y"]), np.flipud(r["u"]), np.flipud(r["v"]), r["count"], r["time_str"]]
    return [r["x"], r["y"], r["u"], r["v"], r["count"], r["time_str"]]


def daily_averages(cube, days, start_hour=12, duration_hours=22, coarseness=1, csv_workspace=None,
                   name_fjord="JohnsHopkins"):
    """The loop of the reference's __main__ (s4:519-537) with all days in one device pass: per day the period
    [day + start_hour, + duration_hours), and what the loop hands to save_csv -- [x, y, u, v, count, time_str] after
    its np.flipud of y, u, v (which undoes the flip for coarseness 1 and turns the coarse fields upside down
    otherwise).  With `csv_workspace` the files are written.  Returns [(day, that list)]; a day without windows or
    without data is left out (the reference's loop stops there with an exception)."""
    periods = [(day + dt.timedelta(hours=start_hour), day + dt.timedelta(hours=start_hour + duration_hours))
               for day in days]
    out = []
    for day, r in zip(days, average_periods(cube, periods, coarseness)):
        if not r["has_data"]:
            continue
        y, u, v = r["y"], r["u"], r["v"]
        if coarseness != 1:
            y, u, v = np.flipud(y), np.flipud(u), np.flipud(v)
        fields = [r["x"], y, u, v, r["count"], r["time_str"]]
        if csv_workspace is not None:
            save_csv(*fields, csv_workspace, name_fjord)
        out.append((day, fields))
    return out

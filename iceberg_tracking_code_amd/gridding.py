"""Gridding of the projected velocities -- host-side mirror of the parts of s3_utm_to_gridded_utm.py that touch every
point: `trm.create_grid_across_fjord` (imports/tracking_misc.py:23-56) and the per-cell selection / averaging loop
(s3:391-421).  Point-in-polygon tests, the per-cell sums (numpy's pairwise order) and the speeds run on the GPU
(`icelk_points_in_polygon`, `icelk_grid_bin`, csrc/k_grid.hip); what stays here is the cell geometry of a few hundred
squares and the packing of the result arrays the reference hands to np.savez (s3:441-445).  No CPU fallback.

The day driver around the loop -- schedule, time windows, clock drift, selection from the hourly files, every window
of a day binned in one device pass (`icelk_grid_bin_windows`) -- is day_grid.utm_to_gridded_utm; `pack_cells` and
`cell_table` here serve both.  The map of a window is velocity_map.py.
"""
import ctypes as C
import math

import numpy as np

from . import _lib


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def points_in_polygon(ctx, poly, points):
    """matplotlib.path.Path(poly).contains_points(points) (radius 0) -> bool array."""
    p = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 2)
    q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(len(q), np.uint8)
    ctx._ck(ctx._lib.icelk_points_in_polygon(ctx._h, _f64(p), len(p), _f64(q), len(q), out.ctypes.data_as(_lib.u8p)))
    return out.astype(bool)


def create_grid_across_fjord(ctx, fjord, spacing):
    """What trm.create_grid_across_fjord returns (tracking_misc.py:23-56): [polygons, centerpoints, indices,
    topleft_px_center, rows, cols] -- squares of `spacing` laid from the top-left corner of the fjord outline, column
    by column, kept when the outline contains the cell centre.  All cells are formed at once (the same float64
    expressions per cell: corner = left + i * spacing, top - j * spacing; centre = corner +/- 0.5 * spacing) and the
    containment test runs on the GPU for all centres together.  `fjord` has 'x' and 'y' arrays."""
    fx, fy = np.asarray(fjord["x"]), np.asarray(fjord["y"])
    left, right, bottom, top = min(fx), max(fx), min(fy), max(fy)
    cols = int(math.ceil((right - left) / spacing))
    rows = int(math.ceil((top - bottom) / spacing))
    ii, jj = (a.ravel() for a in np.meshgrid(np.arange(cols), np.arange(rows), indexing="ij"))   # i-major, as s3 walks
    ox, oy = left + ii * spacing, top - jj * spacing
    centers = np.stack([ox + 0.5 * spacing, oy - 0.5 * spacing], 1)
    keep = points_in_polygon(ctx, np.vstack((fx, fy)).T, centers) if len(centers) else np.zeros(0, bool)
    polygons = [[(x, y), (x + spacing, y), (x + spacing, y - spacing), (x, y - spacing)]
                for x, y in zip(ox[keep], oy[keep])]
    return [polygons, [list(c) for c in centers[keep]], [[int(i), int(j)] for i, j in zip(ii[keep], jj[keep])],
            [left + 0.5 * spacing, top - 0.5 * spacing], rows, cols]


def cell_table(grid, fjord):
    """(left, top, cell_on, idx) of a grid for the kernels: cell_on[i * rows + j] = 1 for the kept cells, idx = that
    index of every kept cell in the grid's order."""
    indices, rows, cols = grid[2], grid[4], grid[5]
    fx, fy = np.asarray(fjord["x"]), np.asarray(fjord["y"])
    on = np.zeros(cols * rows, np.uint8)
    idx = np.array([i * rows + j for i, j in indices], np.int64)
    on[idx] = 1
    return float(min(fx)), float(max(fy)), on, idx


STATS_KEYS = ("u_std", "v_std", "u_median", "v_median", "speed_median", "u_mad", "v_mad")
_STATS_FIELDS = ("std_u", "std_v", "median_u", "median_v", "mad_u", "mad_v")          # icelk_grid_stats_t's members
_STATS_OF_KEY = dict(u_std="std_u", v_std="std_v", u_median="median_u", v_median="median_v", u_mad="mad_u", v_mad="mad_v")


class CellStats:
    """The six per-cell arrays of icelk_grid_stats_t for `nseg` cells (or windows x cells), and the struct over them."""

    def __init__(self, nseg):
        self.arrays = {k: np.zeros(nseg, np.float64) for k in _STATS_FIELDS}
        self.struct = _lib.GridStats(*[_f64(self.arrays[k]) for k in _STATS_FIELDS])

    def window(self, s):
        """what `pack_cells` takes as `stats`, for the cells of slice s"""
        return {k: a[s] for k, a in self.arrays.items()}


def grid_cell_stats_host(a):
    """(std, median, mad) of one cell's values by the library's host statement of the rules (csrc/grid_stats.h,
    `icelk_grid_cell_stats_host`): np.std(a, ddof=1), np.median(a), np.median(np.abs(a - np.median(a))), bit for bit
    numpy 2.2's; all NaN for an empty cell.  No GPU."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    out = [C.c_double(0.0) for _ in range(3)]
    _lib.check(_lib.load().icelk_grid_cell_stats_host(_f64(a), len(a), *[C.byref(o) for o in out]))
    return tuple(np.float64(o.value) for o in out)


def bin_velocities(ctx, x, y, u, v, fjord, spacing, observation_threshold, grid=None, stats=False, validate=None):
    """The loop of s3:391-421 for one time window.  Returns the dict the reference saves (s3:441-445, without
    `grid_size` / `topleft` / `rows` / `cols`, which the caller has): grid_id, i, j, x, y, u, v, speed, count,
    measured, not_measured.  With `stats` also, as lists over the measured cells, u_std, v_std (np.std(ddof=1) of the
    cell's velocities), u_median, v_median, speed_median (their np.hypot), u_mad, v_mad (median absolute deviation),
    from `icelk_grid_bin_stats`.  `validate`: None, True or a dict (validate.validate_options): the normalised median test
    (`validate_velocities`, one group, a lattice over the fjord's box) runs first, everything is computed from the
    surviving points, and the dict also has `rejected` (their number), `validation` (threshold, eps, min_neighbours, side)
    and `status` (per point).  validate=None calls nothing of it."""
    if validate is not None and validate is not False:
        from .validate import validate_options, validate_velocities, validation_array, validation_lattice
        opt = validate_options(validate, spacing)
        res = validate_velocities(ctx, x, y, u, v, validation_lattice(fjord, opt["side"]), opt["threshold"], opt["eps"],
                                  opt["min_neighbours"])
        keep = res["keep"]
        out = bin_velocities(ctx, *[np.asarray(q, np.float64).ravel()[keep] for q in (x, y, u, v)], fjord, spacing,
                             observation_threshold, grid=grid, stats=stats)
        out.update(rejected=int((~keep).sum()), validation=validation_array(opt), status=res["status"])
        return out
    if grid is None:
        grid = create_grid_across_fjord(ctx, fjord, spacing)
    rows, cols = grid[4], grid[5]
    left, top, on, idx = cell_table(grid, fjord)
    a = [np.ascontiguousarray(t, dtype=np.float64).ravel() for t in (x, y, u, v)]
    n = len(a[0])
    cnt = np.zeros(cols * rows, np.int32)
    mu, mv, sp = (np.zeros(cols * rows, np.float64) for _ in range(3))
    args = (ctx._h, _f64(a[0]), _f64(a[1]), _f64(a[2]), _f64(a[3]), n, left, top, float(spacing), cols, rows,
            on.ctypes.data_as(_lib.u8p), cnt.ctypes.data_as(_lib.i32p), _f64(mu), _f64(mv), _f64(sp))
    if not stats:
        ctx._ck(ctx._lib.icelk_grid_bin(*args))
        return pack_cells(grid, idx, cnt, mu, mv, sp, observation_threshold)
    cs = CellStats(cols * rows)
    ctx._ck(ctx._lib.icelk_grid_bin_stats(*args, C.byref(cs.struct)))
    return pack_cells(grid, idx, cnt, mu, mv, sp, observation_threshold, stats=cs.arrays)


def hypot_of_medians(median_u, median_v):
    """speed_median: np.hypot of the two medians, as the reference forms `speed` from the two means (numpy's hypot is the
    one csrc/np_sums.h's hypot_np restates)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.hypot(median_u, median_v)


def pack_cells(grid, idx, cnt, mu, mv, sp, observation_threshold, stats=None):
    """The lists s3:391-421 fills, from per-cell results indexed i * rows + j (idx: that index of every kept cell).
    `stats`: the six per-cell arrays std_u, std_v, median_u, median_v, mad_u, mad_v indexed likewise; the dict then
    also has the lists of STATS_KEYS over the measured cells."""
    polygons, centers, indices = grid[:3]
    out = {k: [] for k in ("grid_id", "i", "j", "x", "y", "u", "v", "speed", "count", "measured", "not_measured")}
    if stats is not None:
        out.update({k: [] for k in STATS_KEYS})
        speed_median = hypot_of_medians(stats["median_u"], stats["median_v"])
    for counter, (poly, center, index, c) in enumerate(zip(polygons, centers, indices, idx)):
        nobs = int(cnt[c])
        if nobs > observation_threshold:                                   # s3:400
            out["grid_id"].append(counter)
            out["i"].append(index[0])
            out["j"].append(index[1])
            out["x"].append(center[0])
            out["y"].append(center[1])
            out["u"].append(mu[c])
            out["v"].append(mv[c])
            out["speed"].append(sp[c])
            out["count"].append(nobs)
            out["measured"].append(poly)
            if stats is not None:
                for key, field in _STATS_OF_KEY.items():
                    out[key].append(stats[field][c])
                out["speed_median"].append(speed_median[c])
        else:
            out["not_measured"].append(poly)
    out["counts_all"] = cnt[idx].astype(np.int64)
    return out

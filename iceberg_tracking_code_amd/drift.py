"""Virtual drifters: particles advected through the gridded velocities.

Where does ice released at the terminus go, how long does it stay, where did the ice in front of a haul-out come from: a
drifter follows one piece of ice through the velocity cube (`VelocityCube`, daylight only) or through a tidal fit of it
(`TideFit`, which also exists at night).  A drifter in a steady field draws a streamline.

The rule (csrc/drift.h; `drift_host` is that text on the CPU, csrc/k_drift.hip the kernels, tests/drift_restatement.py a
restatement in numpy; the three agree bit for bit), everything in double:
- lattice: the cube's nodes x0 + i * dx, y0 + j * dy, row 0 the northern row (`drift_lattice`);
- clock: all drifters share t_s = start + s * step, s = 0 .. nsteps; a negative step runs the field backwards;
- schedule (`drift_schedule`, made here on the host): one row per half step -- for the cube the bracketing windows k0 <= k1,
  the weight a = (t - time[k0]) / (time[k1] - time[k0]) and a flag, 0 outside the record or across a gap longer than
  `max_gap` (policy: twice the median window spacing); for a fit the basis row of that time.  The library searches no time
  axis and evaluates no sine;
- a cube node is measured iff u, v are finite and count >= min_count in both windows, its value (1 - a) * u[k0] + a * u[k1];
  a fit's node is measured iff the cell's status is 0, its value the sum of `TideFit.predict`;
- a sample is bilinear over the four nodes around the position; with fewer than four measured, but at least `min_nodes` and
  a positive weight sum, the measured ones renormalised; a position outside the lattice has no sample;
- a step is Euler (order 1), midpoint (2) or classical Runge-Kutta (4); the first stage without a velocity stops the drifter
  where it was.
`status`: 0 alive at the end, 1 left the lattice, 2 too few measured nodes, 3 no field at that time, 4 never released (a
non-finite seed, or a release step outside 0 .. nsteps - 1).

Declared differences from an ocean particle tracker (OpenDrift, Parcels): no sub-grid diffusion, no windage, no beaching
model; the field is linear in time between windows; the step is fixed.  `max_gap` and `min_nodes` are policy, not
measurements.
"""
import ctypes as C

import numpy as np

from . import _lib
from .postprocess import VelocityCube
from .tides import MAX_TERMS, TideFit

DRIFT_ALIVE, DRIFT_LEFT, DRIFT_TOO_FEW, DRIFT_NO_FIELD, DRIFT_NEVER_RELEASED = 0, 1, 2, 3, 4
_PER_DRIFTER = ("last_x", "last_y", "length", "status", "stop_step")


def drift_lattice(cube):
    """The `_lib.DriftLattice` of a cube: a `VelocityCube`, the dict of `combine_npzs` or anything else with x, y as (rows,
    cols) arrays; a `_lib.DriftLattice` passes through.  ValueError for fewer than 2 x 2 nodes or nodes that do not lie at x0 +
    i * dx, y0 + j * dy to within a millionth of the spacing."""
    if isinstance(cube, _lib.DriftLattice):
        return cube
    x, y = (np.asarray(cube.x if hasattr(cube, "x") else cube["x"], np.float64), np.asarray(cube.y if hasattr(cube, "y") else cube["y"], np.float64))
    if x.ndim != 2 or y.shape != x.shape or x.shape[0] < 2 or x.shape[1] < 2:
        raise ValueError("a lattice needs x, y as (rows, cols) arrays of 2 x 2 nodes at least")
    rows, cols = x.shape
    x0, y0, dx, dy = float(x[0, 0]), float(y[0, 0]), float(x[0, 1] - x[0, 0]), float(y[1, 0] - y[0, 0])
    if not all(np.isfinite(q) for q in (x0, y0, dx, dy)) or dx == 0 or dy == 0:
        raise ValueError("the lattice's origin and spacing must be finite, the spacing not 0")
    off_x = np.abs(x - (x0 + dx * np.arange(cols))[None, :]).max()
    off_y = np.abs(y - (y0 + dy * np.arange(rows))[:, None]).max()
    if not (off_x <= 1e-6 * abs(dx) and off_y <= 1e-6 * abs(dy)):
        raise ValueError("the lattice is not regular: nodes lie up to %g, %g off x0 + i * dx, y0 + j * dy" % (off_x, off_y))
    return _lib.DriftLattice(x0, y0, dx, dy, rows, cols)


def schedule_times(start, step, nsteps):
    """The 2 * nsteps + 1 times of the schedule rows: t_s = start + s * step, and t_s + step / 2 between them"""
    start, step, nsteps = float(start), float(step), int(nsteps)
    if not (np.isfinite(start) and np.isfinite(step)) or step == 0 or nsteps < 1:
        raise ValueError("start and step must be finite, step not 0, nsteps at least 1")
    whole = start + np.arange(nsteps + 1, dtype=np.float64) * step
    t = np.empty(2 * nsteps + 1, np.float64)
    t[0::2] = whole
    t[1::2] = whole[:-1] + step / 2.0
    return t


def drift_schedule(time, start, step, nsteps, max_gap=None):
    """The cube source's schedule table: a dict of t (the rows' times), k0, k1 (int32), a (float64), flag (int32), each 2 *
    nsteps + 1 long.  `time`: the cube's window times, finite and strictly ascending.  Row r: the windows k0 <= k1 that bracket
    t[r] (k0 == k1 and a = 0 on an exact hit), a = (t - time[k0]) / (time[k1] - time[k0]); flag 0 -- and k0 = k1 = 0, a = 0 --
    when t lies outside the record, flag 0 as well when time[k1] - time[k0] > max_gap.  max_gap None: twice the median window
    spacing (policy; no limit for a cube of one window)."""
    time = np.asarray(time, np.float64).ravel()
    if time.size == 0 or not np.all(np.isfinite(time)) or np.any(np.diff(time) <= 0):
        raise ValueError("the window times must be finite and strictly ascending, and one at least")
    if max_gap is None:
        max_gap = 2.0 * float(np.median(np.diff(time))) if time.size > 1 else np.inf
    max_gap = float(max_gap)
    if np.isnan(max_gap):
        raise ValueError("max_gap is NaN")
    t = schedule_times(start, step, nsteps)
    inside = (t >= time[0]) & (t <= time[-1])
    k1 = np.minimum(np.searchsorted(time, t, side="left"), time.size - 1)
    hit = time[k1] == t
    k0 = np.where(hit, k1, np.maximum(k1 - 1, 0))
    span = time[k1] - time[k0]
    with np.errstate(all="ignore"):
        a = np.where(hit, 0.0, (t - time[k0]) / span)
    flag = inside & (span <= max_gap)
    k0, k1, a = np.where(inside, k0, 0), np.where(inside, k1, 0), np.where(inside, a, 0.0)
    return dict(t=t, k0=k0.astype(np.int32), k1=k1.astype(np.int32), a=a.astype(np.float64), flag=flag.astype(np.int32))


def seed_nodes(cube, stride=1, measured_in=None):
    """(x, y), flat: every `stride`-th node of the cube's lattice in both directions.  measured_in: a (rows, cols) boolean
    array, or a `TideFit` (its fitted cells): only nodes where it holds are kept."""
    x, y = (np.asarray(cube.x if hasattr(cube, "x") else cube["x"], np.float64), np.asarray(cube.y if hasattr(cube, "y") else cube["y"], np.float64))
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1")
    keep = np.zeros(x.shape, bool)
    keep[::stride, ::stride] = True
    if measured_in is not None:
        mask = measured_in.status == 0 if isinstance(measured_in, TideFit) else np.asarray(measured_in, bool)
        if mask.shape != x.shape:
            raise ValueError("measured_in must have the lattice's shape")
        keep &= mask
    return x[keep].copy(), y[keep].copy()


def seed_line(p1, p2, n):
    """(x, y): n seeds from p1 to p2, ends included, laid out as `transect.locate_points_along_transect` lays its points: p1 +
    c * dist * (cos, sin) of the line's azimuth, dist = length / (n - 1)"""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    u, v = float(p2[0]) - float(p1[0]), float(p2[1]) - float(p1[1])
    dist = np.hypot(u, v) / (n - 1) if n > 1 else 0.0
    azimuth = np.arctan2(v, u)
    c = np.arange(n, dtype=np.float64)
    return float(p1[0]) + c * (np.cos(azimuth) * dist), float(p1[1]) + c * (np.sin(azimuth) * dist)


class DriftResult:
    """What a run returns.  x, y (n_out, n): the positions at `time` (n_out,), NaN before a drifter's release and after its
    stop; status, stop_step (the step that failed; nsteps for a drifter alive at the end, -1 if never released), last_x,
    last_y, length (the sum of np.hypot of the step displacements), each (n,); visits int32 (rows, cols) or None: recorded
    finite samples per nearest node."""
    FIELDS = ("x", "y", "time") + _PER_DRIFTER

    def __init__(self, fields):
        self.visits = None
        self.__dict__.update(fields)

    def save(self, path):
        extra = {} if self.visits is None else {"visits": self.visits}
        np.savez(path, **{k: getattr(self, k) for k in self.FIELDS}, **extra)


def load_drift(path):
    """A `DriftResult` from the .npz that `DriftResult.save` wrote"""
    with np.load(path, allow_pickle=False) as z:
        fields = {k: z[k] for k in DriftResult.FIELDS}
        fields["visits"] = z["visits"] if "visits" in z.files else None
    return DriftResult(fields)


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def _i32(a):
    return a.ctypes.data_as(_lib.i32p)


def _params(step, nsteps, every, order, min_nodes):
    step, nsteps, every, order, min_nodes = float(step), int(nsteps), int(every), int(order), int(min_nodes)
    if not np.isfinite(step) or step == 0 or nsteps < 1 or every < 1:
        raise ValueError("step must be finite and not 0, nsteps and every at least 1")
    if order not in (1, 2, 4) or not 1 <= min_nodes <= 4:
        raise ValueError("order is 1, 2 or 4, min_nodes 1 .. 4")
    return _lib.DriftParams(step, nsteps, every, order, min_nodes)


def _seeds(x, y, release):
    x, y = (np.ascontiguousarray(np.asarray(a, np.float64).ravel()) for a in (x, y))
    if x.size == 0 or y.size != x.size:
        raise ValueError("x and y must be seeds of one length, one at least")
    release = np.zeros(x.size, np.int32) if release is None else np.asarray(release)
    if release.dtype.kind not in "iu":
        raise ValueError("release must be integer steps")
    release = np.clip(release, -1, 0x7fffffff).astype(np.int32).ravel()       # a negative step, like one past the run: never released
    if release.size not in (1, x.size):
        raise ValueError("release must have one step per seed")
    release = np.ascontiguousarray(np.broadcast_to(release, x.shape))
    return x, y, release


def drift_arrays(call, handle, lattice, params, x, y, release, visits=False, timing=None):
    """Allocate the outputs of one run and call `call(seed_x, seed_y, release, n, out, device_ms)`: a dict of x, y (n_out, n),
    last_x, last_y, length, status, stop_step (n) and visits ((rows, cols) or None)"""
    n = x.size
    n_out = params.nsteps // params.every + 1
    big = n * n_out >= 1 << 31                                # refused by the library; nothing this large is allocated for it
    out = {k: np.zeros((1, 1) if big else (n_out, n), np.float64) for k in ("x", "y")}
    out.update({k: np.zeros(n, np.float64 if k[0] == "l" else np.int32) for k in _PER_DRIFTER})
    out["visits"] = np.zeros((lattice.rows, lattice.cols), np.int32) if visits else None
    o = _lib.DriftOut(*[_f64(out[k]) for k in ("x", "y", "last_x", "last_y", "length")], _i32(out["status"]), _i32(out["stop_step"]),
                      _i32(out["visits"]) if visits else None)
    device_ms = C.c_double(0.0)
    rc = call(_f64(x), _f64(y), _i32(release), n, C.byref(o), C.byref(device_ms) if timing is not None else None)
    _lib.check(rc, handle)
    if timing is not None:
        timing.update(kernels_ms=device_ms.value)
    return out


def _tide_tables(fit, lattice, t):
    rows, cols, m = fit.coef_u.shape
    if (rows, cols) != (lattice.rows, lattice.cols):
        raise ValueError("the fit has %d x %d cells, the lattice %d x %d nodes" % (rows, cols, lattice.rows, lattice.cols))
    if m > MAX_TERMS:
        raise ValueError("more than %d terms" % MAX_TERMS)
    coef = [np.ascontiguousarray(a.reshape(-1, m), dtype=np.float64) for a in (fit.coef_u, fit.coef_v)]
    return coef[0], coef[1], np.ascontiguousarray(fit.status.ravel(), dtype=np.int32), np.ascontiguousarray(fit.basis(t), dtype=np.float64), m


def _result(out, start, params):
    fields = dict(out)
    fields["time"] = float(start) + np.arange(0, params.nsteps + 1, params.every, dtype=np.float64) * params.step
    return DriftResult(fields)


def _is_pair(source):
    return isinstance(source, (tuple, list)) and len(source) == 2 and isinstance(source[0], TideFit)


def drift(source, x, y, start, nsteps, step=60.0, release=None, order=4, min_nodes=4, min_count=1, max_gap=None, every=1, visits=False,
          timing=None, ctx=None):
    """Advect drifters on the device.  source: a `VelocityCube` (`icelk_cube_drift`; the cube is not changed), or a pair
    (`TideFit`, cube or lattice) (`icelk_drift_tide`; it runs on the fit's context, the cube's, or `ctx`).  x, y: the seeds;
    start: epoch seconds of step 0; nsteps steps of `step` seconds (negative: backwards); release: the step at which each
    drifter appears (None: 0); order 1, 2 or 4; min_nodes 1 .. 4 measured nodes a sample needs; min_count: a window's node is
    measured iff u, v are finite and count >= min_count; max_gap: seconds, see `drift_schedule`; every: positions are recorded
    at the steps 0, every, 2 * every, ...; visits: also count the recorded samples per nearest node; timing: a dict that
    receives the kernels' milliseconds.  Returns a `DriftResult`."""
    params = _params(step, nsteps, every, order, min_nodes)
    sx, sy, rel = _seeds(x, y, release)
    if isinstance(source, VelocityCube):
        lattice = drift_lattice(source)
        ctx = source.ctx
        S = drift_schedule(source.time, start, step, nsteps, max_gap)

        def call(*args):
            return ctx._lib.icelk_cube_drift(ctx._h, C.byref(lattice), C.byref(params), _i32(S["k0"]), _i32(S["k1"]), _f64(S["a"]),
                                             _i32(S["flag"]), float(min_count), *args)
    elif _is_pair(source):
        fit = source[0]
        lattice = drift_lattice(source[1])
        ctx = ctx if ctx is not None else (fit.ctx if fit.ctx is not None else getattr(source[1], "ctx", None))
        if ctx is None:
            raise ValueError("drift runs on the device: give a Context")
        cu, cv, status, B, m = _tide_tables(fit, lattice, schedule_times(start, step, nsteps))

        def call(*args):
            return ctx._lib.icelk_drift_tide(ctx._h, C.byref(lattice), C.byref(params), _f64(cu), _f64(cv), _i32(status), m, _f64(B), *args)
    else:
        raise ValueError("source is a VelocityCube or a (TideFit, cube or lattice) pair")
    return _result(drift_arrays(call, ctx._h, lattice, params, sx, sy, rel, visits, timing), start, params)


def drift_host(source, x, y, start, nsteps, step=60.0, release=None, order=4, min_nodes=4, min_count=1, max_gap=None, every=1,
               visits=False):
    """`drift` by the library's host statement of the rule (`icelk_drift_host`): no GPU.  source: the dict of `combine_npzs`
    (u, v, count as (rows, cols, windows), x, y, time) or an open npz of it, or a (`TideFit`, cube or lattice) pair."""
    params = _params(step, nsteps, every, order, min_nodes)
    sx, sy, rel = _seeds(x, y, release)
    lib = _lib.load()
    if _is_pair(source):
        lattice = drift_lattice(source[1])
        cu, cv, status, B, m = _tide_tables(source[0], lattice, schedule_times(start, step, nsteps))

        def call(*args):
            return lib.icelk_drift_host(C.byref(lattice), C.byref(params), None, None, None, 0, None, None, None, None, 0.0, _f64(cu), _f64(cv),
                                        _i32(status), m, _f64(B), *args[:-1])
    else:
        if isinstance(source, VelocityCube) or not all(k in source for k in ("u", "v", "count", "x", "y", "time")):
            raise ValueError("source is a cube dict (u, v, count, x, y, time) or a (TideFit, cube or lattice) pair")
        lattice = drift_lattice(source)
        u, v, count = (np.asarray(source[k], np.float64) for k in ("u", "v", "count"))
        if u.ndim != 3 or v.shape != u.shape or count.shape != u.shape or u.shape[:2] != (lattice.rows, lattice.cols) or u.shape[2] == 0:
            raise ValueError("u, v, count must be (rows, cols, windows) arrays on the lattice of x, y")
        nt = u.shape[2]
        planes = [np.ascontiguousarray(np.moveaxis(a, 2, 0)) for a in (u, v, count)]
        S = drift_schedule(source["time"], start, step, nsteps, max_gap)
        if len(np.asarray(source["time"]).ravel()) != nt:
            raise ValueError("one time per window")

        def call(*args):
            return lib.icelk_drift_host(C.byref(lattice), C.byref(params), _f64(planes[0]), _f64(planes[1]), _f64(planes[2]), nt, _i32(S["k0"]),
                                        _i32(S["k1"]), _f64(S["a"]), _i32(S["flag"]), float(min_count), None, None, None, 0, None, *args[:-1])
    return _result(drift_arrays(call, None, lattice, params, sx, sy, rel, visits), start, params)

"""Tidal harmonics of the velocity cube, per cell.

The flow in a fjord is tidal and the cameras measure in daylight only, so the `nanmean` of a record with gaps
(`average_spatially_temporally`) folds the tide's phase into the "mean".  The standard tool is a least-squares fit, per cell,
of a mean plus a handful of tidal constituents (and perhaps a trend) to whatever samples exist.  It yields the tide-free
residual flow (`mean_u`, `mean_v`), the tidal ellipses (`TideFit.ellipse`) and a gap-free prediction (`TideFit.predict`).

The rule (csrc/tides.h; `fit_tides_host` is that text on the CPU, csrc/k_tides.hip the kernels, tests/tides_restatement.py a
restatement in numpy; the three agree bit for bit):
- the basis table B[nt][m] is made here on the host (`tide_basis`): a column of ones, cos and sin of every constituent, an
  optional trend.  The library never evaluates a sine;
- window t is a sample of a cell iff u and v are finite and count >= min_count; both components share their samples;
- normal equations summed in chunks of 256 windows, Cholesky with the pivot test s > 2^-30 * A[j][j], forward and back
  substitution; then a second pass for the residuals, rms = sqrt(ss_res / (n - m)) and explained = 1 - ss_res / ss_tot.
`status`: 0 fitted, 1 fewer than max(min_samples, m) samples, 2 rank deficient (coefficients, rms, explained NaN).

Declared differences from a tidal analysis package (t_tide, UTide): phases are relative to `t0`, not Greenwich; no nodal
corrections and no astronomical arguments; unweighted.  The pivot tolerance and the Rayleigh factor are policy, not
measurements.
"""
import ctypes as C

import numpy as np

from . import _lib

# speeds in degrees per hour
CONSTITUENTS = {
    "M2": 28.9841042, "S2": 30.0, "N2": 28.4397295, "K2": 30.0821373, "M4": 57.9682084, "M6": 86.9523127, "Mm": 0.5443747,
    "K1": 15.0410686, "O1": 13.9430356, "P1": 14.9589314, "Q1": 13.3986609, "MS4": 58.9841042, "Mf": 1.0980331,
}
MAX_TERMS = 18
TIDE_FITTED, TIDE_TOO_FEW, TIDE_RANK_DEFICIENT = 0, 1, 2
_PER_CELL = ("rms_u", "rms_v", "explained_u", "explained_v", "n", "first", "last", "status")


def constituent_table(constituents):
    """(names, speeds in degrees per hour) of a list of names of `CONSTITUENTS` and (name, degrees_per_hour) pairs"""
    names, speeds = [], []
    for c in constituents:
        if isinstance(c, str):
            if c not in CONSTITUENTS:
                raise ValueError("unknown constituent %r: give (name, degrees_per_hour)" % (c,))
            name, speed = c, CONSTITUENTS[c]
        else:
            name, speed = c
            name, speed = str(name), float(speed)
        if not (np.isfinite(speed) and speed > 0):
            raise ValueError("the speed of %s must be positive and finite" % name)
        if name in names:
            raise ValueError("constituent %s is named twice" % name)
        names.append(name)
        speeds.append(speed)
    return names, speeds


def _hours(time, t0):
    time = np.asarray(time, np.float64).ravel()
    if time.size == 0 or not np.all(np.isfinite(time)) or not np.isfinite(t0):
        raise ValueError("times must be finite, and one at least")
    return (time - float(t0)) / 3600.0


def trend_reference(time, t0):
    """(mid, span) in hours since t0 of a time axis: the trend column is (hours - mid) / span"""
    hours = _hours(time, t0)
    lo, hi = float(hours.min()), float(hours.max())
    return (lo + hi) / 2.0, hi - lo


def tide_basis(time, constituents, t0, trend=False, rayleigh=1.0, trend_ref=None):
    """The basis table, float64 (len(time), m): a column of ones, then np.cos and np.sin of deg2rad(speed) * (time - t0) /
    3600 per constituent (time, t0 in seconds), then with `trend` the column (hours - mid) / span -- of this time axis, or of
    `trend_ref` = (mid, span) when a fit is evaluated on another axis.  Non-finite times raise ValueError; so do two speeds
    that differ by less than `rayleigh` cycles over the span of `time` (the Rayleigh criterion; 0 switches the test off)."""
    names, speeds = constituent_table(constituents)
    hours = _hours(time, t0)
    m = 1 + 2 * len(names) + (1 if trend else 0)
    if m > MAX_TERMS:
        raise ValueError("more than %d terms" % MAX_TERMS)
    span = float(hours.max() - hours.min())
    if rayleigh > 0:
        for a in range(len(names)):
            for b in range(a + 1, len(names)):
                if abs(speeds[a] - speeds[b]) / 360.0 * span < rayleigh:
                    raise ValueError("%s and %s are %.3g cycles apart over %.1f hours: below the Rayleigh factor %g"
                                     % (names[a], names[b], abs(speeds[a] - speeds[b]) / 360.0 * span, span, rayleigh))
    B = np.ones((len(hours), m), np.float64)
    for k, speed in enumerate(speeds):
        arg = np.deg2rad(speed) * hours
        B[:, 1 + 2 * k] = np.cos(arg)
        B[:, 2 + 2 * k] = np.sin(arg)
    if trend:
        mid, tspan = trend_ref if trend_ref is not None else trend_reference(time, t0)
        if not (np.isfinite(mid) and np.isfinite(tspan) and tspan > 0):
            raise ValueError("a trend needs a time axis of positive span")
        B[:, m - 1] = (hours - mid) / tspan
    return B


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def _i32(a):
    return a.ctypes.data_as(_lib.i32p)


def _fit_call(call, handle, ncells, nt, basis, min_count, min_samples, residual, timing=None):
    """Allocate the outputs of one fit and run `call(basis, nt, m, min_count, min_samples, *outputs)`; a dict of flat arrays"""
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    if basis.ndim != 2 or basis.shape[0] != nt:
        raise ValueError("the basis must be (windows, terms)")
    m = basis.shape[1]
    min_samples = m if min_samples is None else int(min_samples)
    big = m > MAX_TERMS or m < 1                      # refused by the library; nothing this wide is allocated for it
    out = {k: np.zeros((ncells, 1 if big else m), np.float64) for k in ("coef_u", "coef_v")}
    out.update({k: np.zeros(ncells, np.float64 if k[0] in "re" else np.int32) for k in _PER_CELL})
    res = [np.zeros((nt, ncells), np.float64) for _ in range(2)] if residual else [None, None]
    device_ms = C.c_double(0.0)
    args = [_f64(basis), nt, m, float(min_count), min_samples, _f64(out["coef_u"]), _f64(out["coef_v"])]
    args += [_f64(out[k]) for k in _PER_CELL[:4]] + [_i32(out[k]) for k in _PER_CELL[4:]]
    args += [None if r is None else _f64(r) for r in res]
    rc = call(*args, C.byref(device_ms) if timing is not None else None)
    _lib.check(rc, handle)
    if timing is not None:
        timing.update(kernels_ms=device_ms.value)
    if residual:
        out["residual_u"], out["residual_v"] = res
    return out


def fit_arrays_host(u, v, count, basis, min_count=1, min_samples=None, residual=False):
    """`icelk_tide_fit_host` on arrays laid out [window][cell]: the host statement of the rule, no GPU.  Returns a dict of
    coef_u, coef_v (cells, m), rms_*, explained_*, n, first, last, status (cells) and, when asked, residual_u, residual_v
    (windows, cells)."""
    u, v, count = (np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, count))
    if u.ndim != 2 or v.shape != u.shape or count.shape != u.shape:
        raise ValueError("u, v, count must be (windows, cells) arrays of one shape")
    nt, ncells = u.shape
    lib = _lib.load()

    def call(b, nt_, m, min_count_, min_samples_, *outs):
        return lib.icelk_tide_fit_host(_f64(u), _f64(v), _f64(count), ncells, nt_, b, m, min_count_, min_samples_, *outs[:-1])
    return _fit_call(call, None, ncells, nt, basis, min_count, min_samples, residual)


def fit_arrays(cube, basis, min_count=1, min_samples=None, residual=False, timing=None):
    """`icelk_cube_tide_fit` on the resident cube with a basis of the caller's: the dict of `fit_arrays_host`"""
    ctx = cube.ctx

    def call(*args):
        return ctx._lib.icelk_cube_tide_fit(ctx._h, *args)
    return _fit_call(call, ctx._h, cube.rows * cube.cols, cube.nt, basis, min_count, min_samples, residual, timing)


def predict_arrays(ctx, coef_u, coef_v, status, basis):
    """`icelk_cube_tide_predict`: (out_u, out_v), each (len(basis), cells), from coefficients (cells, m) and status (cells)"""
    coef_u, coef_v = (np.ascontiguousarray(a, dtype=np.float64) for a in (coef_u, coef_v))
    status = np.ascontiguousarray(status, dtype=np.int32).ravel()
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    if coef_u.ndim != 2 or coef_v.shape != coef_u.shape or basis.ndim != 2 or basis.shape[1] != coef_u.shape[1] or len(status) != len(coef_u):
        raise ValueError("coefficients (cells, m), status (cells) and basis (times, m) do not fit together")
    ncells, m = coef_u.shape
    ntp = basis.shape[0]
    wide = m > MAX_TERMS or ncells * ntp >= 1 << 31   # refused by the library; nothing is allocated for the refusal
    out_u, out_v = (np.zeros((1, 1) if wide else (ntp, ncells), np.float64) for _ in range(2))
    rc = ctx._lib.icelk_cube_tide_predict(ctx._h, _f64(coef_u), _f64(coef_v), _i32(status), ncells, m, _f64(basis), ntp, _f64(out_u),
                                          _f64(out_v))
    _lib.check(rc, ctx._h)
    return out_u, out_v


class TideFit:
    """What a fit returns.  Fields, (rows, cols) unless said otherwise: mean_u, mean_v (the first coefficient: the tide-free
    flow), coef_u, coef_v (rows, cols, m), rms_u, rms_v, explained_u, explained_v, n, first, last, status, span_hours (from
    the first to the last sample; NaN without one), residual_u, residual_v ((rows, cols, nt), or None).  names, speeds: the
    constituents; t0 (seconds), trend, trend_ref: what `predict` rebuilds the basis from."""

    def __init__(self, fields, names, speeds, t0, trend, trend_ref, ctx=None):
        self.__dict__.update(fields)
        self.names, self.speeds = list(names), [float(s) for s in speeds]
        self.t0, self.trend, self.trend_ref = float(t0), bool(trend), trend_ref
        self.ctx = ctx
        self.mean_u, self.mean_v = self.coef_u[..., 0], self.coef_v[..., 0]

    def _cos_sin(self, name):
        k = self.names.index(name) if name in self.names else -1
        if k < 0:
            raise ValueError("%s was not fitted" % name)
        return 1 + 2 * k, 2 + 2 * k

    def amplitude(self, name):
        """(amplitude of u, of v) of a constituent"""
        a, b = self._cos_sin(name)
        return np.hypot(self.coef_u[..., a], self.coef_u[..., b]), np.hypot(self.coef_v[..., a], self.coef_v[..., b])

    def phase(self, name):
        """(phase of u, of v) in degrees, 0 .. 360, relative to t0: u = amplitude * cos(speed * (t - t0) - phase)"""
        a, b = self._cos_sin(name)
        return (np.rad2deg(np.arctan2(self.coef_u[..., b], self.coef_u[..., a])) % 360.0,
                np.rad2deg(np.arctan2(self.coef_v[..., b], self.coef_v[..., a])) % 360.0)

    def ellipse(self, name):
        """The tidal ellipse of a constituent by the rotary components of Pawlowicz, Beardsley & Lentz (2002): u + i v = a+
        exp(i w t) + a- exp(-i w t).  Returns (semi-major axis |a+| + |a-|, semi-minor axis |a+| - |a-| -- positive for
        counter-clockwise rotation --, inclination of the major axis in degrees counter-clockwise from +x, 0 .. 180, and phase
        in degrees, 0 .. 360: w (t - t0) at which the current points along the inclination)."""
        a, b = self._cos_sin(name)
        au, bu, av, bv = self.coef_u[..., a], self.coef_u[..., b], self.coef_v[..., a], self.coef_v[..., b]
        plus = 0.5 * ((au + bv) + 1j * (av - bu))
        minus = 0.5 * ((au - bv) + 1j * (av + bu))
        ep, em = np.angle(plus), np.angle(minus)
        inc = np.rad2deg((ep + em) / 2.0) % 360.0
        phase = np.rad2deg((em - ep) / 2.0)
        flip = inc >= 180.0
        inc = np.where(flip, inc - 180.0, inc)
        phase = np.where(flip, phase + 180.0, phase) % 360.0
        return np.abs(plus) + np.abs(minus), np.abs(plus) - np.abs(minus), inc, phase

    def basis(self, times):
        """the basis of this fit's terms on another time axis (seconds)"""
        return tide_basis(times, list(zip(self.names, self.speeds)), self.t0, self.trend, rayleigh=0, trend_ref=self.trend_ref)

    def predict(self, times, ctx=None):
        """(u, v), each (rows, cols, len(times)): the fitted mean, tide and trend at `times` (seconds), on the device; NaN in
        cells that were not fitted.  `ctx`: a Context, when the fit was loaded from a file or made on the host."""
        ctx = ctx if ctx is not None else self.ctx
        if ctx is None:
            raise ValueError("predict runs on the device: give a Context")
        rows, cols, m = self.coef_u.shape
        out_u, out_v = predict_arrays(ctx, self.coef_u.reshape(-1, m), self.coef_v.reshape(-1, m), self.status.ravel(), self.basis(times))
        return tuple(np.moveaxis(a.reshape(-1, rows, cols), 0, 2) for a in (out_u, out_v))

    def save(self, path):
        extra = {k: getattr(self, k) for k in ("residual_u", "residual_v") if getattr(self, k) is not None}
        np.savez(path, names=np.array(self.names), speeds=np.array(self.speeds), t0=self.t0, trend=self.trend,
                 trend_ref=np.array(self.trend_ref if self.trend_ref is not None else (np.nan, np.nan)),
                 coef_u=self.coef_u, coef_v=self.coef_v, span_hours=self.span_hours, **{k: getattr(self, k) for k in _PER_CELL}, **extra)


def load_tides(path, ctx=None):
    """A `TideFit` from the .npz that `TideFit.save` wrote"""
    with np.load(path) as z:
        fields = {k: z[k] for k in ("coef_u", "coef_v", "span_hours") + _PER_CELL}
        for k in ("residual_u", "residual_v"):
            fields[k] = z[k] if k in z.files else None
        trend = bool(z["trend"])
        return TideFit(fields, [str(s) for s in z["names"]], z["speeds"], float(z["t0"]), trend,
                       tuple(float(q) for q in z["trend_ref"]) if trend else None, ctx)


def _tide_fit(run, rows, cols, time, constituents, t0, trend, min_count, min_samples, residual, rayleigh, ctx):
    time = np.asarray(time, np.float64).ravel()
    names, speeds = constituent_table(constituents)
    if time.size == 0 or not np.all(np.isfinite(time)):
        raise ValueError("times must be finite, and one at least")
    t0 = float(time.min()) if t0 is None else float(t0)
    ref = trend_reference(time, t0) if trend else None
    B = tide_basis(time, list(zip(names, speeds)), t0, trend, rayleigh)
    flat = run(B)
    m, nt = B.shape[1], len(time)
    fields = {k: flat[k].reshape(rows, cols) for k in _PER_CELL}
    fields.update(coef_u=flat["coef_u"].reshape(rows, cols, m), coef_v=flat["coef_v"].reshape(rows, cols, m))
    for k in ("residual_u", "residual_v"):
        fields[k] = np.moveaxis(flat[k].reshape(nt, rows, cols), 0, 2) if residual else None
    have = fields["n"] > 0
    first, last = np.where(have, fields["first"], 0), np.where(have, fields["last"], 0)
    fields["span_hours"] = np.where(have, (time[last] - time[first]) / 3600.0, np.nan)
    return TideFit(fields, names, speeds, t0, trend, ref, ctx)


def fit_tides(cube, constituents=("M2", "S2", "K1", "O1"), t0=None, trend=False, min_count=1, min_samples=None, residual=False,
              timing=None, rayleigh=1.0):
    """Fit a mean, the constituents and (with `trend`) a linear trend to every cell of a `VelocityCube`, on the device
    (`icelk_cube_tide_fit`).  constituents: names of `CONSTITUENTS` or (name, degrees_per_hour); t0: the phase reference in
    epoch seconds (None: the cube's earliest time); min_count: a window is a sample of a cell iff u, v are finite and count
    >= min_count; min_samples: a cell with fewer samples is not fitted (None: the number of terms); residual: also return
    the residual cube; timing: a dict that receives the kernels' milliseconds.  Returns a `TideFit`.  The cube is not
    changed."""
    def run(B):
        return fit_arrays(cube, B, min_count, min_samples, residual, timing)
    return _tide_fit(run, cube.rows, cube.cols, cube.time, constituents, t0, trend, min_count, min_samples, residual, rayleigh, cube.ctx)


def fit_tides_host(cube, constituents=("M2", "S2", "K1", "O1"), t0=None, trend=False, min_count=1, min_samples=None,
                   residual=False, rayleigh=1.0):
    """`fit_tides` by the library's host statement of the rule (`icelk_tide_fit_host`): no GPU.  cube: the dict of
    `combine_npzs` (u, v, count as (rows, cols, windows), time) or an open npz of it."""
    u, v, count = (np.asarray(cube[k], np.float64) for k in ("u", "v", "count"))
    if u.ndim != 3 or v.shape != u.shape or count.shape != u.shape or u.size == 0:
        raise ValueError("u, v, count must be (rows, cols, windows) arrays of one shape")
    rows, cols, nt = u.shape
    planes = [np.ascontiguousarray(np.moveaxis(a, 2, 0)).reshape(nt, rows * cols) for a in (u, v, count)]

    def run(B):
        return fit_arrays_host(planes[0], planes[1], planes[2], B, min_count, min_samples, residual)
    return _tide_fit(run, rows, cols, cube["time"], constituents, t0, trend, min_count, min_samples, residual, rayleigh, None)

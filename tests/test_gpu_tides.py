"""GPU: the per-cell harmonic fit of the velocity cube (csrc/k_tides.hip, icelk_cube_tide_fit, icelk_cube_tide_predict).

- the device fit equals the host statement (`fit_arrays_host`, csrc/tides.h on the CPU) bit for bit on every output over the
  catalogue (tests/tides_cases.py), the residual cubes included -- no tolerance anywhere;
- `predict` equals the host's sum, term by term in the rule's order, at the fitted times and on a second, different time axis;
  cells that were not fitted give NaN;
- fitting twice gives identical bytes;
- the cube's averages are unchanged by a fit;
- the refusals, which leave the handle usable."""
import datetime as dt

import numpy as np
import pytest

import tides_cases as TC
from iceberg_tracking_code_amd import VelocityCube, _lib, average_periods, fit_tides, fit_tides_host, tides
from iceberg_tracking_code_amd.day_grid import EPOCH
from tides_restatement import RESULT_KEYS, same_bits

pytestmark = pytest.mark.gpu

CASES = TC.catalogue()


def cube_dict(case, rows=1):
    """the case's [window][cell] arrays as the (rows, cols, windows) dict a VelocityCube takes"""
    nt, nc = case["u"].shape
    back = lambda a: np.moveaxis(a.reshape(nt, rows, nc // rows), 0, 2)           # noqa: E731
    time = case["info"].get("time", TC.T0 + 1800.0 * np.arange(nt))
    return dict(u=back(case["u"]), v=back(case["v"]), count=back(case["count"]), x=np.zeros((rows, nc // rows)), y=np.zeros((rows, nc // rows)),
                time=time)


def host_sum(coef, status, basis):
    """(times, cells): coef[cell][0] * basis[t][0] + coef[cell][1] * basis[t][1] + ..., NaN where status != 0"""
    out = coef[:, 0][None, :] * basis[:, 0][:, None]
    for j in range(1, basis.shape[1]):
        out = out + coef[:, j][None, :] * basis[:, j][:, None]
    out[:, status != 0] = np.nan
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_host(ctx, case):
    args, kw = TC.call_args(case)
    want = tides.fit_arrays_host(*args, **kw)
    with VelocityCube(cube_dict(case), ctx) as cube:
        timing = {}
        got = tides.fit_arrays(cube, case["basis"], timing=timing, **kw)
        assert same_bits(got, want) is None
        assert timing["kernels_ms"] > 0
        kw["residual"] = False
        plain = tides.fit_arrays(cube, case["basis"], **kw)
        assert same_bits(plain, want, keys=[k for k in RESULT_KEYS if not k.startswith("residual")]) is None
    for cell, status in case["info"].get("status", {}).items():
        assert got["status"][cell] == status


@pytest.mark.parametrize("name", ["planted_30d", "specials", "shape_257x255x3", "shape_64x257x18"])
def test_predict_equals_the_hosts_sum(ctx, name):
    case = TC.case(name)
    args, kw = TC.call_args(case)
    fit = tides.fit_arrays_host(*args, **kw)
    nt, m = case["basis"].shape
    other = np.random.default_rng(5).normal(size=(513 if nt != 513 else 300, m))      # another length: other chunk edges
    for basis in (case["basis"], other):
        got_u, got_v = tides.predict_arrays(ctx, fit["coef_u"], fit["coef_v"], fit["status"], basis)
        for got, coef in ((got_u, fit["coef_u"]), (got_v, fit["coef_v"])):
            want = host_sum(coef, fit["status"], basis)
            assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
            assert got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes()
    if name == "specials":
        assert np.isnan(got_u[:, 0]).all() and np.isfinite(got_u[:, 5]).all()


def test_fit_tides_predict_twice_and_averages(ctx):
    case = TC.case("planted_15d")
    d = cube_dict(case, rows=2)
    constituents = case["info"]["constituents"]
    day = EPOCH + dt.timedelta(seconds=TC.T0)
    periods = [(day + dt.timedelta(days=k, hours=12), day + dt.timedelta(days=k, hours=34)) for k in range(3)]
    with VelocityCube(d, ctx) as cube:
        before = average_periods(cube, periods)
        fit = fit_tides(cube, constituents, residual=True)
        again = fit_tides(cube, constituents, residual=True)
        after = average_periods(cube, periods)
    host = fit_tides_host(d, constituents, residual=True)
    for k in ("coef_u", "coef_v", "rms_u", "rms_v", "explained_u", "explained_v", "n", "first", "last", "status", "span_hours", "residual_u",
              "residual_v", "mean_u", "mean_v"):
        a, b, h = getattr(fit, k), getattr(again, k), getattr(host, k)
        assert a.tobytes() == b.tobytes(), k                                       # twice: identical bytes
        assert a.shape == h.shape and np.array_equal(a, h, equal_nan=True), k      # and the host's values
    assert fit.coef_u.shape == (2, 2, 9) and fit.residual_u.shape == (2, 2, len(d["time"])) and np.all(fit.status == 0)
    assert np.abs(fit.mean_u - 0.05).max() < 0.01
    for p, q in zip(before, after):
        for k in ("u", "v", "speed", "count"):
            assert p[k].tobytes() == q[k].tobytes(), k
    # predict: at the fitted times and on an hourly axis that starts before the record and ends after it
    for times in (d["time"], TC.T0 - 86400.0 + 3600.0 * np.arange(17 * 24 + 5)):
        u, v = fit.predict(times)
        assert u.shape == (2, 2, len(times))
        B = fit.basis(times)
        for got, coef in ((u, fit.coef_u), (v, fit.coef_v)):
            want = host_sum(coef.reshape(4, -1), fit.status.ravel(), B)
            assert np.moveaxis(got, 2, 0).reshape(len(times), 4).tobytes() == want.tobytes()
    # the residual is what is left of a sample after the prediction
    u, _ = fit.predict(d["time"])
    lit = np.isfinite(d["u"])
    assert np.array_equal(np.isfinite(fit.residual_u), lit) and np.abs((d["u"] - u)[lit] - fit.residual_u[lit]).max() == 0.0


def test_refusals(ctx):
    lib, h = ctx._lib, ctx._h
    nc, nt, m = 6, 40, 3
    basis = np.ones((nt, 19))
    f = lambda q: q.ctypes.data_as(_lib.f64p)                                     # noqa: E731
    outs = [np.zeros(nc * 19) for _ in range(6)]
    ints = [np.zeros(nc, np.int32) for _ in range(4)]
    field = [np.zeros(nt * nc) for _ in range(2)]

    def fit(b=basis, windows=nt, terms=m, min_samples=0, drop=None):
        o = [f(q) for q in outs] + [q.ctypes.data_as(_lib.i32p) for q in ints]
        if drop is not None:
            o[drop] = None
        return lib.icelk_cube_tide_fit(h, None if b is None else f(b), windows, terms, 1.0, min_samples, *o, None, None, None)

    def predict(ncells=nc, terms=m, times=nt, drop=None):
        a = [f(outs[0]), f(outs[1]), ints[0].ctypes.data_as(_lib.i32p), ncells, terms, f(basis), times, f(field[0]), f(field[1])]
        if drop is not None:
            a[drop] = None
        return lib.icelk_cube_tide_predict(h, *a)
    assert getattr(ctx, "_cube", None) is None
    assert fit() == _lib.ESTATE                                                   # no cube
    assert lib.icelk_cube_tide_fit(None, f(basis), nt, m, 1.0, 0, *[None] * 13) == _lib.EARG
    case = dict(u=np.zeros((nt, nc)), v=np.zeros((nt, nc)), count=np.ones((nt, nc)), info={})
    with VelocityCube(cube_dict(case), ctx) as cube:
        assert fit() == _lib.OK
        assert fit(b=None) == _lib.EARG
        for k in range(10):
            assert fit(drop=k) == _lib.EARG, k
        assert fit(windows=nt - 1) == _lib.EARG and fit(windows=nt + 1) == _lib.EARG
        assert fit(terms=0) == _lib.EARG and fit(min_samples=-1) == _lib.EARG
        assert fit(terms=18) == _lib.OK and fit(terms=19) == _lib.ECAP
        with pytest.raises(_lib.IcelkError):
            tides.fit_arrays(cube, basis)                                         # 19 terms, through the Python layer
        with pytest.raises(ValueError):
            tides.fit_arrays(cube, basis[:5, :3])
        assert fit() == _lib.OK                                                   # the handle is still usable
    # a workspace of chunk partials beyond 31 bits: 209 sums x 1 chunk x 2^24 cells, on a cube that itself fits
    wide = dict(u=np.zeros((1, 1 << 24)), v=np.zeros((1, 1 << 24)), count=np.zeros((1, 1 << 24)), info={})
    with VelocityCube(cube_dict(wide), ctx):
        assert fit(windows=1, terms=18) == _lib.ECAP
        assert b"31 bits" in lib.icelk_last_error(h)
    assert predict() == _lib.OK                                                   # needs no cube
    for k in (0, 1, 2, 5, 7, 8):
        assert predict(drop=k) == _lib.EARG, k
    assert predict(ncells=0) == _lib.EARG and predict(terms=0) == _lib.EARG and predict(times=0) == _lib.EARG
    assert predict(terms=19) == _lib.ECAP
    assert predict(ncells=1 << 16, times=1 << 15) == _lib.ECAP                    # cells x times = 2^31, refused before any copy
    assert predict() == _lib.OK

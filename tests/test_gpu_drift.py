"""GPU: virtual drifters through the gridded velocities (csrc/k_drift.hip, icelk_cube_drift, icelk_drift_tide).

- the device equals the host statement (`icelk_drift_host`, csrc/drift.h on the CPU) bit for bit on every output over the
  catalogue (tests/drift_cases.py), both sources, the visits included -- no tolerance anywhere;
- `drift` twice on one cube gives identical bytes, equals `drift_host`, and leaves the cube's averages unchanged;
- the tide source through the Python layer, on a fit's own context;
- the refusals, which leave the handle usable; `timing` is filled."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

import drift_cases as DC
from drift_restatement import RESULT_KEYS, same_bits
from iceberg_tracking_code_amd import DriftResult, VelocityCube, _lib, average_periods, drift, drift_host, fit_tides, seed_nodes
from iceberg_tracking_code_amd.day_grid import EPOCH

pytestmark = pytest.mark.gpu

CASES = DC.catalogue()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_host(ctx, case):
    want = DC.run(case)
    timing = {}
    if case["source"] == "cube":
        with VelocityCube(DC.cube_dict(case), ctx):
            got = DC.run(case, ctx, timing)
            plain = DC.run(case, ctx, visits=False)
    else:
        got = DC.run(case, ctx, timing)
        plain = DC.run(case, ctx, visits=False)
    assert same_bits(got, want) is None
    assert plain["visits"] is None and same_bits(plain, want, keys=RESULT_KEYS[:-1]) is None
    assert timing["kernels_ms"] > 0
    for p, status in enumerate(case["info"].get("status", [])):
        assert got["status"][p] == status


def test_drift_twice_and_averages(ctx):
    c = DC.case("shape_33x65x257_n257_s97_e1_o4")
    d = DC.cube_dict(c)
    day = EPOCH + dt.timedelta(seconds=DC.T0)
    periods = [(day + dt.timedelta(hours=k), day + dt.timedelta(hours=k + 30)) for k in (0, 24, 48)]
    kw = dict(start=c["start"], nsteps=97, step=60.0, release=c["release"], order=4, min_nodes=4, every=1, visits=True)
    with VelocityCube(d, ctx) as cube:
        before = average_periods(cube, periods)
        timing = {}
        a = drift(cube, c["x"], c["y"], timing=timing, **kw)
        b = drift(cube, c["x"], c["y"], **kw)
        after = average_periods(cube, periods)
        fit = fit_tides(cube, ("M2",), min_samples=20)
        sx, sy = seed_nodes(cube, stride=4, measured_in=fit)
        tkw = dict(start=DC.T0 - 7200.0, nsteps=50, step=-600.0, order=2, min_nodes=3, every=7, visits=True)
        tide = drift((fit, cube), sx, sy, **tkw)                              # on the fit's context, at times the cube has no window for
    assert timing["kernels_ms"] > 0
    host = drift_host(d, c["x"], c["y"], **kw)
    for k in DriftResult.FIELDS + ("visits",):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k           # twice: identical bytes
        assert getattr(a, k).shape == getattr(host, k).shape and np.array_equal(getattr(a, k), getattr(host, k), equal_nan=True), k
    assert same_bits(a.__dict__, DC.expected(c)) is None
    for p, q in zip(before, after):
        for k in ("u", "v", "speed", "count"):
            assert p[k].tobytes() == q[k].tobytes(), k
    tide_host = drift_host((fit, d), sx, sy, **tkw)
    assert len(sx) > 50 and np.any(tide.status == 0)
    for k in DriftResult.FIELDS + ("visits",):
        assert np.array_equal(getattr(tide, k), getattr(tide_host, k), equal_nan=True), k


def test_tide_source_equals_a_cube_of_predict(ctx):
    """A cube made of `TideFit.predict` (the device's) at its own window times, Euler, a step of one window: row 2s is an exact hit,
    (1 - 0) u + 0 u = u, and the two sources see the same numbers -- the same positions bit for bit, on the device and the host."""
    c = DC.case("shape_33x65x257_n257_s97_e1_o4")
    d = DC.cube_dict(c)
    with VelocityCube(d, ctx) as cube:
        fit = fit_tides(cube, ("M2", "K1"), min_samples=225)                   # some cells hold fewer samples: status 1
        u, v = fit.predict(cube.time)
    assert set(np.unique(fit.status)) == {0, 1} and np.array_equal(np.isnan(u[:, :, 0]), fit.status != 0)
    made = dict(d, u=u, v=v, count=np.ones_like(u))
    sx, sy = seed_nodes(made, stride=2)
    kw = dict(start=d["time"][0], nsteps=len(d["time"]) - 1, step=DC.WINDOW, order=1, min_nodes=2, every=4, visits=True)
    with VelocityCube(made, ctx) as cube:
        a, b = drift(cube, sx + 50.0, sy - 50.0, **kw), drift((fit, cube), sx + 50.0, sy - 50.0, **kw)
    h = drift_host((fit, made), sx + 50.0, sy - 50.0, **kw)
    for k in DriftResult.FIELDS + ("visits",):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
        assert np.array_equal(getattr(a, k), getattr(h, k), equal_nan=True), k
    assert len(np.unique(a.status)) > 1 and a.length.max() > 1000.0


def test_refusals(ctx):
    lib, h = ctx._lib, ctx._h
    c = DC.case("shape_3x5x3_n65_s97_e3_o4")
    t = DC.case("tide_3x5_m5_n64_s2_o4")
    f = lambda q: q.ctypes.data_as(_lib.f64p)                                      # noqa: E731
    i = lambda q: q.ctypes.data_as(_lib.i32p)                                      # noqa: E731
    n = len(c["x"])
    bufs = {k: np.zeros((97 // 3 + 1) * n if k in "xy" else n) for k in ("x", "y", "last_x", "last_y", "length")}
    ints = {k: np.zeros(n, np.int32) for k in ("status", "stop_step")}

    def out(drop=None):
        o = [f(bufs[k]) for k in ("x", "y", "last_x", "last_y", "length")] + [i(ints["status"]), i(ints["stop_step"]), None]
        if drop is not None:
            o[drop] = None
        return _lib.DriftOut(*o)

    def cube_call(lattice=c["lattice"], params=c["params"], count=n, drop=None, drop_out=None, k0=c["k0"]):
        a = [C.byref(_lib.DriftLattice(*lattice)), C.byref(_lib.DriftParams(*params)), i(k0), i(c["k1"]), f(c["a"]), i(c["flag"]), 1.0, f(c["x"]),
             f(c["y"]), i(c["release"]), count, C.byref(out(drop_out)), None]
        if drop is not None:
            a[drop] = None
        return lib.icelk_cube_drift(h, *a)

    def tide_call(lattice=t["lattice"], params=t["params"], m=5, count=64, drop=None):
        a = [C.byref(_lib.DriftLattice(*lattice)), C.byref(_lib.DriftParams(*params)), f(t["coef_u"]), f(t["coef_v"]), i(t["status"]), m, f(t["basis"]),
             f(t["x"]), f(t["y"]), i(t["release"]), count, C.byref(out()), None]
        if drop is not None:
            a[drop] = None
        return lib.icelk_drift_tide(h, *a)
    step, nsteps, every, order, min_nodes = c["params"]
    x0, y0, dx, dy, rows, cols = c["lattice"]
    assert getattr(ctx, "_cube", None) is None
    assert cube_call() == _lib.ESTATE                                              # no cube
    assert b"icelk_cube_set" in lib.icelk_last_error(h)
    assert lib.icelk_cube_drift(None, *[None] * 6, 1.0, *[None] * 3, n, None, None) == _lib.EARG
    with VelocityCube(DC.cube_dict(c), ctx):
        assert cube_call() == _lib.OK
        for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 11):
            assert cube_call(drop=k) == _lib.EARG, k
        for k in range(7):
            assert cube_call(drop_out=k) == _lib.EARG, k
        for params in ((0.0, nsteps, every, order, min_nodes), (np.nan, nsteps, every, order, min_nodes), (np.inf, nsteps, every, order, min_nodes),
                       (step, 0, every, order, min_nodes), (step, nsteps, 0, order, min_nodes), (step, nsteps, every, 3, min_nodes),
                       (step, nsteps, every, 0, min_nodes), (step, nsteps, every, order, 0), (step, nsteps, every, order, 5)):
            assert cube_call(params=params) == _lib.EARG, params
        assert cube_call(count=0) == _lib.EARG
        assert cube_call(lattice=(x0, y0, dx, dy, cols, rows)) == _lib.OK          # as many nodes: the library cannot tell
        assert cube_call(lattice=(x0, y0, dx, dy, rows, cols + 1)) == _lib.EARG    # not the cube's cells
        assert cube_call(lattice=(x0, y0, 0.0, dy, rows, cols)) == _lib.EARG
        assert cube_call(lattice=(x0, np.nan, dx, dy, rows, cols)) == _lib.EARG
        for bad in (-1, 3):                                                        # a window outside the cube of 3, in the last row
            k0 = c["k0"].copy()
            k0[-1] = bad
            assert cube_call(k0=k0) == _lib.EARG
        assert b"outside the cube" in lib.icelk_last_error(h)
        assert cube_call(params=(step, 1023, 1, order, min_nodes), count=1 << 21) == _lib.ECAP   # n * n_out = 2^31, before any copy
        assert b"31 bits" in lib.icelk_last_error(h)
        assert cube_call() == _lib.OK                                              # the handle is still usable
    assert tide_call() == _lib.OK                                                  # needs no cube
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 11):
        assert tide_call(drop=k) == _lib.EARG, k
    assert tide_call(m=0) == _lib.EARG and tide_call(m=19) == _lib.ECAP
    assert tide_call(lattice=(x0, y0, dx, dy, 1, 15)) == _lib.EARG
    assert tide_call(params=(60.0, 0x3fffffff, 1 << 20, 4, 3)) == _lib.ECAP        # (2^31 - 1) schedule rows x 5 terms
    assert tide_call(params=(60.0, 2, 3, 4, 9)) == _lib.EARG
    assert tide_call() == _lib.OK

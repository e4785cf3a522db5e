"""CPU: the per-cell harmonic fit's host statement (csrc/tides.h through icelk_tide_fit_host) and the Python layer
(iceberg_tracking_code_amd/tides.py).  No GPU.

- `fit_arrays_host` equals the numpy restatement (tests/tides_restatement.py) bit for bit on every output over the whole
  catalogue (tests/tides_cases.py), NaNs comparing as NaN; the statuses the catalogue plants are met;
- each planted case is held to np.linalg.lstsq on the same samples within n * m * eps * cond(B)^2 * max|c| -- the forward
  error bound of normal equations with sequential sums, cond from np.linalg.cond on the samples' rows;
- a planted ellipse (axes, inclination, phase, both senses of rotation) is recovered by `ellipse()` to the same bound;
- the nanmean of the planted daylight record misses the planted mean by more than the fit does: the reason for the feature;
- the Rayleigh test, the basis of hand-computed small cases, save / load, and the argument checks of the host call."""
import ctypes as C

import numpy as np
import pytest

import tides_cases as TC
from iceberg_tracking_code_amd import _lib, fit_tides_host, load_tides, tide_basis, tides
from tides_restatement import same_bits

CASES = TC.catalogue()
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_restatement(case):
    args, kw = TC.call_args(case)
    got, want = tides.fit_arrays_host(*args, **kw), TC.expected(case)
    assert same_bits(got, want) is None
    for cell, status in case["info"].get("status", {}).items():
        assert got["status"][cell] == status, cell
    for cell in case["info"].get("rms_nan", []):
        assert np.isnan(got["rms_u"][cell]) and np.isnan(got["rms_v"][cell]) and np.all(np.isfinite(got["coef_u"][cell]))
    bad = got["status"] != 0
    assert np.all(np.isnan(got["coef_u"][bad])) and np.all(np.isnan(got["rms_v"][bad])) and np.all(np.isnan(got["residual_u"][:, bad]))
    # without the residual cubes: the same results
    kw["residual"] = False
    assert same_bits(tides.fit_arrays_host(*args, **kw), want, keys=[k for k in want if not k.startswith("residual")]) is None


def test_catalogue_covers_what_it_names():
    cells = {c["u"].shape[1] for c in CASES}
    windows = {c["u"].shape[0] for c in CASES}
    terms = {c["basis"].shape[1] for c in CASES}
    assert {1, 63, 64, 65, 257} <= cells and {1, 255, 256, 257, 513} <= windows and {1, 3, 17, 18} <= terms
    for m in (3, 17, 18):
        assert {m - 1, m, m + 1} <= {c["u"].shape[0] for c in CASES if c["basis"].shape[1] == m}
    statuses = set()
    for c in CASES:
        statuses |= set(TC.expected(c)["status"].tolist())
    assert statuses == {0, 1, 2}


def lstsq_bound(case, cell):
    """(lstsq coefficients of u and v on the cell's samples, the bound n * m * eps * cond^2 * max|c|)"""
    take = np.isfinite(case["u"][:, cell]) & np.isfinite(case["v"][:, cell])
    B = case["basis"][take]
    cu = np.linalg.lstsq(B, case["u"][take, cell], rcond=None)[0]
    cv = np.linalg.lstsq(B, case["v"][take, cell], rcond=None)[0]
    n, m = B.shape
    return cu, cv, n * m * EPS * np.linalg.cond(B) ** 2 * max(np.abs(cu).max(), np.abs(cv).max())


@pytest.mark.parametrize("name", [p[0] for p in TC.PLANTED])
def test_planted_signal_against_lstsq(name):
    case = TC.case(name)
    args, kw = TC.call_args(case)
    got = tides.fit_arrays_host(*args, **kw)
    assert np.all(got["status"] == 0)
    for cell in range(TC.PLANTED_CELLS):
        cu, cv, bound = lstsq_bound(case, cell)
        err = max(np.abs(got["coef_u"][cell] - cu).max(), np.abs(got["coef_v"][cell] - cv).max())
        print("%s cell %d: error %.3g, bound %.3g" % (name, cell, err, bound))
        assert err <= bound
    # the noise-free cell holds what was planted, to the same bound
    cu, cv, bound = lstsq_bound(case, 0)
    assert np.abs(got["coef_u"][0] - case["info"]["truth_u"][0]).max() <= bound
    assert np.abs(got["coef_v"][0] - case["info"]["truth_v"][0]).max() <= bound
    assert got["explained_u"][0] > 1 - 1e-12 and np.all(got["explained_u"][1:] < 1) and np.all(got["explained_u"][1:] > 0.5)
    assert np.all(np.abs(got["rms_u"][1:] - 0.02) < 0.005) and got["rms_u"][0] < 1e-12


def ellipse_cube(days, params):
    """(rows 1, cols len(params)) cube of planted M2 ellipses (major, minor, inclination, phase in degrees), daylight only"""
    time = TC.planted_time(days)
    arg = np.deg2rad(tides.CONSTITUENTS["M2"]) * (time - TC.T0) / 3600.0
    u, v = np.empty((1, len(params), len(time))), np.empty((1, len(params), len(time)))
    for k, (major, minor, inc, phase) in enumerate(params):
        along, across = major * np.cos(arg - np.deg2rad(phase)), minor * np.sin(arg - np.deg2rad(phase))
        u[0, k] = 0.05 + along * np.cos(np.deg2rad(inc)) - across * np.sin(np.deg2rad(inc))
        v[0, k] = -0.02 + along * np.sin(np.deg2rad(inc)) + across * np.cos(np.deg2rad(inc))
    night = ~TC.daylight(time)
    u[..., night], v[..., night] = np.nan, np.nan
    return dict(u=u, v=v, count=np.ones_like(u), time=time)


def test_planted_ellipse_is_recovered():
    params = [(0.30, 0.10, 30.0, 40.0), (0.30, -0.10, 30.0, 40.0), (0.20, 0.05, 135.0, 300.0), (0.25, -0.20, 5.0, 170.0)]
    cube = ellipse_cube(3, params)
    fit = fit_tides_host(cube, ("M2", "K1"), t0=TC.T0)
    assert fit.mean_u.shape == (1, len(params)) and fit.coef_u.shape == (1, len(params), 5) and np.all(fit.status == 0)
    take = TC.daylight(cube["time"])
    B = tide_basis(cube["time"], ("M2", "K1"), TC.T0)[take]
    bound = B.shape[0] * B.shape[1] * EPS * np.linalg.cond(B) ** 2 * 0.3
    major, minor, inc, phase = fit.ellipse("M2")
    for k, (M, mi, th, g) in enumerate(params):
        assert abs(major[0, k] - M) <= 2 * bound and abs(minor[0, k] - mi) <= 2 * bound       # two rotary amplitudes each
        # an angle moves by at most error / amplitude radians; the smaller rotary amplitude is (M - |mi|) / 2
        angle_bound = np.rad2deg(2 * bound / ((M - abs(mi)) / 2))
        assert abs(inc[0, k] - th) <= angle_bound and abs(phase[0, k] - g) <= angle_bound
    assert np.abs(fit.mean_u - 0.05).max() <= bound and np.abs(fit.mean_v + 0.02).max() <= bound
    au, av = fit.amplitude("K1")
    assert au.max() <= 2 * bound and av.max() <= 2 * bound                      # hypot of two coefficients
    pu, _ = fit.phase("M2")
    assert pu.shape == (1, len(params)) and np.all((pu >= 0) & (pu < 360))


def test_nanmean_misses_the_mean_the_fit_finds():
    """the reason for the feature: M2 of 0.3 m/s on a mean of 0.05 m/s, seen in daylight only"""
    case = TC.case("planted_3d")
    u = case["u"][:, 0]
    args, kw = TC.call_args(case)
    fitted = tides.fit_arrays_host(*args, **kw)["coef_u"][0, 0]
    day_means = [np.nanmean(u[48 * d:48 * (d + 1)]) for d in range(3)]
    print("daily nanmean", day_means, "record nanmean", np.nanmean(u), "fit", fitted)
    assert abs(fitted - 0.05) < 1e-12
    assert abs(np.nanmean(u) - 0.05) > abs(fitted - 0.05)
    assert all(abs(q - 0.05) > 1e3 * abs(fitted - 0.05) for q in day_means)


def test_basis_by_hand():
    time = np.array([0.0, 3600.0, 7200.0, 10800.0])
    B = tide_basis(time, (("S2", 30.0),), 0.0, rayleigh=0)
    want = np.array([[1, 1, 0], [1, np.cos(np.deg2rad(30.0) * 1.0), np.sin(np.deg2rad(30.0) * 1.0)],
                     [1, np.cos(np.deg2rad(30.0) * 2.0), np.sin(np.deg2rad(30.0) * 2.0)],
                     [1, np.cos(np.deg2rad(30.0) * 3.0), np.sin(np.deg2rad(30.0) * 3.0)]])
    assert B.tobytes() == want.astype(np.float64).tobytes()
    assert abs(B[3, 1]) < 1e-15 and abs(B[3, 2] - 1) < 1e-15
    T = tide_basis(time, ("S2",), 3600.0, trend=True, rayleigh=0)
    assert T.shape == (4, 4) and T[1, 1] == 1.0 and T[1, 2] == 0.0
    assert T[:, 3].tolist() == [-0.5, (0.0 - 0.5) / 3.0, (1.0 - 0.5) / 3.0, 0.5]
    assert tide_basis(time[:2], ("S2",), 0.0, trend=True, rayleigh=0, trend_ref=(0.5, 3.0))[:, 3].tolist() == [-0.5 / 3.0, 0.5 / 3.0]
    assert tide_basis(time, (), 0.0).tolist() == [[1.0]] * 4
    assert tides.CONSTITUENTS["M2"] == 28.9841042 and tides.CONSTITUENTS["MS4"] == 58.9841042 and len(tides.CONSTITUENTS) == 13
    for bad in (np.array([0.0, np.nan]), np.array([0.0, np.inf]), np.array([])):
        with pytest.raises(ValueError):
            tide_basis(bad, ("M2",), 0.0)
    with pytest.raises(ValueError):
        tide_basis(time, ("XX",), 0.0)
    with pytest.raises(ValueError):
        tide_basis(time, ("M2", "M2"), 0.0, rayleigh=0)
    with pytest.raises(ValueError):
        tide_basis(time[:1], ("M2",), 0.0, trend=True)
    with pytest.raises(ValueError):
        tide_basis(time, tuple(("c%d" % k, 10.0 + k) for k in range(9)), 0.0, rayleigh=0)      # 19 terms


def test_rayleigh():
    hours = lambda h: 3600.0 * np.arange(0.0, h + 0.5, 0.5)                      # noqa: E731
    # M2 and S2 are 1.0158958 degrees per hour apart: one cycle apart after 354.4 hours
    with pytest.raises(ValueError, match="Rayleigh"):
        tide_basis(hours(354.0), ("M2", "S2"), 0.0)
    assert tide_basis(hours(354.5), ("M2", "S2"), 0.0).shape == (710, 5)
    assert tide_basis(hours(354.0), ("M2", "S2"), 0.0, rayleigh=0).shape == (709, 5)
    assert tide_basis(hours(354.0), ("M2", "S2"), 0.0, rayleigh=0.9).shape == (709, 5)
    with pytest.raises(ValueError, match="Rayleigh"):
        tide_basis(hours(354.5), ("M2", "S2"), 0.0, rayleigh=1.1)
    with pytest.raises(ValueError, match="Rayleigh"):
        tide_basis(hours(24 * 30), ("S2", "K2"), 0.0)
    for name, days, constituents, trend in TC.PLANTED:                             # none of the planted cases trips it
        tide_basis(TC.planted_time(days), constituents, TC.T0, trend)


def test_fit_tides_host_fields_and_files(tmp_path):
    case = TC.case("planted_15d")
    nt, nc = case["u"].shape
    to_cube = lambda a: np.moveaxis(a.reshape(nt, 2, 2), 0, 2)                    # noqa: E731
    cube = dict(u=to_cube(case["u"]), v=to_cube(case["v"]), count=to_cube(case["count"]), time=case["info"]["time"])
    fit = fit_tides_host(cube, case["info"]["constituents"], residual=True)
    flat = TC.expected(case)
    assert fit.t0 == TC.T0 and fit.names == list(case["info"]["constituents"]) and not fit.trend
    assert fit.coef_u.reshape(nc, -1).tobytes() == flat["coef_u"].tobytes() and fit.mean_v.ravel().tobytes() == flat["coef_v"][:, 0].tobytes()
    assert fit.n.shape == (2, 2) and fit.n.ravel().tolist() == flat["n"].tolist()
    assert fit.residual_u.shape == (2, 2, nt)
    assert np.array_equal(np.moveaxis(fit.residual_u, 2, 0).reshape(nt, nc), flat["residual_u"], equal_nan=True)
    time = case["info"]["time"]
    assert np.array_equal(fit.span_hours.ravel(), (time[flat["last"]] - time[flat["first"]]) / 3600.0)
    assert fit.span_hours[0, 0] == 14 * 24 + 15.5
    path = str(tmp_path / "tides.npz")
    fit.save(path)
    back = load_tides(path)
    for k in ("coef_u", "coef_v", "rms_u", "explained_v", "n", "first", "last", "status", "span_hours", "residual_v", "mean_u"):
        assert np.array_equal(getattr(back, k), getattr(fit, k), equal_nan=True), k
    assert (back.names, back.speeds, back.t0, back.trend, back.trend_ref) == (fit.names, fit.speeds, fit.t0, fit.trend, fit.trend_ref)
    with pytest.raises(ValueError):
        back.predict(time)                                                        # the device's: needs a Context
    trended = fit_tides_host(cube, ("M2",), trend=True, min_samples=50)
    trended.save(path)
    assert load_tides(path).trend_ref == trended.trend_ref == tides.trend_reference(time, TC.T0)
    assert load_tides(path).residual_u is None
    with pytest.raises(ValueError):
        fit_tides_host(dict(cube, u=cube["u"][:1]), ("M2",))
    with pytest.raises(ValueError):
        fit_tides_host(cube, ("S2", "K2"))                                        # Rayleigh, over 15 days


def test_host_call_checks_its_arguments():
    lib = _lib.load()
    nc, nt, m = 3, 8, 2
    a = np.zeros((nt, nc))
    basis = np.ones((nt, 19))
    f = lambda q: q.ctypes.data_as(_lib.f64p)                                     # noqa: E731
    outs = [np.zeros(nc * 19) for _ in range(6)]
    ints = [np.zeros(nc, np.int32) for _ in range(4)]

    def call(u=a, v=a, count=a, ncells=nc, windows=nt, b=basis, terms=m, min_samples=0, drop=None):
        o = [f(q) for q in outs] + [q.ctypes.data_as(_lib.i32p) for q in ints]
        if drop is not None:
            o[drop] = None
        return lib.icelk_tide_fit_host(None if u is None else f(u), None if v is None else f(v), None if count is None else f(count),
                                       ncells, windows, None if b is None else f(b), terms, 1.0, min_samples, *o, None, None)
    assert call() == _lib.OK
    assert call(terms=18) == _lib.OK and call(terms=19) == _lib.ECAP
    for kw in (dict(u=None), dict(v=None), dict(count=None), dict(b=None), dict(ncells=0), dict(windows=0), dict(terms=0),
               dict(min_samples=-1)):
        assert call(**kw) == _lib.EARG, kw
    for k in range(10):
        assert call(drop=k) == _lib.EARG, k
    # the workspace of chunk partials: (m (m + 1) / 2 + 2 m + 2) * chunks * cells must fit 31 bits -- refused before anything is read
    assert call(ncells=1 << 24, windows=1, terms=18) == _lib.ECAP                 # 209 sums * 1 chunk * 2^24 cells >= 2^31
    assert call(ncells=1 << 20, windows=1 << 11, terms=1) == _lib.ECAP            # cells x windows = 2^31
    with pytest.raises(ValueError):
        tides.fit_arrays_host(a, a, a[:4], basis[:, :2])
    with pytest.raises(ValueError):
        tides.fit_arrays_host(a, a, a, basis[:4, :2])
    with pytest.raises(_lib.IcelkError):
        tides.fit_arrays_host(a, a, a, basis)
    assert C.sizeof(C.c_double) == 8

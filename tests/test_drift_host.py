"""Virtual drifters on the host (csrc/drift.h through icelk_drift_host).  No GPU.

- the host statement equals the numpy restatement (tests/drift_restatement.py) on every case of the catalogue
  (tests/drift_cases.py), every output compared as bit patterns, NaN included;
- uniform flow in dyadic numbers: every recorded position is seed + s * step * (u, v) exactly;
- solid-body rotation against the closed form of RK4 on a linear system, within a tolerance counted from the operations;
- the tide source against a cube made of the fit's own predictions: the same positions bit for bit;
- `drift_schedule` against a brute-force search; the Python-level refusals; `save` / `load_drift`."""
import numpy as np
import pytest

import drift_cases as DC
from drift_restatement import RESULT_KEYS, same_bits
from iceberg_tracking_code_amd import DriftResult, TideFit, drift_host, drift_lattice, drift_schedule, load_drift, seed_line, seed_nodes
from iceberg_tracking_code_amd import drift as drift_device
from iceberg_tracking_code_amd.transect import locate_points_along_transect

CASES = DC.catalogue()


def cube_of(rows, cols, x0, y0, dx, dy, time, u, v):
    """a cube dict with the node fields u, v (rows, cols) -- or (rows, cols, windows) -- at every window"""
    yy, xx = np.meshgrid(y0 + dy * np.arange(rows), x0 + dx * np.arange(cols), indexing="ij")
    nt = len(time)
    full = lambda a: np.repeat(a[:, :, None], nt, axis=2) if a.ndim == 2 else a      # noqa: E731
    return dict(x=xx, y=yy, time=np.asarray(time, np.float64), u=full(np.asarray(u, np.float64)), v=full(np.asarray(v, np.float64)),
                count=np.ones((rows, cols, nt)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_restatement(case):
    got, want = DC.run(case), DC.expected(case)
    assert same_bits(got, want) is None
    plain = DC.run(case, visits=False)
    assert plain["visits"] is None and same_bits(plain, want, keys=RESULT_KEYS[:-1]) is None


def test_catalogue_reaches_what_it_names():
    seen = np.zeros(5, int)
    for c in CASES:
        seen += np.bincount(DC.expected(c)["status"], minlength=5)
    assert np.all(seen > 0), seen                                   # every status code occurs
    stages = DC.case("stages")
    r = DC.expected(stages)
    assert list(r["status"]) == stages["info"]["status"] and list(r["stop_step"]) == [0, 0, 0, 1]
    assert abs(r["last_x"][3] - stages["x"][3] - stages["info"]["moved"]) < 1e-6 and np.array_equal(r["last_x"][:3], stages["x"][:3])
    for k in (1, 2, 3, 4):                                          # on an unmeasured node with all the weight: too few, whatever min_nodes
        c = DC.case("holes_min_nodes_%d" % k)
        r = DC.expected(c)
        on_hole = ~np.isfinite(c["u"][0] + c["v"][0] + c["u"][1] + c["v"][1])[:c["info"]["on_nodes"]]
        assert on_hole.any() and np.all(r["status"][:c["info"]["on_nodes"]][on_hole] == 2)
        assert np.all(r["stop_step"][:c["info"]["on_nodes"]][on_hole] == 0)
    gap = DC.case("night_gap")
    assert set(np.unique(gap["flag"])) == {0, 1} and np.any((gap["a"] == 0) & (gap["flag"] == 1) & (gap["k0"] == gap["k1"]))
    assert gap["flag"][0] == 0 and gap["flag"][-1] == 0            # starts before the record, ends after it
    assert np.any(DC.expected(gap)["status"] == 3)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_uniform_flow_is_exact(order):
    """Dyadic numbers throughout, so that no operation of the rule rounds: lattice x0 = 1024, y0 = 2048, spacing 256, -256, 5 x 5
    nodes; u = 1/2, v = -1/4 m/s; step 96 s, hence step / 2 = 48 and step / 6 = 16 exactly; seeds on multiples of 4; the two
    windows 1536 s = 32 * 48 apart, so a is a multiple of 1/64.
    On paper: every position met is a multiple of 4 below 4096 (the stage offsets are 24, 48 in x and 12, 24 in y, the step's 48
    and 24), so fx, fy are multiples of 1/64, the weights multiples of 2^-12 that sum to 1, a weight times 1/2 or 1/4 a multiple of
    2^-14, and (1 - a) u + a u = u since (1 - a) and a are multiples of 1/64: each sample returns (1/2, -1/4) exactly.  The sums
    ((k1 + 2 k2) + 2 k3) + k4 are 3 and -3/2, times 16: 48 and -24, the same as 96 * 1/2 and 96 * -1/4 of the lower orders."""
    rng = np.random.default_rng(3)
    cube = cube_of(5, 5, 1024.0, 2048.0, 256.0, -256.0, [1000.0, 2536.0], np.full((5, 5), 0.5), np.full((5, 5), -0.25))
    n, nsteps = 40, 10
    sx, sy = 1024.0 + 4.0 * rng.integers(0, 130, n), 2048.0 - 4.0 * rng.integers(0, 190, n)      # 10 steps stay inside: 520 + 480, 760 + 240
    r = drift_host(cube, sx, sy, start=1000.0, nsteps=nsteps, step=96.0, order=order, every=1)
    assert np.all(r.status == 0) and np.all(r.stop_step == nsteps)
    s = np.arange(nsteps + 1, dtype=np.float64)[:, None]
    assert np.array_equal(r.x, sx[None, :] + s * 48.0) and np.array_equal(r.y, sy[None, :] - s * 24.0)
    assert np.array_equal(r.time, 1000.0 + 96.0 * np.arange(nsteps + 1))
    length = np.zeros(n)
    for _ in range(nsteps):
        length = length + np.hypot(48.0, -24.0)
    assert np.array_equal(r.length, length)


def test_solid_body_rotation_follows_the_closed_form():
    """u = -w (y - yc), v = w (x - xc) on UTM-sized coordinates.  Bilinear interpolation reproduces a linear field, and RK4 of the
    linear system z' = i w (z - c) is z_n - c = G^n (z_0 - c) with G = 1 + i w h - (w h)^2 / 2 - i (w h)^3 / 6 + (w h)^4 / 24.
    The tolerance is nsteps * K * 2^-52 * max(|x|, |y|), K = 10 counted from one step, per coordinate, every rounding bounded by
    2^-53 of the largest coordinate (so 2^-52 leaves a factor of two):
      1  the addition p + (step / 6) * (...) that makes the new position -- the only rounding that lands in the position undamped;
      3  the additions p + c * k that make the positions of stages 2, 3 and 4 (they act through the velocity, scaled by w h << 1);
      4  the subtractions px - x0 (or py - y0) of the four samples, likewise scaled;
      1  all arithmetic on lattice coordinates, weights and velocities together: some 40 operations, each a relative 2^-53 of a
         displacement of metres, not of a coordinate of millions of metres;
      1  the reference: G^n (z_0 - c) in complex double and the one addition of c."""
    rows, cols, x0, y0, d = 33, 65, 500000.0, 6500000.0, 200.0
    xc, yc = x0 + d * 32, y0 - d * 16
    w, h, nsteps, K = 1.0 / 1200.0, 60.0, 500, 10
    yy, xx = np.meshgrid(y0 - d * np.arange(rows), x0 + d * np.arange(cols), indexing="ij")
    cube = cube_of(rows, cols, x0, y0, d, -d, [0.0, h * nsteps], -w * (yy - yc), w * (xx - xc))
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    radius = np.linspace(150.0, 2900.0, 24)
    sx, sy = xc + radius * np.cos(ang), yc + radius * np.sin(ang)
    r = drift_host(cube, sx, sy, start=0.0, nsteps=nsteps, step=h, order=4, every=50)
    assert np.all(r.status == 0)
    wh = w * h
    G = 1 + 1j * wh - wh ** 2 / 2 - 1j * wh ** 3 / 6 + wh ** 4 / 24
    z = ((sx - xc) + 1j * (sy - yc))[None, :] * (G ** np.arange(0, nsteps + 1, 50))[:, None]
    tol = nsteps * K * 2.0 ** -52 * max(np.abs(xx).max(), np.abs(yy).max())
    ex, ey = np.abs(r.x - (xc + z.real)).max(), np.abs(r.y - (yc + z.imag)).max()
    print("rotation: %d steps, w h = %.3f, %.1f turns; largest |error| %.3e, %.3e m against %.3e m" % (nsteps, wh, nsteps * wh / (2 * np.pi), ex, ey, tol))
    assert ex <= tol and ey <= tol
    assert np.abs(r.length / (nsteps * radius * abs(G - 1)) - 1).max() < 1e-3       # chords of the spiral, nearly the circle's


def hand_fit(rng, rows, cols, names=("M2", "K1"), t0=DC.T0):
    speeds = [28.9841042, 15.0410686][:len(names)]
    m = 1 + 2 * len(names)
    status = np.zeros((rows, cols), np.int32)
    status[rng.random((rows, cols)) < 0.15] = 1
    coef_u, coef_v = 0.02 * rng.normal(size=(rows, cols, m)), 0.02 * rng.normal(size=(rows, cols, m))
    coef_u[status != 0], coef_v[status != 0] = np.nan, np.nan
    nanf = np.full((rows, cols), np.nan)
    fields = dict(coef_u=coef_u, coef_v=coef_v, status=status, rms_u=nanf, rms_v=nanf, explained_u=nanf, explained_v=nanf,
                  n=np.zeros((rows, cols), np.int32), first=np.zeros((rows, cols), np.int32), last=np.zeros((rows, cols), np.int32),
                  span_hours=nanf, residual_u=None, residual_v=None)
    return TideFit(fields, names, speeds, t0, False, None)


def predicted(fit, times):
    """(u, v), each (rows, cols, len(times)): the sum of `TideFit.predict`, term by term in the rule's order, NaN where not fitted"""
    B = fit.basis(times)
    out = []
    for coef in (fit.coef_u, fit.coef_v):
        p = coef[:, :, None, 0] * B[None, None, :, 0]
        for j in range(1, B.shape[1]):
            p = p + coef[:, :, None, j] * B[None, None, :, j]
        out.append(np.where((fit.status == 0)[:, :, None], p, np.nan))
    return out


def test_tide_source_equals_a_cube_of_its_predictions():
    rng = np.random.default_rng(11)
    rows, cols, nt = 6, 9, 40
    fit = hand_fit(rng, rows, cols)
    time = DC.T0 + 1800.0 * np.arange(nt)
    u, v = predicted(fit, time)
    cube = cube_of(rows, cols, DC.X0, DC.Y0, DC.DX, DC.DY, time, u, v)
    sx, sy = seed_nodes(cube, measured_in=fit)
    sx, sy = sx + 37.0, sy - 61.0
    kw = dict(start=time[0], nsteps=nt - 1, step=1800.0, order=1, min_nodes=2, every=1, visits=True)
    a, b = drift_host(cube, sx, sy, **kw), drift_host((fit, cube), sx, sy, **kw)
    for k in DriftResult.FIELDS + ("visits",):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert len(np.unique(a.status)) > 1 and a.length.max() > 300.0


def test_schedule_against_brute_force():
    rng = np.random.default_rng(5)
    time = np.cumsum(rng.choice([600.0, 1800.0, 1800.0, 9000.0], 60)) + DC.T0
    for step, start, max_gap in ((77.0, time[0] - 500.0, None), (-300.0, time[-1] + 1000.0, 2000.0), (900.0, time[3], 1e9)):
        nsteps = 400
        S = drift_schedule(time, start, step, nsteps, max_gap)
        gap = 2.0 * np.median(np.diff(time)) if max_gap is None else max_gap
        assert len(S["t"]) == 2 * nsteps + 1 and S["k0"].dtype == np.int32 and S["flag"].dtype == np.int32
        for r in range(2 * nsteps + 1):
            t = start + (r // 2) * step + (step / 2.0 if r % 2 else 0.0)
            assert S["t"][r] == t
            if t < time[0] or t > time[-1]:
                assert (S["flag"][r], S["k0"][r], S["k1"][r], S["a"][r]) == (0, 0, 0, 0.0)
                continue
            k0 = max(k for k in range(len(time)) if time[k] <= t)
            k1 = min(k for k in range(len(time)) if time[k] >= t)
            assert (S["k0"][r], S["k1"][r]) == (k0, k1)
            assert S["a"][r] == (0.0 if k0 == k1 else (t - time[k0]) / (time[k1] - time[k0]))
            assert S["flag"][r] == (1 if time[k1] - time[k0] <= gap else 0)
    assert np.any(drift_schedule(time, time[3], 900.0, 400, 1e9)["k0"] == drift_schedule(time, time[3], 900.0, 400, 1e9)["k1"])
    one = drift_schedule([5.0], 5.0, 1.0, 2)                        # a record of one window: an exact hit, then past its end
    assert list(one["flag"]) == [1, 0, 0, 0, 0]
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [np.nan, 1.0]):
        with pytest.raises(ValueError):
            drift_schedule(bad, 0.0, 1.0, 2)


def test_seeds():
    cube = cube_of(4, 6, DC.X0, DC.Y0, DC.DX, DC.DY, [0.0, 1.0], np.zeros((4, 6)), np.zeros((4, 6)))
    x, y = seed_nodes(cube)
    assert len(x) == 24 and x[1] == DC.X0 + DC.DX and y[6] == DC.Y0 + DC.DY
    x, y = seed_nodes(cube, stride=2)
    assert len(x) == 6
    mask = np.zeros((4, 6), bool)
    mask[2, 4] = mask[1, 1] = True
    x, y = seed_nodes(cube, stride=2, measured_in=mask)
    assert list(x) == [DC.X0 + 4 * DC.DX] and list(y) == [DC.Y0 + 2 * DC.DY]
    p1, p2 = (DC.X0 + 10.0, DC.Y0 - 30.0), (DC.X0 + 410.0, DC.Y0 - 330.0)
    x, y = seed_line(p1, p2, 6)
    pts = np.array(locate_points_along_transect(p1, p2, 100.0)[0])   # 500 m in steps of 100 m: the same six points
    assert np.array_equal(x, pts[:, 0]) and np.array_equal(y, pts[:, 1])
    assert abs(x[-1] - p2[0]) < 1e-6 and abs(y[-1] - p2[1]) < 1e-6


def test_python_refusals():
    cube = cube_of(4, 6, DC.X0, DC.Y0, DC.DX, DC.DY, [0.0, 600.0], np.zeros((4, 6)), np.zeros((4, 6)))
    x, y = seed_nodes(cube)
    ok = dict(start=0.0, nsteps=5)
    assert np.all(drift_host(cube, x, y, **ok).status == 0)
    L = drift_lattice(cube)
    assert (L.x0, L.y0, L.dx, L.dy, L.rows, L.cols) == (DC.X0, DC.Y0, DC.DX, DC.DY, 4, 6)
    bent = dict(cube, x=cube["x"].copy())
    bent["x"][2, 3] += 1.0
    thin = {k: (v[:1] if k != "time" else v) for k, v in cube.items()}
    for bad in (bent, thin, dict(cube, x=cube["x"][:, :1], y=cube["y"][:, :1]), dict(cube, x=cube["x"] * np.nan)):
        with pytest.raises(ValueError):
            drift_lattice(bad)
    for kw in (dict(step=0.0), dict(step=np.inf), dict(nsteps=0), dict(every=0), dict(order=3), dict(min_nodes=0), dict(min_nodes=5),
               dict(release=np.zeros(len(x))), dict(release=np.zeros(3, np.int32)), dict(start=np.nan)):
        with pytest.raises(ValueError):
            drift_host(cube, x, y, **dict(ok, **kw))
    with pytest.raises(ValueError):
        drift_host(cube, x, y[:-1], **ok)
    with pytest.raises(ValueError):
        drift_host(cube, [], [], **ok)
    with pytest.raises(ValueError):
        drift_host(dict(cube, u=cube["u"][:3]), x, y, **ok)            # the field is not on the lattice of x, y
    with pytest.raises(ValueError):
        drift_host((hand_fit(np.random.default_rng(1), 3, 3), cube), x, y, **ok)   # a fit of other cells
    with pytest.raises(ValueError):
        drift_device("a cube", x, y, **ok)
    with pytest.raises(ValueError):
        drift_device((hand_fit(np.random.default_rng(1), 4, 6), cube), x, y, **ok)   # no Context to run on


def test_save_and_load(tmp_path):
    c = DC.case("shape_3x5x3_n65_s97_e3_o4")
    cube = DC.cube_dict(c)
    kw = dict(start=c["start"], nsteps=97, step=60.0, release=c["release"], order=4, min_nodes=3, every=3)
    r = drift_host(cube, c["x"], c["y"], visits=True, **kw)
    want = DC.expected(c)
    assert same_bits(r.__dict__, want) is None                       # the Python layer reaches the same tables as the catalogue
    for with_visits in (True, False):
        if not with_visits:
            r = drift_host(cube, c["x"], c["y"], **kw)
        path = str(tmp_path / ("drift%d.npz" % with_visits))
        r.save(path)
        back = load_drift(path)
        for k in DriftResult.FIELDS:
            assert getattr(back, k).tobytes() == getattr(r, k).tobytes() and getattr(back, k).dtype == getattr(r, k).dtype, k
        assert (back.visits is None) == (not with_visits)
        if with_visits:
            assert back.visits.tobytes() == r.visits.tobytes() and back.visits.sum() == np.isfinite(r.x + r.y).sum() - off_lattice(r, cube)


def off_lattice(r, cube):
    """recorded finite samples whose nearest node is off the lattice"""
    L = drift_lattice(cube)
    fin = np.isfinite(r.x + r.y)
    gx, gy = np.floor((r.x[fin] - L.x0) / L.dx + 0.5), np.floor((r.y[fin] - L.y0) / L.dy + 0.5)
    return int((~((gx >= 0) & (gx <= L.cols - 1) & (gy >= 0) & (gy <= L.rows - 1))).sum())

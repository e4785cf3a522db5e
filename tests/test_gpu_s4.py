"""GPU: the averages of step s4 (postprocess.py, icelk_cube_* in csrc/k_cube.hip).

- every call of the reference's own average_spatially_temporally recorded in tests/golden/s4_golden.npz: all six return
  values, flips included, the six-NaN and the ValueError case;
- average_periods over all recorded periods at once equals the calls one at a time;
- the chain utm_to_gridded_utm (golden day) -> combine_npzs -> averages equals the golden;
- daily_averages: the __main__ loop, its csv files byte for byte;
- a seeded season against numpy itself on the host (np.nanmean, np.nansum, spatial_mean restated below);
- small cubes at the geometries where numpy changes its order of additions, and cubes of one and two cells;
- the ABI's argument checks on a live handle.
Equality is bit for bit on every non-NaN float64, NaN in the same places (G.same_floats); no tolerance anywhere."""
import datetime as dt
import os
import warnings

import numpy as np
import pytest

import day_grid_golden as DG
import s4_golden as G
from iceberg_tracking_code_amd import (Context, IcelkError, VelocityCube, _lib, average_periods,
                                       average_spatially_temporally, combine_npzs, daily_averages, postprocess,
                                       utm_to_gridded_utm)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return G.load()


@pytest.fixture(scope="module")
def cube(z, ctx):
    c = VelocityCube(G.cube(z), ctx)
    yield c
    c.close()


def check_call(got, c):
    if c["kind"] == "nan":
        assert len(got) == 6 and all(isinstance(q, float) and np.isnan(q) for q in got)
        return
    assert len(got) == 6 and got[5] == c["time_str"]
    for a, k in zip(got, ("x", "y", "u", "v", "count")):
        assert G.same_floats(a, c[k]), (k, c["start"], c["coarseness"])


def test_golden_calls_one_at_a_time(z, cube):
    for c in G.calls(z):
        if c["kind"] == "raises":
            with pytest.raises(ValueError):
                average_spatially_temporally(c["start"], c["end"], c["coarseness"], cube)
        else:
            check_call(average_spatially_temporally(c["start"], c["end"], c["coarseness"], cube), c)


def test_call_from_a_dict_and_a_file(z, ctx, cube, tmp_path):
    c = [c for c in G.calls(z) if c["kind"] == "ok" and c["coarseness"] == 3][0]
    with pytest.raises(IcelkError):                              # the context already holds the fixture's cube
        average_spatially_temporally(c["start"], c["end"], 3, G.cube(z), ctx)
    check_call(average_spatially_temporally(c["start"], c["end"], 3, cube), c)      # which is still there
    with Context(64, 64, n_slots=1, max_pts=1024) as other:
        check_call(average_spatially_temporally(c["start"], c["end"], 3, G.cube(z), other), c)
    np.savez(str(tmp_path / "cube.npz"), **G.cube(z))
    check_call(average_spatially_temporally(c["start"], c["end"], 3, np.load(str(tmp_path / "cube.npz"))), c)


def test_all_periods_at_once_equal_single_calls(z, cube):
    calls = G.calls(z)
    for coarseness in sorted({c["coarseness"] for c in calls}):
        periods = [(c["start"], c["end"]) for c in calls]
        together = average_periods(cube, periods, coarseness)
        assert len(together) == len(calls)
        for c, r in zip(calls, together):
            alone = average_periods(cube, [(c["start"], c["end"])], coarseness)[0]
            assert r["has_data"] == alone["has_data"] and r["time_str"] == alone["time_str"]
            for k in ("x", "y", "u", "v", "speed", "count"):
                assert G.same_floats(r[k], alone[k]), (k, c["start"], coarseness)
            assert r["has_data"] == (c["kind"] == "ok") and (r["time_str"] is None) == (c["kind"] == "raises")
            with np.errstate(invalid="ignore"):
                assert G.same_floats(r["speed"], np.hypot(r["u"], r["v"]))
            if c["coarseness"] == coarseness and c["kind"] == "ok":
                flip = np.flipud if coarseness == 1 else (lambda a: a)
                assert G.same_floats(flip(r["u"]), c["u"]) and G.same_floats(flip(r["v"]), c["v"])
                assert G.same_floats(r["count"], c["count"]) and G.same_floats(flip(r["y"]), c["y"])


def test_chain_from_the_day_driver(z, ctx, tmp_path):
    z0 = DG.load()
    DG.build_tree(z0, str(tmp_path / "in"))
    camnames, schedule, drifts, fjord, day, grid_size, thr = DG.args(z0)
    run = tmp_path / "run1"
    run.mkdir()
    written = utm_to_gridded_utm(camnames, str(tmp_path / "in"), "utm", str(run), schedule, drifts, fjord, day, 0.5,
                                 grid_size, thr, ctx=ctx)
    assert len(written) == 10
    G.build_folder(z, str(run), golden_day=False)
    stacked = combine_npzs(str(run), str(tmp_path), "cube.npz")
    want = G.cube(z)
    for k in G.CUBE_KEYS:
        assert stacked[k].dtype == want[k].dtype and stacked[k].tobytes() == want[k].tobytes(), k
    with VelocityCube(str(tmp_path / "cube.npz")) as c2:          # from the file, on a context of its own
        for c in G.calls(z):
            if c["kind"] != "raises":
                check_call(average_spatially_temporally(c["start"], c["end"], c["coarseness"], c2), c)


@pytest.mark.parametrize("coarseness", [1, 2])
def test_daily_averages(z, cube, tmp_path, coarseness):
    days = [dt.datetime(2019, 7, d) for d in range(24, 31)]
    got = daily_averages(cube, days, coarseness=coarseness, csv_workspace=str(tmp_path), name_fjord=str(z["name_fjord"]))
    calls = {c["start"]: c for c in G.calls(z) if c["coarseness"] == 1 and c["start"].hour == 12}
    assert [d for d, _ in got] == [d for d in days if calls[d + dt.timedelta(hours=12)]["kind"] == "ok"]
    assert len(got) == 5
    for d, fields in got:
        alone = average_spatially_temporally(d + dt.timedelta(hours=12), d + dt.timedelta(hours=34), coarseness, cube)
        assert fields[5] == alone[5] and G.same_floats(fields[0], alone[0]) and G.same_floats(fields[4], alone[4])
        for k in (1, 2, 3):
            assert G.same_floats(fields[k], np.flipud(alone[k]))
    # the files of the day the reference's loop was recorded for
    want = G.csv_files(z, "savecsv%d" % coarseness)
    for name, data in want.items():
        assert open(os.path.join(str(tmp_path), name), "rb").read() == data, name


# ---- a seeded season against numpy on the host ------------------------------------------------------------------------

ROWS, COLS, NT = 101, 89, 1500          # primes: every coarseness pads both axes


def spatial_mean_numpy(a, c):
    """Blocks of c x c cells averaged with np.mean after zero padding to a multiple of c; the padded cells count."""
    rows, cols = a.shape
    pr, pc = -(-rows // c) * c, -(-cols // c) * c
    padded = np.zeros((pr, pc))
    padded[:rows, :cols] = a
    return np.mean(padded.reshape(pr // c, c, pc // c, c), axis=(1, 3))


def season():
    rng = np.random.default_rng(41)
    t0 = dt.datetime(2021, 5, 1)
    steps = np.sort(rng.choice(70 * 48, NT, replace=False))            # 30-minute windows with gaps, 70 days
    steps = steps[(steps // 48 != 20) & (steps // 48 != 21)]           # two days without a window
    time = np.array([postprocess.epoch_seconds(t0 + dt.timedelta(minutes=30 * int(s))) for s in steps], np.float64)
    nt = len(time)
    shape = (ROWS, COLS, nt)
    u = rng.normal(0.1, 0.3, shape) * 10.0 ** rng.integers(-3, 2, shape)
    v = rng.normal(-0.05, 0.2, shape) * 10.0 ** rng.integers(-3, 2, shape)
    count = np.where(rng.random(shape) < 0.1, rng.integers(50001, 90000, shape), rng.integers(4, 3000, shape)).astype(np.float64)
    hole = rng.random(shape) < 0.35
    hole[:, :, (steps // 48 == 30)] = True                             # a day whose windows are all empty
    hole[5, 7, :] = True                                               # a cell never measured
    hole[6, 8, :] = True
    hole[6, 8, nt // 2] = False                                        # a cell measured once
    hole[:40, :30, :] |= rng.random((40, 30, 1)) < 0.5                 # half the cells of a corner never measured
    for a in (u, v, count):
        a[hole] = np.nan
    yy, xx = np.meshgrid(7000000.0 - 200.0 * np.arange(ROWS), 500000.0 + 200.0 * np.arange(COLS), indexing="ij")
    days = [t0 + dt.timedelta(days=d) for d in range(70)]
    periods = [(d + dt.timedelta(hours=12), d + dt.timedelta(hours=34)) for d in days]
    periods += [(t0 + dt.timedelta(days=7 * w), t0 + dt.timedelta(days=7 * w + 7)) for w in range(10)]
    periods += [(t0, t0 + dt.timedelta(days=70)), (t0 + dt.timedelta(days=2), t0 + dt.timedelta(days=2, hours=3)),
                (t0 + dt.timedelta(days=5), t0 + dt.timedelta(days=5, hours=7)),
                (t0 + dt.timedelta(days=30), t0 + dt.timedelta(days=31))]      # whole run, a few windows (2), no data
    return dict(x=xx, y=yy, u=u, v=v, count=count, time=time), periods


def numpy_averages(data, mask):
    """The fine fields of one period, the reference's way: np.nanmean / np.nansum over the masked cube."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        um = np.nanmean(data["u"][:, :, mask], 2)
        vm = np.nanmean(data["v"][:, :, mask], 2)
        cs = np.nansum(data["count"][:, :, mask], 2)
    return um, vm, cs


def test_seeded_season_equals_numpy():
    data, periods = season()
    time = data["time"]
    with VelocityCube(data) as cube:
        got = {c: average_periods(cube, periods, c) for c in (1, 3, 8)}
    seen = set()
    for p, (start, end) in enumerate(periods):
        mask = (time >= postprocess.epoch_seconds(start)) & (time < postprocess.epoch_seconds(end))
        if not mask.any():
            assert all(not got[c][p]["has_data"] and got[c][p]["time_str"] is None for c in got)
            seen.add("no window")
            continue
        um, vm, cs = numpy_averages(data, mask)
        with np.errstate(all="ignore"):
            has = not np.isnan(np.hypot(um, vm)).all()
        seen.add("data" if has else "no data")
        seen.add("long" if mask.sum() > 128 else "short" if mask.sum() < 8 else "")
        t = time[mask]
        name = (postprocess.epoch_to_datetime(t.min()).strftime("%Y%m%d_%H%M")
                + postprocess.epoch_to_datetime(t.max()).strftime("-%H%M"))
        for c, results in got.items():
            r = results[p]
            want = dict(u=um, v=vm, count=cs, x=data["x"], y=data["y"])
            if c > 1:
                want = {k: spatial_mean_numpy(a, c) for k, a in want.items()}
            with np.errstate(all="ignore"):
                want["speed"] = np.hypot(want["u"], want["v"])
            assert r["has_data"] == has and r["time_str"] == name
            for k, a in want.items():
                assert G.same_floats(r[k], a), (k, start, end, c)
    assert {"no window", "no data", "data", "long", "short"} <= seen, seen


# ---- the geometries at which numpy changes its order of additions --------------------------------------------------------

# (rows, cols, c): one coarse column with three and five coarse rows, two coarse columns, one coarse row, the smallest
# fields, the first c whose single-column block exceeds numpy's buffer of 8192 elements and larger ones, 128 (where
# the halves of one pairwise run are the buffer's chunks), and rows of more than 128 terms with two coarse columns
GEOMETRIES = [(23, 5, 8), (23, 5, 5), (23, 6, 5), (5, 23, 8), (1, 1, 2), (1, 40, 7), (40, 1, 7), (94, 90, 91),
              (130, 100, 127), (150, 64, 128), (263, 17, 129), (300, 2, 300), (20, 260, 129)]


def small_cube(rows, cols, nt, rng, hole_share=0.3, keep=None):
    """A cube over seven decades with NaN holes.  count is not made of integers here: the device treats it as any
    float64, and integers would add up to the same bits in any order.  keep: windows of which every cell keeps at
    least one value, so that a coarse mean over them is a number and not the NaN a single empty cell makes of it."""
    t0 = dt.datetime(2021, 5, 1)
    time = np.array([postprocess.epoch_seconds(t0 + dt.timedelta(minutes=30 * k)) for k in range(nt)], np.float64)
    shape = (rows, cols, nt)
    u = rng.normal(0.1, 0.3, shape) * 10.0 ** rng.integers(-3, 2, shape)
    v = rng.normal(-0.05, 0.2, shape) * 10.0 ** rng.integers(-3, 2, shape)
    count = rng.uniform(0.5, 3000.0, shape) * 10.0 ** rng.integers(-3, 2, shape)
    hole = rng.random(shape) < hole_share
    if keep is not None:
        empty = hole[:, :, keep].all(axis=2)
        hole[:, :, keep[0]] &= ~empty
    for a in (u, v, count):
        a[hole] = np.nan
    yy, xx = np.meshgrid(7000000.0 - 200.0 * np.arange(rows), 500000.0 + 200.0 * np.arange(cols), indexing="ij")
    at = lambda k: t0 + dt.timedelta(minutes=30 * k)        # noqa: E731
    return dict(x=xx, y=yy, u=u, v=v, count=count, time=time), at


def check_periods_against_numpy(own, data, periods, coarseness, tag):
    with VelocityCube(data, own) as cube:
        got = average_periods(cube, periods, coarseness)
    time = data["time"]
    finite = 0
    for r, (start, end) in zip(got, periods):
        mask = (time >= postprocess.epoch_seconds(start)) & (time < postprocess.epoch_seconds(end))
        assert mask.any()
        um, vm, cs = numpy_averages(data, mask)
        with np.errstate(all="ignore"):
            has = not np.isnan(np.hypot(um, vm)).all()
        want = dict(u=um, v=vm, count=cs)
        if coarseness > 1:
            want = {k: spatial_mean_numpy(a, coarseness) for k, a in want.items()}
        with np.errstate(all="ignore"):
            want["speed"] = np.hypot(want["u"], want["v"])
        assert r["has_data"] == has, (tag, int(mask.sum()))
        for k, a in want.items():
            assert r[k].shape == a.shape and G.same_floats(r[k], a), (k, tag, int(mask.sum()))
        finite += int(np.isfinite(want["u"]).sum())
    return finite


def test_spatial_mean_geometry_equals_numpy():
    """Two periods per cube, all windows but the last and the last alone, about 30 % NaN: u, v, count and speed equal
    np.nanmean / np.nansum / np.mean of the padded blocks at every geometry of the table above."""
    rng = np.random.default_rng(97)
    with Context(64, 64, n_slots=1, max_pts=1024) as own:
        for n, (rows, cols, c) in enumerate(GEOMETRIES):
            nt = 3 + n % 3
            data, at = small_cube(rows, cols, nt, rng, keep=list(range(nt - 1)))
            periods = [(at(0), at(nt - 1)), (at(nt - 1), at(nt))]
            assert 0.2 < np.isnan(data["u"]).mean() < 0.4 or rows * cols < 50
            finite = check_periods_against_numpy(own, data, periods, c, (rows, cols, c))
            assert finite >= -(-rows // c) * -(-cols // c)          # the long period's coarse means are numbers


def test_one_cell_cube_equals_numpy():
    """A cube of one cell is a contiguous run to numpy, added pairwise and not window after window; its neighbours of
    two cells are not.  1000 windows, 30 % NaN, periods of 1, 7, 8, 9, 128, 129, 300 and 900 windows."""
    rng = np.random.default_rng(98)
    spans = [(0, 1), (1, 8), (10, 18), (20, 29), (100, 228), (300, 429), (500, 800), (50, 950)]
    with Context(64, 64, n_slots=1, max_pts=1024) as own:
        for rows, cols in ((1, 1), (1, 2), (2, 1)):
            data, at = small_cube(rows, cols, 1000, rng)
            data["u"][:, :, 0] = 0.25                                 # the period of one window holds a value
            periods = [(at(a), at(b)) for a, b in spans]
            check_periods_against_numpy(own, data, periods, 1, (rows, cols))


# ---- the ABI on a live handle -------------------------------------------------------------------------------------

def test_abi_argument_checks():
    lib = _lib.load()
    own = Context(64, 64, n_slots=1, max_pts=1024)
    try:
        h = own._h
        f64 = lambda a: a.ctypes.data_as(_lib.f64p)               # noqa: E731
        i32 = lambda a: a.ctypes.data_as(_lib.i32p)               # noqa: E731
        rows, cols, nt = 3, 4, 5
        a = np.arange(rows * cols * nt, dtype=np.float64)
        out = [np.zeros(2 * rows * cols) for _ in range(4)]
        has = np.zeros(2, np.int32)
        off, idx = np.array([0, 2, 5], np.int32), np.array([0, 1, 2, 3, 4], np.int32)

        def average(off=off, idx=idx, n=2, rows=rows, cols=cols, c=1, o=out, has=has):
            return lib.icelk_cube_average(h, i32(off) if off is not None else None, i32(idx), n, rows, cols, c,
                                          f64(o[0]), f64(o[1]), f64(o[2]), f64(o[3]) if o[3] is not None else None,
                                          i32(has), None)

        assert average() == _lib.ESTATE                       # no cube yet
        assert lib.icelk_cube_set(h, None, f64(a), f64(a), rows * cols, nt) == _lib.EARG
        assert lib.icelk_cube_set(h, f64(a), f64(a), f64(a), 0, nt) == _lib.EARG
        assert lib.icelk_cube_set(h, f64(a), f64(a), f64(a), rows * cols, -1) == _lib.EARG
        assert lib.icelk_cube_set(h, f64(a), f64(a), f64(a), 1 << 16, 1 << 15) == _lib.ECAP
        assert average() == _lib.ESTATE                       # the refused calls left nothing behind
        assert lib.icelk_cube_set(h, f64(a), f64(a), f64(a), rows * cols, nt) == _lib.OK
        assert average() == _lib.OK
        assert average(off=None) == _lib.EARG
        assert average(n=0) == _lib.EARG
        assert average(rows=-3) == _lib.EARG
        assert average(rows=4) == _lib.EARG                   # not the cube's cells
        assert average(c=0) == _lib.EARG
        assert average(off=np.array([0, 3, 2], np.int32)) == _lib.EARG
        assert average(off=np.array([1, 2, 5], np.int32)) == _lib.EARG
        assert average(idx=np.array([0, 1, 2, 3, 5], np.int32)) == _lib.EARG
        assert average(idx=np.array([0, -1, 2, 3, 4], np.int32)) == _lib.EARG
        assert average(o=out[:3] + [None]) == _lib.EARG
        assert average(c=40000) == _lib.ECAP
        assert average(c=8194) == _lib.ECAP                   # above the largest coarseness checked against numpy
        assert b"coarseness" in lib.icelk_last_error(h)
        coarse = [np.zeros(2) for _ in range(4)]
        assert average(c=8193, o=coarse) == _lib.OK           # at it: one coarse cell per period, mostly padding
        w = a.reshape(nt, rows, cols)
        fine_u = [(0.0 + w[0] + w[1]) / 2, (0.0 + w[2] + w[3] + w[4]) / 3]
        assert G.same_floats(coarse[0], np.array([spatial_mean_numpy(f, 8193)[0, 0] for f in fine_u]))
        assert b"" != lib.icelk_last_error(h)
        # results of the small cube: period 0 = windows 0, 1; period 1 = windows 2, 3, 4
        assert average() == _lib.OK
        cube = a.reshape(nt, rows * cols)
        assert np.array_equal(out[0][:rows * cols], (0.0 + cube[0] + cube[1]) / 2)
        assert np.array_equal(out[3][rows * cols:], cube[2] + cube[3] + cube[4])
        assert list(has) == [1, 1]
        assert lib.icelk_cube_release(h) == _lib.OK
        assert average() == _lib.ESTATE
        assert lib.icelk_cube_release(h) == _lib.OK           # releasing nothing is fine
        with pytest.raises(IcelkError):
            own._ck(average())
    finally:
        own.close()

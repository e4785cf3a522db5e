"""GPU: the normalised median test (csrc/k_validate.hip, icelk_validate, icelk_grid_bin_windows_validated).

- `validate_velocities` equals `validate_velocities_host` bit for bit on every case of the catalogue (tests/validate_cases.py):
  status, r2 and the per-cell arrays -- pools staged in LDS and pools that walk global memory (the two lds_limit cases);
- the day form on a seeded day of 2 cameras x 3 hours with planted outliers: the files of utm_to_gridded_utm(validate=True)
  equal the files of the plain driver run on the same day with the time of every vector the HOST statement rejects set to
  NaN, key for key and byte for byte, with and without stats=True; `rejected` equals the host's count; the caller's arrays
  are not written;
- validate=None: the golden day's files, and none of the new kernels runs (the profiling table);
- refusals leave the handle usable."""
import datetime as dt
import os

import numpy as np
import pytest

import day_grid_golden as G
import validate_cases as VC
from iceberg_tracking_code_amd import (_lib, bin_velocities, day_grid, utm_to_gridded_utm, validate_velocities, validate_velocities_host,
                                       validation_lattice)
from validate_restatement import same_bits

pytestmark = pytest.mark.gpu

CASES = VC.catalogue()
NEW_KERNELS = {"validate_assign", "validate_pools", "validate_judge"}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_host(ctx, case):
    args, kw = VC.call_args(case)
    got, want = validate_velocities(ctx, *args, **kw), validate_velocities_host(*args, **kw)
    assert same_bits(got, want) is None
    for p in case["info"].get("rejected", []):
        assert got["status"][p] == 1


def test_both_fetch_paths_are_met():
    """the catalogue's pools lie on both sides of the staging limit (and exactly on it)"""
    sizes = set()
    for c in CASES:
        args, kw = VC.call_args(c)
        sizes |= set(validate_velocities_host(*args, **kw)["pool_n"].ravel().tolist())
    assert {VC.POOL_LDS_TERMS, VC.POOL_LDS_TERMS + 1} <= sizes and min(sizes - {0}) == 1


# ---- the day form ----------------------------------------------------------------------------------------------------

DAY = dt.datetime(2021, 8, 3)
CAMS = [("north", "06:00", 2.0, 12.5), ("south", "06:00", 2.0, -7.25)]
GRID, THRESHOLD, POINTS = 100, 3, 3000
FJORD = {"x": np.array([500000.0, 500800.0, 500800.0, 500000.0]), "y": np.array([6499400.0, 6499400.0, 6500000.0, 6500000.0])}


def synth_day(root):
    """root/<camera>/utm/<hour>.npz for 2 cameras x 3 hours: a smooth field with +-0.01 m/s of noise and, per file, 15 vectors
    off by 1 m/s; times spill over the hours' edges.  Returns the schedule and drift rows."""
    rng = np.random.default_rng(21)
    for name, _, _, _ in CAMS:
        ws = os.path.join(root, name, "utm")
        os.makedirs(ws)
        for hr in (6, 7, 8):
            e0 = day_grid.epoch_seconds(DAY + dt.timedelta(hours=hr))
            t = np.sort(rng.integers(e0 - 300, e0 + 3900, POINTS)).astype(np.int64)
            x, y = rng.uniform(499950.0, 500850.0, POINTS), rng.uniform(6499350.0, 6500050.0, POINTS)
            u = 0.40 + 0.05 * (x - 500000.0) / 800.0 + rng.uniform(-0.01, 0.01, POINTS)
            v = -0.10 + 0.04 * (6500000.0 - y) / 600.0 + rng.uniform(-0.01, 0.01, POINTS)
            bad = rng.choice(POINTS, 15, replace=False)
            phi = rng.uniform(0, 2 * np.pi, 15)
            u[bad] += np.cos(phi)
            v[bad] += np.sin(phi)
            np.savez(os.path.join(ws, (DAY + dt.timedelta(hours=hr)).strftime("%Y%m%d_%H00") + "_30s_utm.npz"), x=x, y=y, u=u, v=v,
                     speed=np.hypot(u, v), time=t)
    schedule = [dict(camera=n, start_day=20210801, end_day=20210810, start_time=s, tracking_duration=d) for n, s, d, _ in CAMS]
    drifts = [dict(cam=n, start_date=20210801, end_date=20210810, drift_start_sec=c, drift_pday_sec=0.0) for n, _, _, c in CAMS]
    return schedule, drifts


@pytest.fixture(scope="module")
def day(tmp_path_factory):
    """The day on disk; the host statement's verdicts on its concatenated points; the same day with the time of every
    rejected vector set to NaN."""
    root = tmp_path_factory.mktemp("validate_day")
    a, b = str(root / "in"), str(root / "in_nan")
    schedule, drifts = synth_day(a)
    names = [c[0] for c in CAMS]
    plan = day_grid.plan_day(names, a, "utm", schedule, drifts, DAY, 0.5, GRID)
    L = day_grid.load_day(plan)
    nw = L["lo"].shape[1]
    group = day_grid.window_of_points(L["t"], L["off"], L["fcam"], L["lo"], L["hi"], L["wf0"], L["wf1"])
    host = validate_velocities_host(L["x"], L["y"], L["u"], L["v"], validation_lattice(FJORD, 2.0 * GRID), groups=(group, nw))
    rejected = host["status"] == 1
    for k, f in enumerate(plan.files):
        s = slice(int(L["off"][k]), int(L["off"][k + 1]))
        with np.load(f["path"]) as z:
            arrays = {key: z[key] for key in z.files}
        arrays["time"] = np.where(rejected[s], np.nan, arrays["time"].astype(np.float64))
        path = f["path"].replace(a, b)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, **arrays)
    per_window = {plan.name(w): int((rejected & (group == w)).sum()) for w in range(nw)}
    return dict(a=a, b=b, names=names, schedule=schedule, drifts=drifts, per_window=per_window, host=host, group=group, loaded=L)


def run_day(ctx, day, root, **kw):
    return utm_to_gridded_utm(day["names"], root, "utm", None, day["schedule"], day["drifts"], FJORD, DAY, 0.5, GRID, THRESHOLD, ctx=ctx,
                              save=False, **kw)


def test_day_has_something_to_reject(day):
    status, group = day["host"]["status"], day["group"]
    assert (status == 1).sum() >= 40 and (status == 3).sum() > 100 and (group >= 0).sum() > 10000
    assert sum(day["per_window"].values()) == (status == 1).sum() and max(day["per_window"].values()) > 5


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
def test_day_equals_plain_driver_on_host_verdicts(ctx, day, stats, monkeypatch):
    seen = {}
    load_day = day_grid.load_day

    def spy(plan, with_speed=False):
        out = load_day(plan, with_speed)
        seen["arrays"] = {k: out[k] for k in ("x", "y", "u", "v", "t")}
        seen["copies"] = {k: out[k].copy() for k in ("x", "y", "u", "v", "t")}
        return out
    monkeypatch.setattr(day_grid, "load_day", spy)
    got = run_day(ctx, day, day["a"], validate=True, stats=stats)
    for k, arr in seen["arrays"].items():                               # the caller's arrays, t among them, are not written
        assert arr.tobytes() == seen["copies"][k].tobytes(), k
    monkeypatch.setattr(day_grid, "load_day", load_day)
    want = run_day(ctx, day, day["b"], stats=stats)
    assert [name for name, _ in got] == [name for name, _ in want] and len(got) >= 4
    for (name, a), (_, b) in zip(got, want):
        assert sorted(a) == sorted(list(b) + ["rejected", "validation"]), name
        for k in b:
            p, q = np.asarray(a[k]), np.asarray(b[k])
            assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes(), (name, k)
        assert a["rejected"].shape == () and int(a["rejected"]) == day["per_window"][name], name
        assert a["validation"].dtype == np.float64 and a["validation"].tolist() == [2.0, 0.01, 8.0, 2.0 * GRID]
    plain = run_day(ctx, day, day["a"], stats=stats)                     # and the validation changed something
    assert any(a["count"].tobytes() != b["count"].tobytes() for (_, a), (_, b) in zip(got, plain))


def test_day_status_equals_host(ctx, day):
    timing = {}
    plan = day_grid.plan_day(day["names"], day["a"], "utm", day["schedule"], day["drifts"], DAY, 0.5, GRID)
    day_grid._grid_day(ctx, plan, FJORD, GRID, THRESHOLD, timing=timing, validate=day_grid.validate_options(True, GRID))
    assert timing["status"].tobytes() == day["host"]["status"].tobytes()
    nw = len(plan.windows)
    assert timing["rejected"].tolist() == [int(((day["host"]["status"] == 1) & (day["group"] == w)).sum()) for w in range(nw)]
    assert timing["kernels_ms"] > 0.0


def box_outline(lat):
    """the lattice's bounding box as a fjord outline"""
    x0, x1 = lat["left"], lat["left"] + lat["side"] * lat["cols"]
    y0, y1 = lat["top"] - lat["side"] * lat["rows"], lat["top"]
    return {"x": np.array([x0, x1, x1, x0]), "y": np.array([y0, y0, y1, y1])}


def profiled(ctx, call):
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = call()
    finally:
        ctx.prof_enable(False)
    table = ctx.prof_table()
    ctx.prof_reset()
    return out, table


def test_without_validation_nothing_new_runs(ctx, tmp_path):
    z = G.load()
    G.build_tree(z, str(tmp_path / "in"))
    camnames, schedule, drifts, fjord, day_, grid_size, thr = G.args(z)

    def call(**kw):
        return utm_to_gridded_utm(camnames, str(tmp_path / "in"), "utm", None, schedule, drifts, fjord, day_, float(z["time_windows"][0]),
                                  grid_size, thr, ctx=ctx, save=False, **kw)
    got, table = profiled(ctx, lambda: call(validate=None))
    want = G.outputs(z, 0)
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert sorted(a) == sorted(b), name
        for k in b:
            p, q = np.asarray(a[k]), np.asarray(b[k])
            assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes(), (name, k)
    assert "grid_day_assign" in table and not NEW_KERNELS & set(table)
    _, table = profiled(ctx, lambda: call(validate=True))               # the same look does see them when they run
    assert NEW_KERNELS <= set(table)


def test_bin_velocities_validated(ctx):
    case = [c for c in CASES if c["name"] == "planted_outliers"][0]
    lat = case["lattice"]
    fjord = box_outline(lat)
    x, y, u, v = (case[k] for k in "xyuv")
    _, table = profiled(ctx, lambda: bin_velocities(ctx, x, y, u, v, fjord, 50, 3))
    assert not NEW_KERNELS & set(table)
    got = bin_velocities(ctx, x, y, u, v, fjord, 50, 3, validate=True)      # side 100: the case's own lattice
    keep = np.ones(len(x), bool)
    keep[case["info"]["rejected"]] = False
    want = bin_velocities(ctx, x[keep], y[keep], u[keep], v[keep], fjord, 50, 3)
    assert got["rejected"] == VC.PLANTED and np.flatnonzero(got["status"] == 1).tolist() == case["info"]["rejected"]
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


@pytest.mark.parametrize("change,kind", VC.REFUSALS, ids=VC.REFUSAL_IDS)
def test_refusals_leave_the_handle_usable(ctx, change, kind):
    case = CASES[2]
    lat = case["lattice"]
    fjord = box_outline(lat)
    before = bin_velocities(ctx, case["x"], case["y"], case["u"], case["v"], fjord, lat["side"], 0)
    with pytest.raises(ValueError if kind == "arg" else _lib.IcelkError):
        VC.refused_call(lambda *a, **k: validate_velocities(ctx, *a, **k), change)
    after = bin_velocities(ctx, case["x"], case["y"], case["u"], case["v"], fjord, lat["side"], 0)
    assert sorted(before) == sorted(after) and sum(before["count"]) > 0
    for k in before:
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k


def test_day_refusals_leave_the_handle_usable(ctx, day):
    before = run_day(ctx, day, day["a"])
    for bad in (dict(threshold=0.0), dict(eps=float("nan")), dict(min_neighbours=0), dict(side=0.0)):
        with pytest.raises(ValueError):
            run_day(ctx, day, day["a"], validate=bad)
    with pytest.raises(_lib.IcelkError):                                 # a lattice of 2^40 cells
        run_day(ctx, day, day["a"], validate=dict(side=1e-3))
    after = run_day(ctx, day, day["a"])
    assert [n for n, _ in before] == [n for n, _ in after]
    for (_, a), (_, b) in zip(before, after):
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k

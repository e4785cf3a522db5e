#!/usr/bin/env python3
"""Generates tests/golden/s4_golden.npz by RUNNING THE REFERENCE'S OWN s4 (development container only):
`s4_postprocess_gridded_utm.combine_npzs`, `average_spatially_temporally` (viz 1, plot_num 1, Agg backend, the module
global `figure_workspace` pointed at a temporary directory, a small fjord outline file), `npz_to_csv`, `save_csv` and
`npz_to_mat`, on a folder of 30-minute window files:

- 2019-07-24: the files the reference's s3 wrote for the golden day (day_grid_golden.npz, run 0), so the chain
  s3 -> s4 rests on the reference's own files, the window with points and no kept cell included;
- 2019-07-25: three files, all without a kept cell (the daily period has windows and no data: six NaN);
- 2019-07-26, 27: no file (the daily period of the 26th selects nothing: the reference raises ValueError; that of the
  27th reaches into the morning of the 28th);
- 2019-07-28 .. 30: 48 seeded windows a day on the same grid, written with s3's keys and dtypes: values over five
  decades, counts up to 9e4, every kept cell in ~65 % of the windows -- except one cell that is in none of them and
  one that is in a single window (cells outside the outline are in no file of the run).
Calls recorded: the __main__ period (12:00 + 22 h) of every day 24 .. 30, the three seeded days as one period (144
windows > 128), a period of 5 windows, and the three-day period at coarseness 2, 3, 4, 8, 9 and 16 plus one day at
2 -- the golden day's grid is 9 rows x 14 cols, so every one of them pads the rows, the cols or both, and 16 leaves a
single coarse cell of 256 terms.
Committed: this script and the data; no reference source.
"""
import datetime as dt
import glob
import os
import sys
import tempfile

import matplotlib
matplotlib.use("Agg")
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "s4_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
import day_grid_golden  # noqa: E402

SEEDED_DAYS = (28, 29, 30)
EMPTY_WINDOWS = ("20190725_1300-1330", "20190725_1330-1400", "20190725_2000-2030")
COARSE = (2, 3, 4, 8, 9, 16)
NAME_FJORD = "GoldenFjord"


def day(d):
    return dt.datetime(2019, 7, d)


def stamp(t):
    return t.strftime("%Y-%m-%d %H:%M")


def window_file(grid, grid_size, ids, u, v, count):
    """A window file as s3 writes it (s3:441-445 through np.savez: lists become arrays)."""
    polygons, centers, indices, topleft, rows, cols = grid
    keep = set(int(k) for k in ids)
    r = dict(grid_size=grid_size, topleft=topleft, rows=rows, cols=cols, grid_id=[int(k) for k in ids],
             i=[indices[k][0] for k in ids], j=[indices[k][1] for k in ids], x=[centers[k][0] for k in ids],
             y=[centers[k][1] for k in ids], u=list(u), v=list(v), speed=list(np.hypot(u, v)),
             count=[int(c) for c in count], measured=[polygons[k] for k in ids],
             not_measured=[p for k, p in enumerate(polygons) if k not in keep])
    return {k: np.asanyarray(a) for k, a in r.items()}


def main():
    sys.path.insert(0, REF)
    import imports.tracking_misc as trm
    import s4_postprocess_gridded_utm as s4
    z0 = day_grid_golden.load()
    fjord = {"x": z0["fjord_x"], "y": z0["fjord_y"]}
    grid_size = int(z0["grid_size"])
    grid = trm.create_grid_across_fjord(fjord, grid_size)
    ncell = len(grid[2])
    golden_day = day_grid_golden.outputs(z0, 0)
    # the golden day measures every kept cell at least twice, so "never" and "once" hold for the seeded days: one kept
    # cell is in none of their windows, one in a single window (cells outside the outline are in no file at all)
    never, once = 73, 9
    rng = np.random.default_rng(2704)
    out = dict(never=np.array(never), once=np.array(once), grid_size=np.array(grid_size),
               grid_polygons=np.array(grid[0]), grid_centers=np.array(grid[1]), grid_indices=np.array(grid[2]),
               topleft=np.array(grid[3]), rows=np.array(grid[4]), cols=np.array(grid[5]), name_fjord=np.array(NAME_FJORD))
    names, off, cat = [], [0], {k: [] for k in ("grid_id", "u", "v", "count")}
    with tempfile.TemporaryDirectory() as tmp:
        folder, work = os.path.join(tmp, "run1"), os.path.join(tmp, "work")
        for d in (folder, work, os.path.join(work, "csv"), os.path.join(work, "csv1"), os.path.join(work, "csv2"),
                  os.path.join(work, "mat")):
            os.makedirs(d)
        for name, arrays in golden_day:
            np.savez(os.path.join(folder, name), **arrays)
        seeded = [(w, np.zeros(0, int)) for w in EMPTY_WINDOWS]
        once_at = (SEEDED_DAYS[1], 31)
        for d in SEEDED_DAYS:
            for w in range(48):
                t0 = day(d) + dt.timedelta(minutes=30 * w)
                ids = np.array([k for k in range(ncell) if k not in (never, once) and rng.random() < 0.65], int)
                if (d, w) == once_at:
                    ids = np.sort(np.append(ids, once))
                seeded.append((t0.strftime("%Y%m%d_%H%M") + (t0 + dt.timedelta(minutes=30)).strftime("-%H%M"), ids))
        for w, ids in seeded:
            n = len(ids)
            u = rng.normal(0.1, 0.3, n) * 10.0 ** rng.integers(-3, 2, n)
            v = rng.normal(-0.05, 0.2, n) * 10.0 ** rng.integers(-3, 2, n)
            count = np.where(rng.random(n) < 0.2, rng.integers(50001, 90000, n), rng.integers(4, 3000, n))
            name = "%s_30min_%dm.npz" % (w, grid_size)
            np.savez(os.path.join(folder, name), **window_file(grid, grid_size, ids, u, v, count))
            names.append(name)
            off.append(off[-1] + n)
            for k, a in zip(("grid_id", "u", "v", "count"), (ids, u, v, count)):
                cat[k].append(a)
        out["seed_names"], out["seed_off"] = np.array(names), np.array(off, np.int64)
        out["seed_grid_id"] = np.concatenate(cat["grid_id"]).astype(np.int64)
        out["seed_u"], out["seed_v"] = np.concatenate(cat["u"]), np.concatenate(cat["v"])
        out["seed_count"] = np.concatenate(cat["count"]).astype(np.int64)

        # ---- the cube
        s4.combine_npzs(folder, work, "cube.npz")
        with np.load(os.path.join(work, "cube.npz")) as z:
            cube = {k: z[k] for k in z.files}
        out["cube_keys"] = np.array(list(cube))
        for k, a in cube.items():
            out["cube_" + k] = a
        assert cube["u"].shape[:2] == (9, 14)    # every coarseness below pads rows, cols or both
        assert np.nanmax(cube["count"]) > 5e4

        # ---- the averages
        np.savez(os.path.join(tmp, "fjord_outline.npz"), **fjord)
        s4.figure_workspace = os.path.join(work, "figures")
        os.makedirs(s4.figure_workspace)
        three_days = (day(SEEDED_DAYS[0]), day(SEEDED_DAYS[-1] + 1))
        noon = lambda d: (day(d) + dt.timedelta(hours=12), day(d) + dt.timedelta(hours=34))   # noqa: E731
        calls = [noon(d) + (1,) for d in range(24, 31)]
        calls += [three_days + (1,), (day(28) + dt.timedelta(hours=3), day(28) + dt.timedelta(hours=5, minutes=30), 1)]
        calls += [three_days + (c,) for c in COARSE] + [noon(29) + (2,)]
        kinds = []
        for n, (start, end, coarseness) in enumerate(calls):
            try:
                r = s4.average_spatially_temporally(start, end, coarseness, cube, "call %02d" % n,
                                                    os.path.join(tmp, "fjord_outline.npz"), 1, 1)
            except ValueError:
                kinds.append("raises")
                continue
            if isinstance(r[0], float):
                assert all(np.isnan(q) for q in r)
                kinds.append("nan")
                continue
            kinds.append("ok")
            for key, a in zip(("x", "y", "u", "v", "count"), r):
                out["call_%02d_%s" % (n, key)] = np.array(a)
            out["call_%02d_time_str" % n] = np.array(r[5])
            nsel = int(((cube["time"] >= trm.datetime_to_epoch(start)) & (cube["time"] < trm.datetime_to_epoch(end))).sum())
            out["call_%02d_nsel" % n] = np.array(nsel)
            # the __main__ loop's flip-back and save_csv, for one day at coarseness 1 and 2
            if (start, end) == noon(29):
                x, y, u, v, count, time_str = r
                y, u, v = np.flipud(y), np.flipud(u), np.flipud(v)
                target = os.path.join(work, "csv%d" % coarseness)
                s4.save_csv(x, y, u, v, count, time_str, target, NAME_FJORD)
                store_csv(out, "savecsv%d" % coarseness, target)
        out["call_start"] = np.array([stamp(c[0]) for c in calls])
        out["call_end"] = np.array([stamp(c[1]) for c in calls])
        out["call_coarseness"] = np.array([c[2] for c in calls])
        out["call_kind"] = np.array(kinds)
        assert kinds[:3] == ["ok", "nan", "raises"] and all(k == "ok" for k in kinds[3:]), kinds
        assert int(out["call_07_nsel"]) > 128 and int(out["call_08_nsel"]) < 8

        # ---- the exports: csv of the first 16 windows (golden day, empty windows, seeded), the cube as .mat
        head = {k: (a[:, :, :16] if a.ndim == 3 else a[:16] if k.startswith("time") else a) for k, a in cube.items()}
        s4.npz_to_csv(head, os.path.join(work, "csv"), NAME_FJORD)
        out["csv_windows"] = np.array(16)
        store_csv(out, "npzcsv", os.path.join(work, "csv"))
        s4.npz_to_mat(os.path.join(work, "cube.npz"), os.path.join(work, "mat"))
        import scipy.io
        mat = scipy.io.loadmat(os.path.join(work, "mat", "cube.mat"))
        out["mat_keys"] = np.array(sorted(k for k in mat if not k.startswith("__")))
        # loadmat returns the cube's own arrays (time = time_matlab as a row): checked here, and only the shapes are
        # stored, not a second copy of the cube
        for k in out["mat_keys"]:
            a, c = mat[str(k)], cube["time_matlab" if k == "time" else str(k)]
            assert a.dtype == c.dtype and np.array_equal(a.ravel(), c.ravel(), equal_nan=True)
            out["mat_%s_shape" % k] = np.array(a.shape)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; cube", cube["u"].shape, "calls", kinds, "numpy", np.__version__)


def store_csv(out, prefix, folder):
    files = sorted(glob.glob(os.path.join(folder, "*.csv")))
    out[prefix + "_names"] = np.array([os.path.basename(f) for f in files])
    for k, f in enumerate(files):
        out["%s_%03d" % (prefix, k)] = np.frombuffer(open(f, "rb").read(), np.uint8)


if __name__ == "__main__":
    main()

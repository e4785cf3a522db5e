#!/usr/bin/env python3
"""Generates tests/golden/day_grid_golden.npz by RUNNING THE REFERENCE'S DAY DRIVER (development container only):
`s3_utm_to_gridded_utm.utm_to_gridded_utm` (s3:222-446, plot_switch 0) on one synthetic day, with 30-minute,
full-day (24.0) and 1/7-hour windows (514.2857... s: float accumulation and microseconds in the window edges,
names with time_diff 8; where a drifted window crosses an hour with end microseconds below the start's, the end's
hour drops out, and a window inside one hour with end microseconds below its start's loads no file at all).

The day: cameras camA (no drift row), camB (drift 12.3 s + 4 days x 0.05 s = 12.5 s: fractional, bounds truncate),
camC (drift 95.2 s: its windows reach back into the previous hour's file), camD (two matching schedule rows: skipped)
and camE (scheduled, no files).  camA lacks its 12:00 file; every file holds some points of the neighbouring hours (in
no window when that window does not load the file); camB's 13:00 file lies outside the grid, so the last window has
points and no kept cell; many points lie exactly on cell edges and corners.  Hour files are written as s2 writes them
(int64 epoch times).

What the function READS is supplied, not emulated: `pandas.read_excel` returns the in-memory tables below.  What it
FORMS is recorded by wrapping the reference's own helpers while it runs: `trm.correct_time_drift` (per camera and
window, 0 where it raises, as s3:306-310 has it), `trm.return_velocities_by_time` (arguments and selection),
`trm.datetime_to_epoch` (the epoch bounds), `pandas.date_range` inside it (the hours) and `glob.glob` (the files
found), and `np.savez` (names in writing order; each file is read back as written).
Committed: this script and the data; no reference source.
"""
import datetime as dt
import glob
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "day_grid_golden.npz")

DAY = dt.datetime(2019, 7, 24)
CAMNAMES = ["camA", "camB", "camC", "camD", "camE"]
ROW = dict(start_day=20190701, end_day=20190831)
SCHEDULE = [dict(ROW, camera="camA", start_time="10:00", tracking_duration=3.0),
            dict(ROW, camera="camB", start_time="10:30", tracking_duration=3.5),
            dict(ROW, camera="camC", start_time="10:15", tracking_duration=3.0),
            dict(ROW, camera="camD", start_time="10:00", tracking_duration=2.0),
            dict(ROW, camera="camD", start_time="11:00", tracking_duration=1.0),
            dict(ROW, camera="camE", start_time="09:00", tracking_duration=2.0)]
DRIFTS = [dict(cam="camB", start_date=20190720, end_date=20190731, drift_start_sec=12.3, drift_pday_sec=0.05),
          dict(cam="camC", start_date=20190701, end_date=20190731, drift_start_sec=95.2, drift_pday_sec=0.0),
          dict(cam="camA", start_date=20190724, end_date=20190731, drift_start_sec=7.0, drift_pday_sec=1.0)]  # not < day
FILES = {"camA": (9, 10, 11, 13), "camB": (10, 11, 12, 13), "camC": (9, 10, 11, 12)}
WINDOWS = (0.5, 24.0, 1 / 7.0)
SPACING, THRESHOLD = 300, 3
N_PER_FILE = 900


def hour_file(rng, fjord, camname, hr, epoch):
    t0 = DAY + dt.timedelta(hours=hr)
    e0 = epoch(t0)
    n = N_PER_FILE
    tt = rng.integers(e0, e0 + 3600, n)
    k = n // 7
    tt[:k] = e0 + rng.integers(-2400, 0, k)                    # points of the previous hour
    tt[k:2 * k] = e0 + 3600 + rng.integers(0, 2400, k)         # and of the next
    if camname == "camA" and hr == 13:
        tt = e0 + rng.integers(0, 25 * 60, n)                  # nothing at or after 13:30
    tt = np.sort(tt).astype(np.int64)
    left, top = min(fjord["x"]), max(fjord["y"])
    x = np.round(rng.uniform(left - 200, max(fjord["x"]) + 200, n) * 64) / 64
    y = np.round(rng.uniform(min(fjord["y"]) - 200, top + 200, n) * 64) / 64
    e = n // 5
    x[:e] = left + SPACING * rng.integers(0, 12, e)                               # on vertical edges
    y[e:2 * e] = top - SPACING * rng.integers(0, 10, e)                           # on horizontal edges
    x[2 * e:3 * e] = left + SPACING * rng.integers(0, 12, e)                      # on corners
    y[2 * e:3 * e] = top - SPACING * rng.integers(0, 10, e)
    if camname == "camB" and hr == 13:
        x = max(fjord["x"]) + 500 + rng.uniform(0, 100, n)                        # outside every cell
    u = rng.normal(0.1, 0.3, n) * 10.0 ** rng.integers(-3, 2, n)
    v = rng.normal(-0.05, 0.2, n) * 10.0 ** rng.integers(-3, 2, n)
    return t0.strftime("%Y%m%d_%H00") + "_60s_utm.npz", dict(x=x, y=y, u=u, v=v, speed=np.hypot(u, v), time=tt)


def stamp(t):
    return t.strftime("%Y-%m-%d %H:%M:%S.%f")


def main():
    sys.path.insert(0, REF)
    import imports.tracking_misc as trm
    import s3_utm_to_gridded_utm as s3
    tables = {"parameter_file.xlsx": pd.DataFrame(SCHEDULE), "camera_time_drifts.xlsx": pd.DataFrame(DRIFTS)}
    rng = np.random.default_rng(2407)
    out = {}
    ang = np.sort(rng.uniform(0, 2 * np.pi, 30))
    rad = rng.uniform(1100, 1700, 30)
    fjord = dict(x=497000.0 + np.round(1.3 * rad * np.cos(ang), 1), y=6521000.0 + np.round(rad * np.sin(ang), 1))
    out["fjord_x"], out["fjord_y"] = fjord["x"], fjord["y"]
    out["schedule"] = np.array(json.dumps(SCHEDULE))
    out["clock_drifts"] = np.array(json.dumps(DRIFTS))
    out["camnames"] = np.array(CAMNAMES)
    out["day"] = np.array(DAY.strftime("%Y%m%d"))
    out["time_windows"] = np.array(WINDOWS)
    out["grid_size"], out["observation_threshold"] = np.array(SPACING), np.array(THRESHOLD)

    real = dict(read_excel=pd.read_excel, date_range=pd.date_range, savez=np.savez, glob=glob.glob,
                drift=trm.correct_time_drift, select=trm.return_velocities_by_time, epoch=trm.datetime_to_epoch)
    log = {}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            head = os.path.join(tmp, "out")
            k = 0
            for camname in CAMNAMES:
                ws = os.path.join(head, camname, "utm")
                os.makedirs(ws)
                for hr in FILES.get(camname, ()):
                    name, arrays = hour_file(rng, fjord, camname, hr, real["epoch"])
                    np.savez(os.path.join(ws, name), **arrays)
                    out["in_%02d_cam" % k], out["in_%02d_name" % k] = np.array(camname), np.array(name)
                    for key, a in arrays.items():
                        out["in_%02d_%s" % (k, key)] = a
                    k += 1
            out["in_n"] = np.array(k)
            np.savez(os.path.join(tmp, "fjord_outline.npz"), **fjord)

            pd.read_excel = lambda path, *a, **kw: tables[os.path.basename(str(path))].copy()

            def drift(camname, day_str, table):
                try:
                    r = real["drift"](camname, day_str, table)
                except Exception:
                    log["drifts"].append((camname, 0))
                    raise
                log["drifts"].append((camname, float(r)))
                return r

            def select(workspace, start, end):
                log["call"] = dict(cam=os.path.basename(os.path.dirname(workspace)), start=stamp(start),
                                   end=stamp(end), epochs=[], hours=[], found=[])
                r = real["select"](workspace, start, end)
                t = r[5]
                log["call"].update(n=len(t), tmin=float(t.min()) if len(t) else 0.0,
                                   tmax=float(t.max()) if len(t) else 0.0)
                log["calls"].append(log.pop("call"))
                return r

            def epoch(t):
                e = real["epoch"](t)
                if "call" in log:
                    log["call"]["epochs"].append(e)
                return e

            def date_range(*a, **kw):
                r = real["date_range"](*a, **kw)
                if "call" in log:
                    log["call"]["hours"] = [stamp(h) for h in r]
                return r

            def globber(pattern, *a, **kw):
                r = real["glob"](pattern, *a, **kw)
                if "call" in log:
                    log["call"]["found"].append(os.path.basename(r[0]) if r else "")
                return r

            def savez(path, **arrays):
                real["savez"](path, **arrays)
                with np.load(path) as z:
                    log["saved"].append((os.path.basename(path), {key: z[key] for key in z.files}))

            trm.correct_time_drift, trm.return_velocities_by_time, trm.datetime_to_epoch = drift, select, epoch
            pd.date_range, np.savez, glob.glob = date_range, savez, globber
            for r, tw in enumerate(WINDOWS):
                log.update(drifts=[], calls=[], saved=[])
                target = os.path.join(tmp, "gridded_%d" % r)
                os.makedirs(target)
                args = (CAMNAMES, head, "utm", target, tmp, os.path.join(tmp, "parameter_file.xlsx"),
                        os.path.join(tmp, "camera_time_drifts.xlsx"), os.path.join(tmp, "fjord_outline.npz"), DAY,
                        tw, SPACING, 0.5, THRESHOLD, 0)
                s3.utm_to_gridded_utm(args)
                # camnames_filtered: the cameras correct_time_drift sees in the first window; then windows in order
                names = []
                for cam, _ in log["drifts"]:
                    if cam in names:
                        break
                    names.append(cam)
                nw = len(log["drifts"]) // len(names)
                out["r%d_cameras" % r] = np.array(names)
                out["r%d_corrections" % r] = np.array([c for _, c in log["drifts"][:len(names)]], np.float64)
                assert all(log["drifts"][w * len(names) + i] == log["drifts"][i] for w in range(nw)
                           for i in range(len(names)))
                calls = log["calls"]
                cams_called = sorted({c["cam"] for c in calls}, key=names.index)
                assert len(calls) == nw * len(cams_called)
                out["r%d_called" % r] = np.array(cams_called)
                out["r%d_n_windows" % r] = np.array(nw)
                # per (window, called camera): corrected bounds, epochs, hours, files found, selection
                out["r%d_starts" % r] = np.array([c["start"] for c in calls])
                out["r%d_ends" % r] = np.array([c["end"] for c in calls])
                out["r%d_epochs" % r] = np.array([c["epochs"] for c in calls], np.int64)
                out["r%d_hours" % r] = np.array(json.dumps([c["hours"] for c in calls]))
                out["r%d_found" % r] = np.array(json.dumps([c["found"] for c in calls]))
                out["r%d_sel_n" % r] = np.array([c["n"] for c in calls], np.int64)
                out["r%d_sel_tmin" % r] = np.array([c["tmin"] for c in calls], np.float64)
                out["r%d_sel_tmax" % r] = np.array([c["tmax"] for c in calls], np.float64)
                out["r%d_n_out" % r] = np.array(len(log["saved"]))
                for fi, (name, z) in enumerate(log["saved"]):
                    out["r%d_%02d_name" % (r, fi)] = np.array(name)
                    for key, a in z.items():
                        out["r%d_%02d_%s" % (r, fi, key)] = a
                print("time_window %.6f: %d windows, %d files, %d selected" % (tw, nw, len(log["saved"]),
                                                                             int(out["r%d_sel_n" % r].sum())))
                if tw == 1 / 7.0:
                    st = [dt.datetime.strptime(s, "%Y-%m-%d %H:%M:%S.%f") for s in out["r%d_starts" % r]]
                    en = [dt.datetime.strptime(s, "%Y-%m-%d %H:%M:%S.%f") for s in out["r%d_ends" % r]]
                    assert any(e.microsecond < s.microsecond for s, e in zip(st, en))
    finally:
        trm.correct_time_drift, trm.return_velocities_by_time = real["drift"], real["select"]
        trm.datetime_to_epoch = real["epoch"]
        pd.read_excel, pd.date_range, np.savez, glob.glob = (real["read_excel"], real["date_range"], real["savez"],
                                                             real["glob"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; numpy", np.__version__, "pandas", pd.__version__)


if __name__ == "__main__":
    main()

"""tests/golden/s4_golden.npz (made by tests/golden/make_s4_golden.py from the reference's own s4): the folder of
window files rebuilt on disk, the cube the reference stacked from it, and its recorded calls and exports."""
import datetime as dt
import os

import numpy as np

import day_grid_golden

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s4_golden.npz")
CUBE_KEYS = ("x", "y", "i", "j", "u", "v", "speed", "count", "time", "time_matlab")


def load():
    return np.load(GOLD, allow_pickle=False)


def seeded_file(z, k):
    """(name, arrays) of seeded window file k, with the keys and dtypes s3 writes (lists through np.savez)."""
    a, b = int(z["seed_off"][k]), int(z["seed_off"][k + 1])
    ids = z["seed_grid_id"][a:b]
    polygons, centers, indices = z["grid_polygons"], z["grid_centers"], z["grid_indices"]
    keep = set(int(q) for q in ids)
    u, v = z["seed_u"][a:b], z["seed_v"][a:b]
    r = dict(grid_size=int(z["grid_size"]), topleft=[float(q) for q in z["topleft"]], rows=int(z["rows"]),
             cols=int(z["cols"]), grid_id=[int(q) for q in ids], i=[int(indices[q][0]) for q in ids],
             j=[int(indices[q][1]) for q in ids], x=[centers[q][0] for q in ids], y=[centers[q][1] for q in ids],
             u=list(u), v=list(v), speed=list(np.hypot(u, v)), count=[int(c) for c in z["seed_count"][a:b]],
             measured=[polygons[q] for q in ids],
             not_measured=[p for q, p in enumerate(polygons) if q not in keep])
    return str(z["seed_names"][k]), {key: np.asanyarray(val) for key, val in r.items()}


def build_folder(z, folder, golden_day=True):
    """The run folder the reference's combine_npzs read: the golden day's 30-minute files as the reference's s3
    wrote them (unless `golden_day` is False: the caller supplies them) and the seeded files."""
    if golden_day:
        for name, arrays in day_grid_golden.outputs(day_grid_golden.load(), 0):
            np.savez(os.path.join(folder, name), **arrays)
    for k in range(len(z["seed_names"])):
        name, arrays = seeded_file(z, k)
        np.savez(os.path.join(folder, name), **arrays)


def cube(z):
    return {k: z["cube_" + k] for k in CUBE_KEYS}


def calls(z):
    """The recorded calls of average_spatially_temporally: dict(start, end, coarseness, kind ('ok', 'nan': six NaN,
    'raises': ValueError), and for 'ok' x, y, u, v, count, time_str, nsel)."""
    out = []
    for n, kind in enumerate(z["call_kind"]):
        c = dict(start=dt.datetime.strptime(str(z["call_start"][n]), "%Y-%m-%d %H:%M"),
                 end=dt.datetime.strptime(str(z["call_end"][n]), "%Y-%m-%d %H:%M"),
                 coarseness=int(z["call_coarseness"][n]), kind=str(kind))
        if c["kind"] == "ok":
            for key in ("x", "y", "u", "v", "count"):
                c[key] = z["call_%02d_%s" % (n, key)]
            c["time_str"] = str(z["call_%02d_time_str" % n])
            c["nsel"] = int(z["call_%02d_nsel" % n])
        out.append(c)
    return out


def csv_files(z, prefix):
    """{file name: bytes} of a recorded csv export ('npzcsv', 'savecsv1', 'savecsv2')."""
    return {str(name): z["%s_%03d" % (prefix, k)].tobytes() for k, name in enumerate(z[prefix + "_names"])}


def same_floats(a, b):
    """Bit for bit on every non-NaN float64, NaN in the same places (sign and payload of a NaN are not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float64 or b.dtype != np.float64:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))

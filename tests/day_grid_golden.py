"""tests/golden/day_grid_golden.npz (made by tests/golden/make_day_grid_golden.py from the reference's own
utm_to_gridded_utm): the day's inputs rebuilt on disk, and its recorded runs."""
import datetime as dt
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "day_grid_golden.npz")
OUT_KEYS = ("grid_size", "topleft", "rows", "cols", "grid_id", "i", "j", "x", "y", "u", "v", "speed", "count",
            "measured", "not_measured")


def load():
    return np.load(GOLD, allow_pickle=False)


def build_tree(z, root):
    """The camera workspaces root/<camera>/utm with the golden's hourly files; every camera named gets a folder."""
    for cam in z["camnames"]:
        os.makedirs(os.path.join(root, str(cam), "utm"), exist_ok=True)
    for k in range(int(z["in_n"])):
        arrays = {key: z["in_%02d_%s" % (k, key)] for key in ("x", "y", "u", "v", "speed", "time")}
        np.savez(os.path.join(root, str(z["in_%02d_cam" % k]), "utm", str(z["in_%02d_name" % k])), **arrays)


def args(z):
    """(camnames, schedule, clock_drifts, fjord, day, grid_size, observation_threshold) as a user passes them."""
    return ([str(c) for c in z["camnames"]], json.loads(str(z["schedule"])), json.loads(str(z["clock_drifts"])),
            {"x": z["fjord_x"], "y": z["fjord_y"]}, dt.datetime.strptime(str(z["day"]), "%Y%m%d"),
            int(z["grid_size"]), int(z["observation_threshold"]))


def outputs(z, r):
    """[(name, {key: array})] run r of the reference wrote, in writing order."""
    return [(str(z["r%d_%02d_name" % (r, f)]), {k: z["r%d_%02d_%s" % (r, f, k)] for k in OUT_KEYS})
            for f in range(int(z["r%d_n_out" % r]))]


def parse(stamp):
    return dt.datetime.strptime(stamp, "%Y-%m-%d %H:%M:%S.%f")

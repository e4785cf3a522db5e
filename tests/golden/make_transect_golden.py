#!/usr/bin/env python3
"""Generates tests/golden/transect_golden.npz (development container only: needs /root/reference, matplotlib, pandas).

(a) RUNS THE REFERENCE: the box geometry of `imports.tracking_misc` (tracking_misc.py:76-185), imported from
    /root/reference -- azimuth_transect, locate_points_along_transect, create_squares_rot, create_squares_along_transect,
    create_squares_around_mooring -- on the profiles and moorings of CASES below.
(b) The loop a user of the reference runs over such boxes is not in the reference as a function; it is restated HERE with
    the third-party calls it makes -- matplotlib.path.Path(poly).contains_points(points), np.sum(...) / n, np.hypot --
    on a few hundred velocities that include the boxes' vertices and the midpoints of their shared edges.  This pins the
    primitives' semantics (tie rule, summation order), as make_grid_golden.py does for the fjord grid.
Committed: this script and the data; no reference source.
"""
import os
import sys

import matplotlib.path as mplPath
import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transect_golden.npz")

# name: (p1, p2, spacing, width).  Coordinates >= 1e5, offsets <= 5e3 (the margin the host test allows is derived for these).
PROFILES = {
    "we": ((436000.0, 6523000.0), (437050.0, 6523000.0), 200.0, 600.0),
    "ew": ((437050.0, 6523000.0), (436000.0, 6523000.0), 200.0, 600.0),
    "diag": ((436000.0, 6523000.0), (437000.0, 6524000.0), 200.0, 600.0),
    "short": ((436000.0, 6523000.0), (436100.0, 6523050.0), 200.0, 300.0),       # shorter than a spacing
    "exact": ((436000.0, 6523000.0), (436600.0, 6523800.0), 250.0, 400.0),       # 1000 m: 4 spacings exactly
    "plus07": ((436000.0, 6523000.0), (436705.0, 6523940.0), 250.0, 400.0),      # 1175 m: 4.7 spacings
}
# name: (coordinates, azimuth in degrees, width, nr)
MOORINGS = {
    "moor7": ((436500.0, 6523500.0), -45, 100, 7),
    "moor4": ((436500.0, 6523500.0), -45, 100, 4),          # floor(4 / 2) on each side: 5 x 5
    "moor1": ((436500.0, 6523500.0), 30, 150, 1),
}
BINNED = ("diag", "moor7")


def tie_points(polys):
    """the boxes' vertices and the midpoint of every box's leading edge (the edge it shares with the next box)"""
    pts = [v for poly in polys for v in poly]
    pts += [(0.5 * (poly[0][0] + poly[1][0]), 0.5 * (poly[0][1] + poly[1][1])) for poly in polys]
    return np.array(pts, np.float64)


def main():
    sys.path.insert(0, REF)
    import imports.tracking_misc as trm
    out = {"profile_names": np.array(list(PROFILES)), "mooring_names": np.array(list(MOORINGS)), "binned_names": np.array(BINNED)}
    boxes = {}
    for name, (p1, p2, spacing, width) in PROFILES.items():
        profile = {"x": np.array([p1[0], 0.5 * (p1[0] + p2[0]) + 17.0, p2[0]]), "y": np.array([p1[1], 0.5 * (p1[1] + p2[1]) - 5.0, p2[1]])}
        polys, points, distances = trm.create_squares_along_transect(profile, spacing, width)
        located = trm.locate_points_along_transect(np.array(p1), np.array(p2), spacing)
        azimuth = trm.azimuth_transect(np.array(p1), np.array(p2))
        out.update({name + "_profile_x": profile["x"], name + "_profile_y": profile["y"], name + "_spacing": np.float64(spacing),
                    name + "_width": np.float64(width), name + "_polygons": np.array(polys, np.float64),
                    name + "_points": np.array(points, np.float64), name + "_distances": np.array(distances, np.float64),
                    name + "_located_points": np.array(located[0], np.float64),
                    name + "_located_distances": np.array(located[1], np.float64), name + "_azimuth": np.float64(azimuth),
                    name + "_rot_first": np.array(trm.create_squares_rot([points[0][0], points[0][1]], spacing, width, azimuth), np.float64)})
        boxes[name] = (polys, azimuth)
    for name, (coord, azimuth, width, nr) in MOORINGS.items():
        polys, centers, distances = trm.create_squares_around_mooring(list(coord), azimuth=azimuth, width=width, nr=nr)
        out.update({name + "_coord": np.array(coord), name + "_azimuth_deg": np.float64(azimuth), name + "_width": np.float64(width),
                    name + "_nr": np.int64(nr), name + "_polygons": np.array(polys, np.float64),
                    name + "_centers": np.array(centers, np.float64), name + "_distances": np.array(distances, np.float64)})
        boxes[name] = (polys, np.radians(azimuth))
    # defaults of the mooring call
    polys, centers, distances = trm.create_squares_around_mooring([436500.0, 6523500.0])
    out.update(moor_default_polygons=np.array(polys, np.float64), moor_default_centers=np.array(centers, np.float64),
               moor_default_distances=np.array(distances, np.float64))

    # velocities: a cloud over the boxes of BINNED + the tie points of both
    rng = np.random.default_rng(2024)
    n = 360
    x = rng.uniform(435600.0, 437400.0, n)
    y = rng.uniform(6522600.0, 6524400.0, n)
    k = n // 3
    x[:k] = rng.uniform(436200.0, 436800.0, k)                                # over the mooring lattice
    y[:k] = rng.uniform(6523200.0, 6523800.0, k)
    ties = np.concatenate([tie_points(boxes["diag"][0]), tie_points(boxes["moor7"][0])[::5], tie_points(boxes["we"][0])])
    x, y = np.concatenate([x, ties[:, 0]]), np.concatenate([y, ties[:, 1]])
    order = rng.permutation(len(x))
    x, y = x[order], y[order]
    u = rng.normal(0.1, 0.3, len(x)) * 10.0 ** rng.integers(-3, 2, len(x))
    v = rng.normal(-0.05, 0.2, len(x)) * 10.0 ** rng.integers(-3, 2, len(x))
    points = np.vstack((x, y)).T
    out.update(px=x, py=y, pu=u, pv=v, n_ties_diag=np.int64(len(tie_points(boxes["diag"][0]))))
    for name in BINNED:
        polys = boxes[name][0]
        member = np.array([mplPath.Path(poly).contains_points(points) for poly in polys])
        cnt = member.sum(1)
        mean_u, mean_v, speed = (np.full(len(polys), np.nan) for _ in range(3))
        for b in range(len(polys)):
            if cnt[b] > 0:
                mean_u[b] = np.sum(u[member[b]]) / cnt[b]
                mean_v[b] = np.sum(v[member[b]]) / cnt[b]
                speed[b] = np.hypot(mean_u[b], mean_v[b])
        hits = member.sum(0)
        print(name, "boxes", len(polys), "counts", list(cnt), "points with 0 / 1 / 2 hits", [int((hits == h).sum()) for h in (0, 1, 2)])
        assert set(hits) >= {0, 1} and hits.max() <= 2 and (cnt > 0).sum() >= 2
        out.update({name + "_member": member, name + "_count": cnt.astype(np.int64), name + "_mean_u": mean_u,
                    name + "_mean_v": mean_v, name + "_speed": speed})
    # the tie points of the diagonal transect alone: vertices and shared-edge midpoints in 0, 1 and 2 boxes
    diag_ties = tie_points(boxes["diag"][0])
    th = np.array([mplPath.Path(poly).contains_points(diag_ties) for poly in boxes["diag"][0]]).sum(0)
    print("diag ties", len(diag_ties), "with 0 / 1 / 2 hits", [int((th == h).sum()) for h in (0, 1, 2)])
    all_hits = out["diag_member"].sum(0)
    assert {0, 1, 2} <= set(all_hits), "the fixture needs points in no box, in one and in two"
    np.savez_compressed(OUT, **out)
    import matplotlib
    print("wrote", OUT, os.path.getsize(OUT), "bytes; numpy", np.__version__, "matplotlib", matplotlib.__version__)


if __name__ == "__main__":
    main()

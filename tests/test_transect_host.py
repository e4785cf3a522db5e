"""Host, no GPU: the box geometry of transect.py against what the reference's own functions returned
(tests/golden/transect_golden.npz, made by tests/golden/make_transect_golden.py), the packing of a box list, and the
refusals of the new ABI that need no handle.

Counts, distances and shapes are compared exactly.  Coordinates may differ by 2 * np.spacing(|coordinate|): the
reference rotates with np.dot (BLAS), the package writes the products and sums out.  The two differ by at most 1 ulp of
the half extent, libm's cos and sin by about 1 ulp; with offsets <= 5e3 on coordinates >= 1e5 that is far below one
spacing of the coordinate, so the rounded sum centre + offset moves by at most one step, and two are allowed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iceberg_tracking_code_amd as pkg
from iceberg_tracking_code_amd import _lib, transect

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transect_golden.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD, allow_pickle=False)


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(want) >= 1e5), "the margin is derived for UTM-sized coordinates"
    return bool(np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want))))


def test_fixture_ranges(z):
    """the fixture stays where the margin was derived: coordinates >= 1e5, offsets <= 5e3; ties in 0, 1 and 2 boxes"""
    for name in list(z["profile_names"]) + list(z["mooring_names"]):
        poly = z[name + "_polygons"]
        assert poly.min() >= 1e5 and np.abs(poly - poly.mean((0, 1))).max() <= 5e3
    assert {0, 1, 2} <= set(z["diag_member"].sum(0))


def test_profiles(z):
    for name in z["profile_names"]:
        profile = {"x": z[name + "_profile_x"], "y": z[name + "_profile_y"]}
        spacing, width = float(z[name + "_spacing"]), float(z[name + "_width"])
        p1, p2 = np.array((profile["x"][0], profile["y"][0])), np.array((profile["x"][-1], profile["y"][-1]))
        out = pkg.create_squares_along_transect(profile, spacing, width)
        assert isinstance(out, list) and len(out) == 3
        polys, points, distances = out
        want = z[name + "_polygons"]
        assert len(polys) == len(points) == len(distances) == len(want), name
        assert all(isinstance(p, list) and len(p) == 4 and all(isinstance(q, tuple) and len(q) == 2 for q in p) for p in polys)
        assert np.array(distances).tobytes() == z[name + "_distances"].tobytes(), name
        assert close(polys, want), name
        assert np.array(points, np.float64).tobytes() == z[name + "_points"].tobytes(), name
        located = pkg.locate_points_along_transect(p1, p2, spacing)
        assert np.array(located[0], np.float64).tobytes() == z[name + "_located_points"].tobytes()
        assert np.array(located[1], np.float64).tobytes() == z[name + "_located_distances"].tobytes()
        assert np.float64(pkg.azimuth_transect(p1, p2)).tobytes() == z[name + "_azimuth"].tobytes()
        assert close(pkg.create_squares_rot([points[0][0], points[0][1]], spacing, width, float(z[name + "_azimuth"])),
                     z[name + "_rot_first"])


def test_count_rule(z):
    """np.ceil((length + 0.3 * dist) / dist): 4 spacings exactly give 5 boxes, 4.7 give 5, a profile shorter than a spacing 1"""
    assert [len(z[k + "_polygons"]) for k in ("exact", "plus07", "short", "diag", "we", "ew")] == [5, 5, 1, 8, 6, 6]
    for name, want in (("exact", 5), ("plus07", 5), ("short", 1)):
        profile = {"x": z[name + "_profile_x"], "y": z[name + "_profile_y"]}
        assert len(pkg.create_squares_along_transect(profile, float(z[name + "_spacing"]), float(z[name + "_width"]))[0]) == want


def test_moorings(z):
    for name in z["mooring_names"]:
        coord, az, width, nr = list(z[name + "_coord"]), float(z[name + "_azimuth_deg"]), float(z[name + "_width"]), int(z[name + "_nr"])
        polys, centers, distances = pkg.create_squares_around_mooring(coord, azimuth=az, width=width, nr=nr)
        side = 2 * (nr // 2) + 1
        assert len(polys) == len(centers) == len(distances) == side * side == len(z[name + "_polygons"]), name
        assert np.array(distances, np.float64).tobytes() == z[name + "_distances"].tobytes()
        assert np.array(centers, np.float64).tobytes() == z[name + "_centers"].tobytes()
        assert close(polys, z[name + "_polygons"]), name
    assert len(z["moor4_polygons"]) == 25 and len(z["moor1_polygons"]) == 1
    polys, centers, distances = pkg.create_squares_around_mooring([436500.0, 6523500.0])
    assert close(polys, z["moor_default_polygons"]) and np.array(distances, np.float64).tobytes() == z["moor_default_distances"].tobytes()


def test_rotation_is_written_out():
    """the vertex offsets are a*c + b*(-s) and a*s + b*c in that order, bit for bit, and height lies along the azimuth"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        cx, cy = rng.uniform(1e5, 7e6, 2)
        h, w, rot = rng.uniform(1, 5e3), rng.uniform(1, 5e3), rng.uniform(-np.pi, np.pi)
        c, s = np.cos(rot), np.sin(rot)
        want = [(cx + (a * c + b * (-s)), cy + (a * s + b * c)) for a, b in
                ((0.5 * h, 0.5 * w), (0.5 * h, -0.5 * w), (-0.5 * h, -0.5 * w), (-0.5 * h, 0.5 * w))]
        assert np.array(pkg.create_squares_rot([cx, cy], h, w, rot)).tobytes() == np.array(want).tobytes()
    poly = np.array(pkg.create_squares_rot([1e5, 2e5], 10.0, 2.0, 0.0))
    assert np.ptp(poly[:, 0]) == 10.0 and np.ptp(poly[:, 1]) == 2.0


def test_box_set(z):
    profile = {"x": z["diag_profile_x"], "y": z["diag_profile_y"]}
    b = pkg.BoxSet.along_transect(profile, 200.0, 600.0, name="gate")
    assert len(b) == 8 and b.name == "gate" and b.azimuth == float(z["diag_azimuth"]) and b.centers.shape == (8, 2)
    xy, off = b.packed()
    assert xy.shape == (32, 2) and xy.dtype == np.float64 and list(off) == list(range(0, 33, 4)) and off.dtype == np.int32
    assert b.polygon_array().shape == (8, 4, 2)
    m = pkg.BoxSet.around_mooring([436500.0, 6523500.0], nr=4)
    assert len(m) == 25 and m.azimuth == np.radians(-45) and m.distances.shape == (25, 2)
    ragged = pkg.BoxSet([[(0, 0), (1, 0), (0, 1)], [(0, 0), (1, 0), (1, 1), (0, 1)]])
    assert list(ragged.packed()[1]) == [0, 3, 7] and ragged.polygon_array().shape == (7, 2)
    with pytest.raises(ValueError):
        transect._BoxArgs(b, "fjord")


def boxes_struct(polys):
    b = pkg.BoxSet(polys)
    xy, off = b.packed()
    return _lib.Boxes(xy.ctypes.data_as(_lib.f64p), off.ctypes.data_as(_lib.i32p), len(b)), (xy, off)


SQUARE = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]


def test_box_list_refusals_need_no_handle():
    lib = _lib.load()
    st, keep = boxes_struct([SQUARE, SQUARE[:3]])
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.OK
    assert lib.icelk_boxes_check(None) == _lib.EARG
    st, keep = boxes_struct([SQUARE] * 1024)
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.ECAP                  # 4096 vertices
    st, keep = boxes_struct([SQUARE[:3]] * 1024)
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.ECAP                  # 3072 vertices
    st, keep = boxes_struct([SQUARE[:3]] * 682 + [SQUARE[:2] + [(0.5, 0.5)]])
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.ECAP                  # 2049 vertices
    st, keep = boxes_struct([SQUARE[:3]] * 682 + [SQUARE[:2]])
    assert keep[1][-1] == 2048 and lib.icelk_boxes_check(C.byref(st)) == _lib.EARG       # 2048 vertices, a polygon of two
    st, keep = boxes_struct([SQUARE[:3]] * 1025)
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.ECAP                  # 1025 boxes
    st, keep = boxes_struct([SQUARE, SQUARE[:2]])
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG                  # a polygon of two vertices
    for bad in (np.nan, np.inf, -np.inf):
        st, keep = boxes_struct([SQUARE, [(0.0, 0.0), (1.0, bad), (1.0, 1.0)]])
        assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG              # a vertex that is not finite
    st, keep = boxes_struct([SQUARE, SQUARE])
    keep[1][0] = 1
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG                  # offsets do not start at 0
    keep[1][:] = [0, 8, 4]
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG                  # offsets descend
    st = _lib.Boxes(None, None, 1)
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG
    st, keep = boxes_struct([SQUARE])
    st.nboxes = 0
    assert lib.icelk_boxes_check(C.byref(st)) == _lib.EARG


def test_entry_points_without_a_handle():
    lib = _lib.load()
    st, keep = boxes_struct([SQUARE])
    a = np.zeros(4)
    cnt = np.zeros(1, np.int32)
    f = lambda q: q.ctypes.data_as(_lib.f64p)        # noqa: E731
    assert lib.icelk_boxes_bin(None, f(a), f(a), f(a), f(a), 4, C.byref(st), None, cnt.ctypes.data_as(_lib.i32p), f(a), f(a), f(a),
                               None) == _lib.EARG
    assert lib.icelk_boxes_bin_windows(None, f(a), f(a), f(a), f(a), f(a), 4, None, C.byref(st), None, cnt.ctypes.data_as(_lib.i32p),
                                       f(a), f(a), f(a), None, cnt.ctypes.data_as(_lib.i32p), f(a), f(a), None) == _lib.EARG


def test_header_and_signatures_name_the_new_calls():
    text = open(os.path.join(ROOT, "include", "icelk.h")).read()
    for name in ("icelk_boxes_check", "icelk_boxes_bin", "icelk_boxes_bin_windows"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "icelk_boxes_t" in text and "icelk_day_tables_t" in text
    lib = _lib.load()
    names = [lib.icelk_prof_name(k) for k in range(lib.icelk_prof_count())]
    assert names[3] == b"lk_fb" and names[-3:] == [b"boxes_assign", b"boxes_day_assign", b"grid_day_assign"]


def test_exports():
    for name in ("azimuth_transect", "locate_points_along_transect", "create_squares_rot", "create_squares_along_transect",
                 "create_squares_around_mooring", "BoxSet", "bin_boxes", "utm_to_transect", "utm_to_transect_days"):
        assert hasattr(pkg, name), name

"""GPU: gridding (k_grid.hip through icelk_points_in_polygon / icelk_grid_bin and gridding.py) against
tests/golden/grid_golden.npz (grid from the reference's create_grid_across_fjord; per-cell means from the s3 loop body
restated with matplotlib / numpy in the generator), against the oracle on a larger seeded set, and against np.sum
itself at the cell populations where it changes strategy.  float64, bit-exact."""
import numpy as np
import pytest

import np_sums_cases as K
from test_oracle_grid import GOLD, grid_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD, allow_pickle=False)


def test_grid_equals_reference(ctx, z):
    from iceberg_tracking_code_amd import create_grid_across_fjord
    fjord = {"x": z["fjord_x"], "y": z["fjord_y"]}
    polygons, centers, indices, topleft_c, rows, cols = create_grid_across_fjord(ctx, fjord, int(z["spacing"]))
    assert rows == int(z["rows"]) and cols == int(z["cols"])
    assert np.array_equal(np.array(topleft_c, np.float64), z["topleft_center"])
    assert np.array_equal(np.array(polygons, np.float64), z["polygons"])
    assert np.array_equal(np.array(centers, np.float64), z["centers"])
    assert np.array_equal(np.array(indices, np.int64), z["indices"])


def test_binned_velocities_equal_golden(ctx, z):
    from iceberg_tracking_code_amd import bin_velocities
    fjord = {"x": z["fjord_x"], "y": z["fjord_y"]}
    r = bin_velocities(ctx, z["px"], z["py"], z["pu"], z["pv"], fjord, int(z["spacing"]),
                       int(z["observation_threshold"]))
    assert np.array_equal(r["counts_all"], z["counts_all"])
    for key in ("grid_id", "i", "j", "count"):
        assert np.array_equal(np.array(r[key], np.int64), z["res_" + key].astype(np.int64)), key
    for key in ("x", "y", "u", "v", "speed"):
        assert np.array(r[key], np.float64).tobytes() == z["res_" + key].tobytes(), key
    assert len(r["measured"]) + len(r["not_measured"]) == len(z["polygons"])


def test_large_set_equals_oracle(ctx, orc, z):
    """10^6 velocities, a quarter of them exactly on cell edges or corners, cells with up to ~10^5 observations.  The
    oracle adds a cell of more than 8192 points as np.sum does, in the chunks of numpy's buffer (oracle/grid_oracle.c)."""
    left, top, sp, cols, rows, on = grid_of(z)
    rng = np.random.default_rng(5)
    n = 1000000
    x = rng.uniform(left - 100, left + cols * sp + 100, n)
    y = rng.uniform(top - rows * sp - 100, top + 100, n)
    k = n // 8
    x[:k] = left + sp * rng.integers(0, cols + 1, k)
    y[k:2 * k] = top - sp * rng.integers(0, rows + 1, k)
    x[2 * k:3 * k] = x[3 * k:4 * k] * 0 + left + sp * 5.5 + rng.normal(0, 40, k)     # a crowded spot
    y[2 * k:3 * k] = top - sp * 7.5 + rng.normal(0, 40, k)
    u = rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 3, n)
    v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 3, n)
    from iceberg_tracking_code_amd import _lib
    import ctypes as C
    cnt = np.zeros(cols * rows, np.int32)
    mu, mv, spd = (np.zeros(cols * rows, np.float64) for _ in range(3))
    f = lambda a: a.ctypes.data_as(_lib.f64p)   # noqa: E731
    ctx._ck(ctx._lib.icelk_grid_bin(ctx._h, f(x), f(y), f(u), f(v), n, left, top, sp, cols, rows,
                                    on.ctypes.data_as(_lib.u8p), cnt.ctypes.data_as(_lib.i32p), f(mu), f(mv), f(spd)))
    want = orc.grid_bin(x, y, u, v, left, top, sp, cols, rows, on)
    assert np.array_equal(cnt, want["count"]) and cnt.max() > 50000 and (cnt[on == 1] > 0).all()
    assert mu.tobytes() == want["mean_u"].tobytes() and mv.tobytes() == want["mean_v"].tobytes()
    assert spd.tobytes() == want["speed"].tobytes()
    assert C.sizeof(C.c_double) == 8
    # the most crowded cell against numpy itself: far beyond the 8192 elements np.sum adds at a time, where the oracle
    # and the kernel once shared one pairwise run over the whole cell and so agreed with each other and not with numpy
    kmax = int(cnt.argmax())
    ox, oy = left + (kmax // rows) * sp, top - (kmax % rows) * sp
    poly = np.array([[ox, oy], [ox + sp, oy], [ox + sp, oy - sp], [ox, oy - sp]])
    sel = orc.points_in_polygon(poly, np.stack([x, y], 1)).astype(bool)
    assert sel.sum() == cnt[kmax]
    assert mu[kmax] == np.sum(u[sel]) / cnt[kmax] and mv[kmax] == np.sum(v[sel]) / cnt[kmax]


# ---- per-cell populations where np.sum changes strategy, against numpy itself --------------------------------------------

POPULATIONS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 135, 136, 137, 143, 144, 145, 255, 256, 257, 263, 264,
               265, 271, 272, 511, 512, 513, 519, 520, 1023, 1024, 1025, 1031, 1032, 2047, 2048, 2049, 2055, 2056, 4097,
               4104, 8191, 8192, 8193]
B_LEFT, B_TOP, B_SPACING, B_COLS, B_ROWS = 431000.0, 7652000.0, 200.0, 8, 8


def boundary_points(seed=0):
    """Cell k of an 8 x 8 grid (k = i * rows + j, every cell on) receives exactly POPULATIONS[k] points strictly inside
    it, the cells beyond the table small random numbers; all points shuffled into one array, u and v over seven decades."""
    rng = np.random.default_rng(seed)
    ncells = B_COLS * B_ROWS
    per_cell = np.array(POPULATIONS + list(rng.integers(0, 40, ncells - len(POPULATIONS))))
    cell = rng.permutation(np.repeat(np.arange(ncells), per_cell))
    n = len(cell)
    x = B_LEFT + B_SPACING * (cell // B_ROWS + rng.uniform(0.05, 0.95, n))
    y = B_TOP - B_SPACING * (cell % B_ROWS + rng.uniform(0.05, 0.95, n))
    u = rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 3, n)
    v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 3, n)
    # a cell's values are drawn again until their sum shows the order it was taken in (np_sums_cases.py: about one draw
    # in ten gives the same bits in numpy's order and in a wrong one)
    for k in np.flatnonzero(per_cell >= 16):
        sel = cell == k
        for a in (u, v):
            for _ in range(64):
                if K.tells_orders_apart(a[sel]):
                    break
                a[sel] = rng.normal(0, 1, per_cell[k]) * 10.0 ** rng.integers(-4, 3, per_cell[k])
    return per_cell, cell, x, y, u, v


def grid_bin(ctx, x, y, u, v, left, top, spacing, cols, rows):
    from iceberg_tracking_code_amd import _lib
    on = np.ones(cols * rows, np.uint8)
    cnt = np.full(cols * rows, -1, np.int32)
    mu, mv, spd = (np.full(cols * rows, 7.0, np.float64) for _ in range(3))
    f = lambda a: a.ctypes.data_as(_lib.f64p)   # noqa: E731
    rc = ctx._lib.icelk_grid_bin(ctx._h, f(x), f(y), f(u), f(v), len(x), left, top, spacing, cols, rows,
                                 on.ctypes.data_as(_lib.u8p), cnt.ctypes.data_as(_lib.i32p), f(mu), f(mv), f(spd))
    return rc, cnt, mu, mv, spd


def check_boundary_populations(ctx):
    from iceberg_tracking_code_amd import _lib
    per_cell, cell, x, y, u, v = boundary_points()
    rc, cnt, mu, mv, spd = grid_bin(ctx, x, y, u, v, B_LEFT, B_TOP, B_SPACING, B_COLS, B_ROWS)
    assert rc == _lib.OK
    want_u, want_v = np.zeros(len(per_cell)), np.zeros(len(per_cell))
    for k, n in enumerate(per_cell):
        sel = cell == k                                  # the cell's points in their original order
        assert sel.sum() == n
        if n > 0:
            want_u[k], want_v[k] = np.sum(u[sel]) / n, np.sum(v[sel]) / n
        if n >= 16:                                      # values whose sum shows the order it was taken in
            assert K.tells_orders_apart(u[sel]) and K.tells_orders_apart(v[sel]), (k, n)
    assert np.array_equal(cnt, per_cell)
    assert mu.tobytes() == want_u.tobytes(), np.flatnonzero(mu != want_u)
    assert mv.tobytes() == want_v.tobytes(), np.flatnonzero(mv != want_v)
    assert spd.tobytes() == np.hypot(want_u, want_v).tobytes()


def test_cell_populations_at_numpy_boundaries(ctx):
    check_boundary_populations(ctx)


def test_too_many_edge_points_is_refused_and_harmless(ctx, orc):
    """A cell's far edges are formed as (left + i * s) + s, its neighbour's near edge as left + (i + 1) * s; where the two
    round differently the cells overlap by an ulp or two, and a point in that sliver at a corner lies in all four cells
    round it.  2000 such points make 8000 keys, more than the 2 * 2000 + 1024 slots there are.  The call is refused,
    and the same handle goes on answering."""
    from iceberg_tracking_code_amd import _lib
    left, top, sp, side = 7.111428779897499, 9.320596866133782, 0.3, 40
    on = np.ones(side * side, np.uint8)
    one = np.ones(1)
    corners = []
    for i in range(side - 1):
        far_x, near_x = left + i * sp + sp, left + (i + 1) * sp
        for j in range(side - 1):
            far_y, near_y = (top - j * sp) - sp, top - (j + 1) * sp
            if near_x < far_x and near_y > far_y:
                corners += [(px, py) for px in (near_x, np.nextafter(near_x, far_x), far_x)
                            for py in (near_y, np.nextafter(near_y, far_y), far_y)]
    four = [c for c in corners if orc.grid_bin(np.array([c[0]]), np.array([c[1]]), one, one, left, top, sp, side, side,
                                               on)["count"].sum() == 4]
    assert len(four) >= 5, four
    n = 2000
    x, y = (np.ascontiguousarray(np.array(four)[np.arange(n) % len(four), k]) for k in (0, 1))
    want = orc.grid_bin(x, y, np.ones(n), np.ones(n), left, top, sp, side, side, on)
    assert want["count"].sum() == 4 * n > 2 * n + 1024
    rc, cnt, mu, mv, spd = grid_bin(ctx, x, y, np.ones(n), np.ones(n), left, top, sp, side, side)
    assert rc == _lib.ECAP
    assert b"" != ctx._lib.icelk_last_error(ctx._h)
    check_boundary_populations(ctx)
    # half as many such points fit, and land in all four cells
    h = n // 4
    rc, cnt, mu, mv, spd = grid_bin(ctx, x[:h], y[:h], np.ones(h), np.ones(h), left, top, sp, side, side)
    want = orc.grid_bin(x[:h], y[:h], np.ones(h), np.ones(h), left, top, sp, side, side, on)
    assert rc == _lib.OK and cnt.sum() == 4 * h and np.array_equal(cnt, want["count"])


def test_points_in_polygon_degenerate(ctx, orc):
    from iceberg_tracking_code_amd import points_in_polygon
    pts = np.array([[0.5, 0.5], [2.0, 2.0], [0.0, 0.0], [1.0, 0.5]])
    sq = [(0, 0), (1, 0), (1, 1), (0, 1)]
    assert np.array_equal(points_in_polygon(ctx, sq, pts), orc.points_in_polygon(sq, pts))
    assert not points_in_polygon(ctx, [(0, 0), (1, 1)], pts).any()
    assert points_in_polygon(ctx, sq, np.zeros((0, 2))).shape == (0,)

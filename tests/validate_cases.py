"""The catalogue the normalised median test is checked on (test_validate_host.py and tests/validate_main.cpp on the CPU,
test_gpu_validate.py on the device): named, seeded cases of a few hundred points at most -- but the two at the limit of the
pool kernel's LDS staging, which need POOL_LDS_TERMS points and one more.

A case is dict(name, x, y, u, v, lattice, params, groups, info): `params` the keywords threshold / eps / min_neighbours (the
defaults where absent), `groups` None or (group number per point, number of groups), `info` what the case itself knows about
its answer (checked on the numpy restatement by test_validate_host.py, never on the code under test).
"""
import functools
import struct

import numpy as np

POOL_LDS_TERMS = 2048          # csrc/k_validate.hip: kPoolLds
LAT = dict(left=1000.0, top=5000.0, side=10.0, cols=7, rows=7)


def _case(name, x, y, u, v, lattice=LAT, params=None, groups=None, **info):
    a = [np.ascontiguousarray(q, np.float64).ravel() for q in (x, y, u, v)]
    return dict(name=name, x=a[0], y=a[1], u=a[2], v=a[3], lattice=dict(lattice), params=dict(params or {}), groups=groups, info=info)


def _in_cell(rng, lattice, i, j, n):
    """n points strictly inside cell (i, j)"""
    s = lattice["side"]
    return lattice["left"] + (i + rng.uniform(0.05, 0.95, n)) * s, lattice["top"] - (j + rng.uniform(0.05, 0.95, n)) * s


def _cells(rng, lattice, spec):
    """points of [(i, j, n)] joined"""
    xs, ys = zip(*[_in_cell(rng, lattice, i, j, n) for i, j, n in spec])
    return np.concatenate(xs), np.concatenate(ys)


def small_pools():
    """pools of 1, 2 and 3 terms in cells too far apart to share a point; min_neighbours 1 judges the two larger ones"""
    rng = np.random.default_rng(1)
    x, y = _cells(rng, LAT, [(1, 1, 1), (4, 1, 2), (1, 4, 3)])
    u, v = np.array([0.3, 0.1, 0.5, -0.2, 0.0, 0.4]), np.array([0.0, 0.2, 0.2, 0.1, 0.1, 0.9])
    return _case("small_pools", x, y, u, v, params=dict(min_neighbours=1), status2=[0], pool_sizes=[1, 2, 3])


def at_min_neighbours():
    """a pool of min_neighbours terms (status 2) and one of min_neighbours + 1 (judged)"""
    rng = np.random.default_rng(2)
    x, y = _cells(rng, LAT, [(1, 1, 8), (5, 5, 9)])
    return _case("at_min_neighbours", x, y, rng.uniform(0.1, 0.2, 17), rng.uniform(-0.1, 0.1, 17), status2=list(range(8)), pool_sizes=[8, 9])


def corners_and_edges():
    """every cell of a 4 x 3 lattice filled: corner pools take 4 cells, edge pools 6, inner ones 9"""
    rng = np.random.default_rng(3)
    lat = dict(left=-35.0, top=12.5, side=2.5, cols=4, rows=3)
    x, y = _cells(rng, lat, [(i, j, 3 + (i + 2 * j) % 4) for i in range(4) for j in range(3)])
    u, v = 0.2 + 0.01 * x + rng.uniform(-0.01, 0.01, len(x)), -0.1 + rng.uniform(-0.01, 0.01, len(x))
    u[::11] += 0.7
    return _case("corners_and_edges", x, y, u, v, lattice=lat)


def one_cell_lattice():
    rng = np.random.default_rng(4)
    lat = dict(left=0.0, top=1.0, side=1.0, cols=1, rows=1)
    u, v = rng.uniform(-0.01, 0.01, 40) + 0.5, rng.uniform(-0.01, 0.01, 40)
    v[7] = 1.0
    return _case("one_cell_lattice", rng.uniform(0, 1, 40), rng.uniform(0, 1, 40), u, v, lattice=lat, rejected=[7])


def on_lines():
    """points exactly on lattice lines, on left and top (inside), on the far edges (outside), and just outside"""
    rng = np.random.default_rng(5)
    lat = dict(left=1000.0, top=5000.0, side=10.0, cols=3, rows=3)
    bx, by = _cells(rng, lat, [(i, j, 10) for i in range(3) for j in range(3)])
    lx = np.array([1000.0, 1010.0, 1020.0, 1030.0, 1005.0, 1005.0, 1005.0, 1005.0, 1000.0, 1030.0, np.nextafter(1000.0, 0), np.nextafter(1030.0, 0)])
    ly = np.array([4995.0, 4995.0, 4995.0, 4995.0, 5000.0, 4990.0, 4980.0, 4970.0, 5000.0, 4970.0, 4995.0, np.nextafter(4970.0, 9e9)])
    x, y = np.concatenate([bx, lx]), np.concatenate([by, ly])
    return _case("on_lines", x, y, rng.uniform(0.0, 0.1, len(x)), rng.uniform(0.0, 0.1, len(x)), lattice=lat,
                 status3=[90 + 3, 90 + 7, 90 + 9, 90 + 10], judged=[90, 90 + 1, 90 + 2, 90 + 4, 90 + 5, 90 + 6, 90 + 8, 90 + 11])


def outside_and_not_finite():
    """points around the lattice, and NaN, +inf, -inf in each of x, y, u, v: all status 3, none in a pool"""
    rng = np.random.default_rng(6)
    x, y = _cells(rng, LAT, [(3, 3, 30)])
    u, v = rng.uniform(0.0, 0.1, 30), rng.uniform(0.0, 0.1, 30)
    ox, oy = np.array([990.0, 1075.0, 1035.0, 1035.0, -1e300, 1e300, 1035.0]), np.array([4965.0, 4965.0, 5001.0, 4929.0, 4965.0, 4965.0, 1e300])
    bad = []
    for k in range(4):
        for s in (np.nan, np.inf, -np.inf):
            row = [1035.0, 4965.0, 0.05, 0.05]
            row[k] = s
            bad.append(row)
    bad = np.array(bad)
    x, y = np.concatenate([x, ox, bad[:, 0]]), np.concatenate([y, oy, bad[:, 1]])
    u, v = np.concatenate([u, np.full(7, 0.05), bad[:, 2]]), np.concatenate([v, np.full(7, 0.05), bad[:, 3]])
    return _case("outside_and_not_finite", x, y, u, v, status3=list(range(30, 30 + 7 + 12)), pool_sizes=[30])


def all_equal():
    """every velocity equal but two: MAD 0, eps alone decides"""
    rng = np.random.default_rng(7)
    x, y = _cells(rng, LAT, [(2, 2, 20)])
    u, v = np.full(20, 0.25), np.full(20, -0.5)
    u[3] += 0.019          # 1.9 eps: kept
    v[11] -= 0.021         # 2.1 eps: rejected
    return _case("all_equal", x, y, u, v, rejected=[11])


def at_threshold():
    """r2 exactly threshold^2 (kept) and one ulp of u above it (rejected): MAD 0, eps 0.5, |u - med| = 1.0 -> ru = 2.0"""
    rng = np.random.default_rng(8)
    x, y = _cells(rng, LAT, [(2, 2, 12)])
    u, v = np.full(12, 1.0), np.full(12, 0.0)
    u[4], u[9] = 2.0, np.nextafter(2.0, 3.0)
    return _case("at_threshold", x, y, u, v, params=dict(eps=0.5, threshold=2.0), rejected=[9], r2_exact={4: 4.0})


def overflowing_medians():
    """the middle pair's sum overflows: med inf, MAD inf, r2 NaN, kept"""
    rng = np.random.default_rng(9)
    x, y = _cells(rng, LAT, [(2, 2, 10)])
    return _case("overflowing_medians", x, y, np.full(10, 1.7e308), rng.uniform(0, 0.1, 10), nan_r2_kept=list(range(10)))


def two_groups():
    """the same coordinates in two groups: the vector at 5 m/s is an outlier among group 0's, at home in group 1's; group
    numbers outside 0 .. 2 are in no group, and group 2 has no point"""
    rng = np.random.default_rng(10)
    x0, y0 = _cells(rng, LAT, [(3, 3, 15)])
    u0, u1 = np.full(15, 1.0) + rng.uniform(-0.01, 0.01, 15), np.full(15, 5.0) + rng.uniform(-0.01, 0.01, 15)
    u0[6] = u1[6] = 5.0
    v = rng.uniform(-0.01, 0.01, 15)
    g = np.concatenate([np.zeros(15), np.ones(15), [-1, 3, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    x, y = np.concatenate([x0, x0, x0[:4]]), np.concatenate([y0, y0, y0[:4]])
    return _case("two_groups", x, y, np.concatenate([u0, u1, u0[:4]]), np.concatenate([v, v, v[:4]]), groups=(g, 3), rejected=[6],
                 status3=[30, 31, 32, 33])


def lds_limit(extra):
    """a 3 x 3 lattice whose centre cell's pool is every point: POOL_LDS_TERMS of them (the largest pool staged in LDS), or one
    more (the smallest that walks global memory); the other cells' pools are parts of it"""
    rng = np.random.default_rng(11 + extra)
    n = POOL_LDS_TERMS + extra
    lat = dict(left=0.0, top=30.0, side=10.0, cols=3, rows=3)
    x, y = rng.uniform(0.01, 29.99, n), rng.uniform(0.01, 29.99, n)
    u, v = 0.3 + rng.uniform(-0.01, 0.01, n), -0.2 + rng.uniform(-0.01, 0.01, n)
    bad = rng.choice(n, 9, replace=False)
    u[bad] += 1.0
    return _case("lds_limit_plus_%d" % extra, x, y, u, v, lattice=lat, rejected=sorted(int(b) for b in bad), largest_pool=n)


def no_points():
    z = np.zeros(0)
    return _case("no_points", z, z, z, z)


def mixed_groups():
    """three groups over a 5 x 4 lattice with empty cells, clustered points, duplicates and values of both signs"""
    rng = np.random.default_rng(13)
    lat = dict(left=-20.0, top=7.0, side=4.0, cols=5, rows=4)
    n = 400
    x, y = rng.uniform(-22, 2, n), rng.uniform(-11, 9, n)
    x[:120], y[:120] = rng.uniform(-12, -8, 120), rng.uniform(-1, 3, 120)      # one crowded cell
    u, v = rng.normal(0, 0.05, n), rng.normal(0, 0.05, n)
    u[200:230] = u[200]                                                          # ties
    u[::17] *= -30.0
    return _case("mixed_groups", x, y, u, v, lattice=lat, params=dict(threshold=3.0, eps=0.02, min_neighbours=5),
                 groups=(rng.integers(-1, 4, n).astype(np.int32), 3))


PLANTED = 12


def planted_outliers():
    """A smooth field on an 8 x 6 lattice, about 40 points per cell, a seeded noise of +-0.01 m/s, and PLANTED vectors off by
    1 m/s.  With the defaults exactly the planted set is rejected and no point has status 2; test_validate_host.py asserts
    both on the numpy restatement.  (Were it to fail, the data would be wrong -- never the rule or its defaults.)"""
    rng = np.random.default_rng(14)
    lat = dict(left=500000.0, top=6500000.0, side=100.0, cols=8, rows=6)
    n = 8 * 6 * 40
    x, y = rng.uniform(500000.0, 500800.0, n), rng.uniform(6499400.0, 6500000.0, n)
    u = 0.40 + 0.05 * (x - 500000.0) / 800.0 + rng.uniform(-0.01, 0.01, n)
    v = -0.10 + 0.04 * (6500000.0 - y) / 600.0 + rng.uniform(-0.01, 0.01, n)
    bad = np.sort(rng.choice(n, PLANTED, replace=False))
    phi = rng.uniform(0, 2 * np.pi, PLANTED)
    u[bad] += np.cos(phi)
    v[bad] += np.sin(phi)
    return _case("planted_outliers", x, y, u, v, lattice=lat, rejected=[int(b) for b in bad], exact_rejected=True, no_status2=True)


@functools.lru_cache(maxsize=None)
def catalogue():
    return (small_pools(), at_min_neighbours(), corners_and_edges(), one_cell_lattice(), on_lines(), outside_and_not_finite(), all_equal(),
            at_threshold(), overflowing_medians(), two_groups(), lds_limit(0), lds_limit(1), no_points(), mixed_groups(), planted_outliers())


def call_args(case):
    """(positional, keywords) for validate_velocities_host(*positional, **keywords) and the restatement alike"""
    return (case["x"], case["y"], case["u"], case["v"], case["lattice"]), dict(case["params"], groups=case["groups"])


# what the entry points refuse: a change to a small good call, and the kind of refusal ("arg": ICELK_EARG, "cap": ICELK_ECAP)
_NAN, _INF = float("nan"), float("inf")
REFUSALS = [(dict(threshold=0.0), "arg"), (dict(threshold=-1.0), "arg"), (dict(threshold=_NAN), "arg"), (dict(threshold=_INF), "arg"),
            (dict(eps=0.0), "arg"), (dict(eps=_NAN), "arg"), (dict(eps=_INF), "arg"), (dict(min_neighbours=0), "arg"),
            (dict(lattice=dict(side=0.0)), "arg"), (dict(lattice=dict(side=_INF)), "arg"), (dict(lattice=dict(side=_NAN)), "arg"),
            (dict(lattice=dict(cols=0)), "arg"), (dict(lattice=dict(rows=0)), "arg"), (dict(lattice=dict(cols=1 << 16, rows=1 << 15)), "cap")]
REFUSAL_IDS = ["-".join("%s=%s" % (k, v) for k, v in sorted(c.get("lattice", c).items())) for c, _ in REFUSALS]


def refused_call(call, change):
    """call(x, y, u, v, lattice, **keywords) on the at_min_neighbours case with one of REFUSALS' changes applied"""
    args, kw = call_args(catalogue()[1])
    kw = dict(kw)
    lattice = dict(args[4])
    lattice.update(change.get("lattice", {}))
    kw.update({k: v for k, v in change.items() if k != "lattice"})
    return call(*args[:4], lattice, **kw)


def dump(cases, results):
    """The catalogue and its expected results as the bytes tests/validate_main.cpp reads: int32 case count; per case int32 n,
    ngroups, has_group, cols, rows, min_neighbours; float64 left, top, side, threshold, eps; x, y, u, v (float64 n each);
    group (int32 n, if has_group); status (uint8 n), r2 (float64 n); pool_n (int32 nseg), med_u, med_v, mad_u, mad_v (float64
    nseg each)."""
    out = [struct.pack("<i", len(cases))]
    for c, r in zip(cases, results):
        p = dict(threshold=2.0, eps=0.01, min_neighbours=8)
        p.update(c["params"])
        lat, groups = c["lattice"], c["groups"]
        n = len(c["x"])
        out.append(struct.pack("<6i5d", n, groups[1] if groups else 1, 1 if groups else 0, lat["cols"], lat["rows"], p["min_neighbours"],
                               lat["left"], lat["top"], lat["side"], p["threshold"], p["eps"]))
        out += [c[k].astype("<f8").tobytes() for k in ("x", "y", "u", "v")]
        if groups:
            out.append(np.asarray(groups[0]).astype("<i4").tobytes())
        out += [r["status"].astype(np.uint8).tobytes(), r["r2"].astype("<f8").tobytes(), r["pool_n"].astype("<i4").tobytes()]
        out += [r[k].astype("<f8").tobytes() for k in ("med_u", "med_v", "mad_u", "mad_v")]
    return b"".join(out)

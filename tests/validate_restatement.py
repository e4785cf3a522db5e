"""The normalised median test restated with numpy, from the rule as DESIGN.md 7.3b states it -- np.floor, np.median and plain
float64 array arithmetic, none of the library's text.  test_validate_host.py holds `validate_velocities_host` to it bit for
bit, test_gpu_validate.py the kernels to that.

    lattice   i = floor((x - left) / side), j = floor((top - y) / side); judged: x, y, u, v finite, 0 <= i < cols,
              0 <= j < rows, 0 <= group < ngroups
    pool      of (group, i, j): the judged points of the group with |i' - i| <= 1 and |j' - j| <= 1, the point itself included
    verdict   ru = |u - med_u| / (mad_u + eps), rv likewise, r2 = ru ru + rv rv, rejected iff r2 > threshold threshold
    status    0 kept, 1 rejected, 2 pool of fewer than min_neighbours + 1 terms (r2 NaN), 3 not judged (r2 NaN)
"""
import numpy as np


def restate(x, y, u, v, lattice, threshold=2.0, eps=0.01, min_neighbours=8, groups=None):
    """The dict `validate_velocities_host` returns."""
    x, y, u, v = (np.asarray(q, np.float64).ravel() for q in (x, y, u, v))
    n = len(x)
    left, top, side = (np.float64(lattice[k]) for k in ("left", "top", "side"))
    cols, rows = int(lattice["cols"]), int(lattice["rows"])
    if groups is None:
        g, ngroups = np.zeros(n, np.int64), 1
    else:
        g, ngroups = np.asarray(groups[0], np.int64).ravel(), int(groups[1])
    with np.errstate(all="ignore"):
        fi, fj = np.floor((x - left) / side), np.floor((top - y) / side)
        judged = (np.isfinite(x) & np.isfinite(y) & np.isfinite(u) & np.isfinite(v) & (fi >= 0) & (fi < cols) & (fj >= 0) & (fj < rows)
                  & (g >= 0) & (g < ngroups))
    ci, cj = np.where(judged, fi, 0).astype(np.int64), np.where(judged, fj, 0).astype(np.int64)
    status, r2 = np.full(n, 3, np.uint8), np.full(n, np.nan)
    pool_n = np.zeros((ngroups, rows, cols), np.int32)
    med_u, med_v, mad_u, mad_v = (np.full((ngroups, rows, cols), np.nan) for _ in range(4))
    where = np.flatnonzero(judged)
    for gg, jj, ii in sorted({(int(g[p]), int(cj[p]), int(ci[p])) for p in where}):
        in_group = where[g[where] == gg]
        pool = in_group[(np.abs(ci[in_group] - ii) <= 1) & (np.abs(cj[in_group] - jj) <= 1)]
        own = pool[(ci[pool] == ii) & (cj[pool] == jj)]
        with np.errstate(all="ignore"):
            mu, mv = np.median(u[pool]), np.median(v[pool])
            du, dv = np.median(np.abs(u[pool] - mu)), np.median(np.abs(v[pool] - mv))
            pool_n[gg, jj, ii] = len(pool)
            med_u[gg, jj, ii], med_v[gg, jj, ii], mad_u[gg, jj, ii], mad_v[gg, jj, ii] = mu, mv, du, dv
            if len(pool) < min_neighbours + 1:
                status[own] = 2
                continue
            ru, rv = np.abs(u[own] - mu) / (du + np.float64(eps)), np.abs(v[own] - mv) / (dv + np.float64(eps))
            r = ru * ru + rv * rv
            r2[own] = r
            status[own] = (r > np.float64(threshold) * np.float64(threshold)).astype(np.uint8)
    return dict(status=status, keep=status != 1, r2=r2, pool_n=pool_n, med_u=med_u, med_v=med_v, mad_u=mad_u, mad_v=mad_v)


RESULT_KEYS = ("status", "keep", "r2", "pool_n", "med_u", "med_v", "mad_u", "mad_v")


def same_bits(a, b):
    """None when two result dicts agree -- shapes, dtypes and bits, a NaN matching any NaN (their signs and payloads are not
    numpy's everywhere) --, else the first key that differs"""
    for k in RESULT_KEYS:
        p, q = np.asarray(a[k]), np.asarray(b[k])
        if p.shape != q.shape or p.dtype != q.dtype:
            return k
        if p.dtype.kind == "f":
            nan = np.isnan(p)
            if not np.array_equal(nan, np.isnan(q)) or p[~nan].tobytes() != q[~nan].tobytes():
                return k
        elif p.tobytes() != q.tobytes():
            return k
    return None

"""Virtual drifters restated in numpy, written from the rule's text, not from csrc/drift.h.

The drifters of a run are carried along as the one array axis, the steps are a Python loop; each operation on the axis is a
single correctly rounded float64 operation per drifter (no dot, no sum, no fused multiply-add), and "this drifter does not
take part" is a np.where that keeps the old value.  The library's host statement must agree with this bit for bit.

The rule.  Lattice nodes x0 + i dx, y0 + j dy, cell = j cols + i.  Schedule row r is the time start + r step / 2.  Cube source:
row r has windows k0 <= k1, a weight a and a flag; a window's node is measured iff u, v are finite and count >= min_count, the
node iff both windows' are, its value (1 - a) u[k0] + a u[k1].  Tide source: the node is measured iff status == 0, its value
c[0] B[0] + c[1] B[1] + ...; the flag is always set.  Sample at (px, py): fx = (px - x0) / dx, fy alike; outside unless 0 <= fx
<= cols - 1 and 0 <= fy <= rows - 1; i = min(floor(fx), cols - 2), tx = fx - i; weights (1 - tx)(1 - ty), tx (1 - ty), (1 -
tx) ty, tx ty over (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1); all four measured: the weighted sum in that order; fewer:
the measured terms onto +0.0 in that order over the measured weights summed likewise, if at least min_nodes are measured and
the weight sum is positive.  A stage fails with 3 when the flag is 0, else 1 outside, else 2 with too few nodes.  Order 4: k1
at (p, row 2s), k2 at (p + (step / 2) k1, row 2s + 1), k3 at (p + (step / 2) k2, row 2s + 1), k4 at (p + step k3, row 2s + 2),
p' = p + (step / 6) (((k1 + 2 k2) + 2 k3) + k4); order 2: p' = p + step k2; order 1: p' = p + step k1.  The first failing stage
stops the drifter where it was (status, stop_step = s); a non-finite p' stops it with 1.  Drifter p exists from step release[p]
on iff its seed is finite and 0 <= release[p] < nsteps, else status 4, stop_step -1.  x, y are recorded at the steps 0, every,
2 every, ... while release <= s <= stop_step (nsteps if alive), NaN otherwise; length adds np.hypot of the step displacements
in step order; visits counts every finite recorded sample at the node floor(fy + 0.5), floor(fx + 0.5) if it is on the lattice."""
import numpy as np

RESULT_KEYS = ("x", "y", "last_x", "last_y", "length", "status", "stop_step", "visits")


def cube_row(c, r):
    """(flag, measured [cells], u [cells], v [cells]) of schedule row r of a cube case"""
    k0, k1, a = int(c["k0"][r]), int(c["k1"][r]), c["a"][r]
    mc = np.float64(c["min_count"])
    ok = [np.isfinite(c["u"][k]) & np.isfinite(c["v"][k]) & (c["count"][k] >= mc) for k in (k0, k1)]
    one = np.float64(1.0)
    return (bool(c["flag"][r]), ok[0] & ok[1], (one - a) * c["u"][k0] + a * c["u"][k1], (one - a) * c["v"][k0] + a * c["v"][k1])


def tide_row(c, r):
    B = c["basis"][r]
    out = []
    for coef in (c["coef_u"], c["coef_v"]):
        pred = coef[:, 0] * B[0]
        for j in range(1, len(B)):
            pred = pred + coef[:, j] * B[j]
        out.append(pred)
    return True, c["status"] == 0, out[0], out[1]


def stage(row, lattice, min_nodes, px, py):
    """(why, u, v) per drifter at the positions px, py in a schedule row"""
    x0, y0, dx, dy, rows, cols = lattice
    flag, measured, U, V = row
    fx, fy = (px - x0) / dx, (py - y0) / dy
    inside = (fx >= 0) & (fx <= cols - 1) & (fy >= 0) & (fy <= rows - 1)
    i = np.minimum(np.where(inside, np.floor(fx), 0.0).astype(np.int64), cols - 2)
    j = np.minimum(np.where(inside, np.floor(fy), 0.0).astype(np.int64), rows - 2)
    tx, ty = fx - i, fy - j
    one = np.float64(1.0)
    w = [(one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty]
    cell = [j * cols + i, j * cols + i + 1, (j + 1) * cols + i, (j + 1) * cols + i + 1]
    have = [measured[c] for c in cell]
    count = have[0].astype(int) + have[1] + have[2] + have[3]
    out = []
    for F in (U, V):
        f = [F[c] for c in cell]
        full = ((w[0] * f[0] + w[1] * f[1]) + w[2] * f[2]) + w[3] * f[3]
        acc, wsum = np.zeros(len(px)), np.zeros(len(px))
        for k in range(4):
            acc = np.where(have[k], acc + w[k] * f[k], acc)
            wsum = np.where(have[k], wsum + w[k], wsum)
        out.append(np.where(count == 4, full, acc / wsum))
    good = (count == 4) | ((count >= min_nodes) & (wsum > 0))
    why = np.where(inside, np.where(good, 0, 2), 1) if flag else np.full(len(px), 3)
    return why, out[0], out[1]


def restate(c):
    """The results of a catalogue case (tests/drift_cases.py): a dict of RESULT_KEYS"""
    lattice = c["lattice"]
    x0, y0, dx, dy, rows, cols = lattice
    h, nsteps, every, order, min_nodes = c["params"]
    h = np.float64(h)
    half, sixth, two = h / np.float64(2.0), h / np.float64(6.0), np.float64(2.0)
    sx, sy, rel = c["x"], c["y"], c["release"]
    n = len(sx)
    row_of = cube_row if c["source"] == "cube" else tide_row
    born = np.isfinite(sx) & np.isfinite(sy) & (rel >= 0) & (rel < nsteps)
    status = np.where(born, 0, 4).astype(np.int32)
    stop = np.where(born, nsteps, -1).astype(np.int32)
    x, y, length = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    live = np.zeros(n, bool)
    n_out = nsteps // every + 1
    rec_x, rec_y = np.full((n_out, n), np.nan), np.full((n_out, n), np.nan)
    with np.errstate(all="ignore"):
        for s in range(nsteps + 1):
            new = born & (rel == s)
            x, y, live = np.where(new, sx, x), np.where(new, sy, y), live | new
            if s % every == 0:
                rec_x[s // every], rec_y[s // every] = np.where(live, x, np.nan), np.where(live, y, np.nan)
            if s == nsteps:
                break
            why, k1u, k1v = stage(row_of(c, 2 * s), lattice, min_nodes, x, y)
            if order == 1:
                nx, ny = x + h * k1u, y + h * k1v
            else:
                mid = row_of(c, 2 * s + 1)
                w2, k2u, k2v = stage(mid, lattice, min_nodes, x + half * k1u, y + half * k1v)
                why = np.where(why == 0, w2, why)
                if order == 2:
                    nx, ny = x + h * k2u, y + h * k2v
                else:
                    w3, k3u, k3v = stage(mid, lattice, min_nodes, x + half * k2u, y + half * k2v)
                    why = np.where(why == 0, w3, why)
                    w4, k4u, k4v = stage(row_of(c, 2 * s + 2), lattice, min_nodes, x + h * k3u, y + h * k3v)
                    why = np.where(why == 0, w4, why)
                    nx = x + sixth * (((k1u + two * k2u) + two * k3u) + k4u)
                    ny = y + sixth * (((k1v + two * k2v) + two * k3v) + k4v)
            why = np.where((why == 0) & ~(np.isfinite(nx) & np.isfinite(ny)), 1, why)
            stopped, moved = live & (why != 0), live & (why == 0)
            status = np.where(stopped, why, status).astype(np.int32)
            stop = np.where(stopped, s, stop).astype(np.int32)
            length = np.where(moved, length + np.hypot(nx - x, ny - y), length)
            x, y = np.where(moved, nx, x), np.where(moved, ny, y)
            live = moved
        visits = np.zeros((rows, cols), np.int32)
        fin = np.isfinite(rec_x) & np.isfinite(rec_y)
        gx, gy = np.floor((rec_x - x0) / dx + 0.5), np.floor((rec_y - y0) / dy + 0.5)
        on = fin & (gx >= 0) & (gx <= cols - 1) & (gy >= 0) & (gy <= rows - 1)
        np.add.at(visits, (gy[on].astype(np.int64), gx[on].astype(np.int64)), 1)
    return dict(x=rec_x, y=rec_y, last_x=x, last_y=y, length=length, status=status, stop_step=stop, visits=visits)


def same_bits(a, b, keys=RESULT_KEYS):
    """None when two result dicts agree -- shapes, dtypes and bits, a NaN matching any NaN --, else the first key that differs"""
    for k in keys:
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

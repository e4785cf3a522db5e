"""Validation of projected velocities between projection and gridding: the normalised median test.

s2's per-track rules (speed bounds, speed ratio, turning angle) pass a track that is smooth and wrong -- a wave crest, a bird,
a reflection, a feature that slid along an edge -- and s3's cell mean swallows it.  The check here is spatial: a vector is
compared with the vectors around it (Westerweel & Scarano 2005, "Universal outlier detection for PIV data").

The rule (csrc/validate.h; `validate_velocities_host` is that text on the CPU, csrc/k_validate.hip the kernels, and
tests/validate_restatement.py restates it in numpy; the three agree bit for bit):
- a lattice of squares (`validation_lattice`), independent of the gridder's cells: i = floor((x - left) / side),
  j = floor((top - y) / side); a point is judged if x, y, u, v are finite, its cell lies in the lattice and it has a group
  (a time window of the day form);
- its pool is every judged point of its group in the 3 x 3 cells around its own, clipped at the lattice edge -- the point
  itself included, where the paper leaves it out (a median per cell instead of one per point; with the pool sizes met here
  the difference is small);
- with med and mad np.median's bits of the pool's u and of |u - med| (v likewise): ru = |u - med_u| / (mad_u + eps),
  r2 = ru * ru + rv * rv, rejected iff r2 > threshold * threshold.
`status`: 0 judged and kept, 1 rejected, 2 a pool of fewer than min_neighbours + 1 points (kept), 3 not judged.

The defaults -- threshold 2.0, eps 0.01 m/s, min_neighbours 8, a lattice side of twice the gridder's cell -- are policy, not
measurements.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import VALIDATE_FEW_NEIGHBOURS, VALIDATE_KEPT, VALIDATE_NOT_JUDGED, VALIDATE_REJECTED  # noqa: F401

DEFAULTS = dict(threshold=2.0, eps=0.01, min_neighbours=8)
CELL_KEYS = ("pool_n", "med_u", "med_v", "mad_u", "mad_v")


def validation_lattice(fjord, side):
    """The lattice over a fjord outline's bounding box: dict(left, top, side, cols, rows) with left = min x, top = max y and as
    many columns and rows of `side` as cover the box (one at least)."""
    fx, fy = np.asarray(fjord["x"], np.float64), np.asarray(fjord["y"], np.float64)
    left, right, bottom, top = float(fx.min()), float(fx.max()), float(fy.min()), float(fy.max())
    side = float(side)
    if not (side > 0 and math.isfinite(side)):
        raise ValueError("side must be positive and finite")
    return dict(left=left, top=top, side=side, cols=max(int(math.ceil((right - left) / side)), 1),
                rows=max(int(math.ceil((top - bottom) / side)), 1))


def lattice_struct(lattice):
    return _lib.ValidateLattice(left=float(lattice["left"]), top=float(lattice["top"]), side=float(lattice["side"]),
                                cols=int(lattice["cols"]), rows=int(lattice["rows"]))


def params_struct(threshold=2.0, eps=0.01, min_neighbours=8):
    """icelk_validate_params_t of the keywords; the ranges are the library's to check"""
    return _lib.ValidateParams(threshold=float(threshold), eps=float(eps), min_neighbours=int(min_neighbours), reserved=0)


def validate_options(validate, grid_size):
    """What the drivers' `validate=` means: None -> None; True -> the defaults on a lattice side of 2 * grid_size; a dict ->
    its threshold / eps / min_neighbours / side over those.  Returns dict(threshold, eps, min_neighbours, side)."""
    if validate is None or validate is False:
        return None
    out = dict(DEFAULTS, side=2.0 * float(grid_size))
    if validate is not True:
        unknown = set(validate) - set(out)
        if unknown:
            raise ValueError("validate: unknown keys %s" % sorted(unknown))
        out.update(validate)
    return out


def validation_array(options):
    """the `validation` entry of a window file: threshold, eps, min_neighbours, side as float64"""
    return np.array([options["threshold"], options["eps"], options["min_neighbours"], options["side"]], np.float64)


def _validate(call, handle, x, y, u, v, lattice, threshold, eps, min_neighbours, groups):
    a = [np.ascontiguousarray(q, dtype=np.float64).ravel() for q in (x, y, u, v)]
    n = len(a[0])
    if any(len(q) != n for q in a):
        raise ValueError("x, y, u, v must have one length")
    g, ngroups = None, 1
    if groups is not None:
        g, ngroups = groups
        g, ngroups = np.ascontiguousarray(g, dtype=np.int32).ravel(), int(ngroups)
        if len(g) != n:
            raise ValueError("one group number per point")
    L, P = lattice_struct(lattice), params_struct(threshold, eps, min_neighbours)
    nseg = max(ngroups, 0) * max(L.cols, 0) * max(L.rows, 0)
    if nseg >= 1 << 31:
        nseg = 0                                  # refused below; nothing this large is allocated for the refusal
    status, r2 = np.zeros(n, np.uint8), np.zeros(n, np.float64)
    cells = {k: np.zeros(nseg, np.int32 if k == "pool_n" else np.float64) for k in CELL_KEYS}
    cs = _lib.ValidateCells(cells["pool_n"].ctypes.data_as(_lib.i32p), *[cells[k].ctypes.data_as(_lib.f64p) for k in CELL_KEYS[1:]])
    f64 = lambda q: q.ctypes.data_as(_lib.f64p)                       # noqa: E731
    rc = call(f64(a[0]), f64(a[1]), f64(a[2]), f64(a[3]), n, None if g is None else g.ctypes.data_as(_lib.i32p), ngroups,
              C.byref(L), C.byref(P), status.ctypes.data_as(_lib.u8p), f64(r2), C.byref(cs))
    _lib.check(rc, handle)
    shape = (ngroups, L.rows, L.cols)
    out = dict(status=status, keep=status != VALIDATE_REJECTED, r2=r2)
    out.update({k: c.reshape(shape) for k, c in cells.items()})
    return out


def validate_velocities(ctx, x, y, u, v, lattice, threshold=2.0, eps=0.01, min_neighbours=8, groups=None):
    """The normalised median test on the device (`icelk_validate`).  x, y, u, v: the projected velocities; lattice: what
    `validation_lattice` returns; groups: None (one pool set), or (group number per point, number of groups) -- points of
    different groups never share a pool, a number outside 0 .. ngroups - 1 is in no group.  Returns dict(status (uint8), keep
    (bool: everything but the rejected), r2 (float64, NaN where not judged), pool_n, med_u, med_v, mad_u, mad_v (each
    (ngroups, rows, cols); 0 and NaN for a cell without a point of its own))."""
    def call(*args):
        return ctx._lib.icelk_validate(ctx._h, *args)
    return _validate(call, ctx._h, x, y, u, v, lattice, threshold, eps, min_neighbours, groups)


def validate_velocities_host(x, y, u, v, lattice, threshold=2.0, eps=0.01, min_neighbours=8, groups=None):
    """`validate_velocities` by the library's host statement of the rule (`icelk_validate_host`): no GPU, the same dict."""
    return _validate(_lib.load().icelk_validate_host, None, x, y, u, v, lattice, threshold, eps, min_neighbours, groups)

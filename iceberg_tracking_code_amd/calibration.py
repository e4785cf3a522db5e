"""Step s0_2: s0_2_camera_calibration.py -- the camera angles theta, phi, psi and the scale sigma fitted so that the
shoreline digitised on a photo, projected to the map, falls on the waterline digitised from a satellite image.

The misfit (`optimizefun_calibration`, s0_2:240-275: project every shoreline point, s0_2:117-152, and take its distance
to the nearest waterline vertex, s0_2:231-238) runs on the device for any number of candidates at once
(`icelk_calib_residuals` / `icelk_calib_cost`, csrc/k_calib.hip), bit for bit the reference's numbers.  What stays
here is the preparation of the candidates (eleven doubles each, vectorised numpy with the products in the order of
s0_2:124-136), the Levenberg-Marquardt loop that polishes all seeds together, and the table bookkeeping of
`run_calibration` (s0_2:279-450).  There is no CPU fallback for the misfit.

Deliberate differences from the reference: the fit is this module's own Levenberg-Marquardt loop with
clipping at the bounds, not lmfit's MINPACK call with its sine transform of bounded parameters, so the fitted numbers
are not pinned against lmfit -- only the misfit is; and the best nodes of a dense lattice over the parameter box can
be added as seeds.  Reference quirk kept: without a tide series H is the elevation column as it stands (s0_2:330-342
subtracts the antenna height only together with the tide).
Not built: shapefile and workbook readers and writers, `create_shapefile`, the .prj download.
"""
import ctypes as C
import datetime as dt

import numpy as np

from . import _lib
from .context import Context
from .utm import CameraModel

TOL = 1.5e-8                       # ftol = xtol of the fit: what lmfit hands MINPACK (1.5e-8)
_PARAMS = ("theta", "phi", "psi", "sigma")
_CHUNK = 1 << 18                   # candidates per launch of the lattice
DEL_FIELDS = ("image", "imagefolder", "sigma_min", "sigma_max", "theta_min", "theta_max", "phi_min", "phi_max",
              "psi_min", "psi_max")                                                  # s0_2:442-443


def prepare_candidates(theta, phi, psi, sigma, H, image_width, sensor_width):
    """(P, 11) float64: X[3], U[3], V[3], sigma in pixels, H per candidate -- the expressions of s0_2:254-257 and
    124-136 (the same as CameraModel.direction_vectors) on arrays.  Angles in degrees, sigma unscaled."""
    theta, phi, psi, sigma, H = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, np.float64))
                                                      for a in (theta, phi, psi, sigma, H)))
    th, ph, ps = np.radians(theta), np.radians(phi), np.radians(psi)
    sth, cth, sph, cph, sps, cps = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph), np.sin(ps), np.cos(ps)
    c = np.empty((th.shape[0], 11), np.float64)
    c[:, 0], c[:, 1], c[:, 2] = cth * cph, sth * cph, sph
    c[:, 3], c[:, 4], c[:, 5] = sth * cps - cth * sph * sps, -cth * cps - sth * sph * sps, cph * sps
    c[:, 6], c[:, 7], c[:, 8] = -sth * sps - cth * sph * cps, cth * sps - sth * sph * cps, cph * cps
    c[:, 9] = (np.float64(image_width) / np.float64(sensor_width)) * sigma
    c[:, 10] = H
    return c


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def _root(meansq):
    """meansq ** 0.5 as the reference takes it (s0_2:393): the power of a numpy SCALAR, which is libm's pow.  On an
    array `** 0.5` turns into sqrt and np.power into a vectorised pow, and both differ from it in the last bit now
    and then; np.float_power runs the scalar's pow over the array."""
    return np.float_power(meansq, 0.5)


class ShorelineScene:
    """The data of one calibration on the device: the shoreline points of the photo (`x`, `y` as
    `x_y_from_shapefile` returns them, y already negated) and the waterline vertices (W, 2) on the map, with the
    image size, sensor width and camera position they are evaluated with.  A context holds one scene at a time;
    without `ctx` the scene makes and owns a context.  All methods take the workbook's units (degrees, sigma
    unscaled), broadcast their arguments to P candidates and return exactly the reference's float64 numbers."""

    def __init__(self, ctx, x, y, waterline_xy, image_width, image_height, sensor_width, easting, northing):
        x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
        water = np.ascontiguousarray(waterline_xy, dtype=np.float64)
        if x.shape != y.shape or x.size < 1:
            raise ValueError("x and y must be two arrays of one length, at least one point")
        if water.ndim != 2 or water.shape[1] != 2 or water.shape[0] < 1:
            raise ValueError("waterline_xy must be (W, 2) with W >= 1")
        if not np.isfinite(water).all():
            raise ValueError("the waterline holds a non-finite vertex")
        self.x, self.y, self.waterline = x, y, water
        self.image_width, self.image_height, self.sensor_width = image_width, image_height, sensor_width
        self.easting, self.northing = np.float64(easting), np.float64(northing)
        self.M, self.W = x.size, water.shape[0]
        shore = np.ascontiguousarray(np.stack([x - image_width / 2.0, y - image_height / 2.0], 1))    # s0_2:260-261
        if ctx is not None and getattr(ctx, "_calib_scene", None) is not None:
            raise _lib.IcelkError("this context already holds a calibration scene: close that one first")
        self._own = ctx is None
        self.ctx = Context(64, 64, n_slots=1, max_pts=1024) if self._own else ctx
        self._set = False
        try:
            self.ctx._ck(self.ctx._lib.icelk_calib_set(self.ctx._h, _f64(shore), self.M, _f64(water), self.W,
                                                       float(self.easting), float(self.northing)))
            self._set = True
            self.ctx._calib_scene = self
        except Exception:
            self.close()
            raise

    def close(self):
        if self._set:
            if self.ctx._h.value:
                self.ctx._lib.icelk_calib_release(self.ctx._h)
            self.ctx._calib_scene = None
        self._set = False
        if self._own:
            self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- device calls, chunked over P so that P * M fits 31 bits -------------------------------------------------
    def _chunk(self, chunk):
        return max(1, min(int(chunk) if chunk else _CHUNK, 0x7fffffff // self.M))

    def _candidates(self, theta, phi, psi, sigma, H):
        return prepare_candidates(theta, phi, psi, sigma, H, self.image_width, self.sensor_width)

    def _residuals(self, cand, want_xy, chunk, timing):
        P = cand.shape[0]
        dist = np.empty((P, self.M), np.float64)
        tx, ty = (np.empty((P, self.M), np.float64) for _ in range(2)) if want_xy else (None, None)
        step, ms, total = self._chunk(chunk), C.c_double(0.0), 0.0
        for a in range(0, P, step):
            b = min(P, a + step)
            part = np.ascontiguousarray(cand[a:b])
            self.ctx._ck(self.ctx._lib.icelk_calib_residuals(
                self.ctx._h, _f64(part), b - a, _f64(dist[a:b]), _f64(tx[a:b]) if want_xy else None,
                _f64(ty[a:b]) if want_xy else None, C.byref(ms) if timing is not None else None))
            total += ms.value
        if timing is not None:
            timing.update(kernels_ms=total, pairs=P * self.M * self.W)
        return dist, tx, ty

    def _meansq(self, cand, chunk, timing):
        P = cand.shape[0]
        out = np.empty(P, np.float64)
        step, ms, total = self._chunk(chunk), C.c_double(0.0), 0.0
        for a in range(0, P, step):
            b = min(P, a + step)
            part = np.ascontiguousarray(cand[a:b])
            self.ctx._ck(self.ctx._lib.icelk_calib_cost(self.ctx._h, _f64(part), b - a, _f64(out[a:b]),
                                                        C.byref(ms) if timing is not None else None))
            total += ms.value
        if timing is not None:
            timing["kernels_ms"] = timing.get("kernels_ms", 0.0) + total
            timing["pairs"] = timing.get("pairs", 0) + P * self.M * self.W
        return out

    # ---- the public forms --------------------------------------------------------------------------------------
    def residuals(self, theta, phi, psi, sigma, H, chunk=None, timing=None):
        """(P, M): what optimizefun_calibration returns for each candidate."""
        return self._residuals(self._candidates(theta, phi, psi, sigma, H), False, chunk, timing)[0]

    def project(self, theta, phi, psi, sigma, H, chunk=None):
        """tx, ty (P, M) each: the shoreline points on the map (photo_to_utm, s0_2:117-152)."""
        return self._residuals(self._candidates(theta, phi, psi, sigma, H), True, chunk, None)[1:]

    def rmse(self, theta, phi, psi, sigma, H, chunk=None, timing=None):
        """(P,): np.mean(residuals ** 2) ** 0.5 (s0_2:393 before rounding), without the (P, M) array."""
        return _root(self._meansq(self._candidates(theta, phi, psi, sigma, H), chunk, timing))

    def lattice(self, bounds, n, H, chunk=None, timing=None):
        """The rmse on a regular lattice over the box `bounds` = ((theta_min, theta_max), (phi_min, phi_max),
        (psi_min, psi_max), (sigma_min, sigma_max)): `n` nodes per axis (one number or four), axes from np.linspace.
        Returns (axes, rmse) with rmse of shape (n_theta, n_phi, n_psi, n_sigma): flattened, it is in
        itertools.product(*axes) order."""
        n = (int(n),) * 4 if np.ndim(n) == 0 else tuple(int(k) for k in n)
        if len(n) != 4 or min(n) < 1:
            raise ValueError("n: one positive count, or one per parameter")
        axes = [np.linspace(float(lo), float(hi), k) for (lo, hi), k in zip(bounds, n)]
        total = int(np.prod(n))
        out = np.empty(total, np.float64)
        step = self._chunk(chunk)
        for a in range(0, total, step):
            b = min(total, a + step)
            idx = np.unravel_index(np.arange(a, b), n)
            cand = self._candidates(axes[0][idx[0]], axes[1][idx[1]], axes[2][idx[2]], axes[3][idx[3]], H)
            out[a:b] = self._meansq(cand, step, timing)
        return axes, _root(out).reshape(n)


class CalibrationResult:
    """What `calibrate` returns.  Per seed s: params[s] = (theta, phi, psi, sigma) fitted, rmse[s], seeds[s] (where
    it started), seed_rmse[s], iterations[s]; `row_seeds` = how many leading seeds are row midpoints (the rest
    come from the lattice); `best` = the index of the smallest rmse (the first of equals; NaN never wins)."""

    def __init__(self, scene, H, params, rmse, seeds, seed_rmse, iterations, row_seeds):
        self.scene, self.H = scene, H
        self.params, self.rmse, self.seeds, self.seed_rmse = params, rmse, seeds, seed_rmse
        self.iterations, self.row_seeds = iterations, row_seeds
        finite = np.where(np.isnan(rmse), np.inf, rmse)
        self.best = int(np.argmin(finite))

    def camera_model(self, seed=None, **crop):
        """The CameraModel of seed `seed` (default: the best) for the projection step; `crop`: crop_left, crop_right,
        crop_top, crop_bottom of the tracked images."""
        theta, phi, psi, sigma = (float(v) for v in self.params[self.best if seed is None else seed])
        s = self.scene
        return CameraModel(s.image_width, s.image_height, s.sensor_width, s.easting, s.northing, self.H, 0.0, theta,
                           phi, psi, sigma, **crop)


def _sumsq(r):
    return np.sum(r * r, axis=1)


def levenberg_marquardt(evaluate, H, seeds, lower, upper, max_iter=200, tol=TOL):
    """All seeds (S, 4) polished together inside their boxes lower, upper (S, 4 each).  `evaluate(theta, phi, psi,
    sigma, H)` -> (P, M) residuals.  Per iteration one call for every seed that moved -- its point and the four
    forward-difference neighbours (step sqrt(eps) |x|, backwards where the upper bound is in the way) -- and one
    call for the trial points x + d of all live seeds, (J'J + lambda diag(J'J)) d = -J'r, clipped to the box.  A trial
    is accepted only when the sum of squares decreases (lambda / 3), else lambda * 4.  A seed stops when an accepted
    step gains no more than tol of the sum of squares, when a step is shorter than tol (|x| + tol), when lambda
    passes 1e12, or at max_iter.  Returns x (S, 4), residuals (S, M), iterations (S,), first residuals (S, M)."""
    x = np.clip(np.array(seeds, np.float64, ndmin=2), lower, upper)
    S = x.shape[0]
    lam = np.full(S, 1e-3)
    live = np.ones(S, bool)
    moved = np.ones(S, bool)
    iters = np.zeros(S, np.int64)
    r = J = first = None
    eps = np.sqrt(np.finfo(np.float64).eps)
    for _ in range(max_iter):
        need = np.flatnonzero(live & moved)
        if need.size:
            h = eps * np.abs(x[need])
            h[h == 0.0] = eps
            h = np.where(x[need] + h > upper[need], -h, h)
            pts = np.repeat(x[need], 5, axis=0)
            for j in range(4):
                pts[j + 1::5, j] += h[:, j]
                h[:, j] = pts[j + 1::5, j] - x[need, j]        # the difference actually taken
            res = np.asarray(evaluate(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], H))
            if r is None:
                r = np.empty((S, res.shape[1]))
                J = np.empty((S, res.shape[1], 4))
            r[need] = res[0::5]
            for j in range(4):
                J[need, :, j] = (res[j + 1::5] - res[0::5]) / h[:, j][:, None]
            if first is None:
                first = r.copy()
            bad = ~np.isfinite(_sumsq(r[need])) | ~np.isfinite(J[need]).all(axis=(1, 2))
            live[need[bad]] = False          # a seed whose misfit or slope is not finite stays where it is
            moved[need] = False
        idx = np.flatnonzero(live)
        if not idx.size:
            break
        A = np.einsum("smi,smj->sij", J[idx], J[idx])
        g = np.einsum("smi,sm->si", J[idx], r[idx])
        diag = np.einsum("sii->si", A)
        damp = lam[idx, None] * np.where(diag > 0.0, diag, 1.0)
        A = A + damp[:, :, None] * np.eye(4)
        try:
            d = np.linalg.solve(A, -g[:, :, None])[:, :, 0]
        except np.linalg.LinAlgError:
            d = np.stack([np.linalg.lstsq(a, -b, rcond=None)[0] for a, b in zip(A, g)])
        trial = np.clip(x[idx] + d, lower[idx], upper[idx])
        rt = np.asarray(evaluate(trial[:, 0], trial[:, 1], trial[:, 2], trial[:, 3], H))
        iters[idx] += 1
        ss0, ss1 = _sumsq(r[idx]), _sumsq(rt)
        ok = ss1 < ss0                                   # NaN never passes
        step = np.sqrt(np.sum((trial - x[idx]) ** 2, axis=1))
        small_step = step <= tol * (np.sqrt(np.sum(x[idx] ** 2, axis=1)) + tol)
        small_gain = ok & (ss0 - ss1 <= tol * ss0)
        acc = idx[ok]
        x[acc] = trial[ok]
        r[acc] = rt[ok]
        moved[acc] = True
        lam[acc] = np.maximum(lam[acc] / 3.0, 1e-15)
        lam[idx[~ok]] *= 4.0
        live[idx[small_gain | small_step | (lam[idx] > 1e12)]] = False
    return x, r, iters, first


def _lattice_nodes(scene, evaluate, lo, hi, n, H, top_k):
    """The `top_k` nodes of smallest rmse of the n-per-axis lattice over the box lo, hi (ties by lattice index; NaN
    last), as (k, 4)."""
    bounds = list(zip(lo, hi))
    if evaluate is None:
        axes, cost = scene.lattice(bounds, n, H)
    else:
        n = (int(n),) * 4 if np.ndim(n) == 0 else tuple(int(k) for k in n)
        axes = [np.linspace(float(a), float(b), k) for (a, b), k in zip(bounds, n)]
        grid = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], 1)
        res = np.asarray(evaluate(grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3], H))
        cost = _root(np.array([np.mean(row ** 2) for row in res])).reshape(n)
    flat = np.where(np.isnan(cost.ravel()), np.inf, cost.ravel())
    pick = np.argsort(flat, kind="stable")[:int(top_k)]
    return np.stack([ax[i] for ax, i in zip(axes, np.unravel_index(pick, cost.shape))], 1)


def _rmse_rows(r):
    return np.array([np.mean(row ** 2) ** 0.5 for row in r])          # s0_2:393, row by row


def calibrate(scene, H, rows, lattice_n=None, top_k=8, refine=0, evaluate=None, max_iter=200):
    """The fit of s0_2:364-393 for every row of the workbook that shares a scene, all at once.  `rows`: one
    (theta_min, theta_max, phi_min, phi_max, psi_min, psi_max, sigma_min, sigma_max) box each; a row starts at the
    midpoint of its box (s0_2:367-374) and stays inside it.  With `lattice_n` the `top_k` best nodes of the lattice
    over the union of the boxes (ties by lattice index) are added as seeds, bounded by the union box; and each of
    `refine` further rounds lays the same lattice over a box around the best result so far -- one cell of the
    previous lattice to either side -- and polishes its `top_k` best nodes as well.  H is fixed (s0_2:375).
    `evaluate`, a callable (theta, phi, psi, sigma, H) -> (P, M), replaces the device calls (the lattices then go
    through it too); the CPU tests hand in the numpy restatement, which is its only purpose.  Returns a
    CalibrationResult; its seeds come in the order rows, lattice, refinement rounds."""
    rows = np.array(rows, np.float64, ndmin=2)
    if rows.shape[1] != 8:
        raise ValueError("a row is (theta_min, theta_max, phi_min, phi_max, psi_min, psi_max, sigma_min, sigma_max)")
    lower, upper = rows[:, 0::2], rows[:, 1::2]
    if (lower > upper).any():
        raise ValueError("a box has min > max")
    seeds = np.stack([np.mean(rows[:, 2 * j:2 * j + 2], axis=1) for j in range(4)], 1)
    ev = evaluate if evaluate is not None else scene.residuals
    lo, hi = lower.min(axis=0), upper.max(axis=0)
    use_lattice = lattice_n is not None and top_k > 0
    if use_lattice:
        nodes = _lattice_nodes(scene, evaluate, lo, hi, lattice_n, H, top_k)
        seeds = np.concatenate([seeds, nodes])
        lower = np.concatenate([lower, np.tile(lo, (len(nodes), 1))])
        upper = np.concatenate([upper, np.tile(hi, (len(nodes), 1))])
    x, r, iters, first = levenberg_marquardt(ev, H, seeds, lower, upper, max_iter=max_iter)
    rmse, seed_rmse = _rmse_rows(r), _rmse_rows(first)
    cell = (hi - lo) / np.maximum(np.broadcast_to(np.asarray(lattice_n if use_lattice else 2), (4,)) - 1, 1)
    for _ in range(int(refine) if use_lattice else 0):
        finite = np.where(np.isnan(rmse), np.inf, rmse)
        centre = x[int(np.argmin(finite))]
        blo, bhi = np.clip(centre - cell, lo, hi), np.clip(centre + cell, lo, hi)
        nodes = _lattice_nodes(scene, evaluate, blo, bhi, lattice_n, H, top_k)
        k = len(nodes)
        x2, r2, it2, first2 = levenberg_marquardt(ev, H, nodes, np.tile(lo, (k, 1)), np.tile(hi, (k, 1)),
                                                  max_iter=max_iter)
        x, iters, seeds = np.concatenate([x, x2]), np.concatenate([iters, it2]), np.concatenate([seeds, nodes])
        rmse, seed_rmse = np.concatenate([rmse, _rmse_rows(r2)]), np.concatenate([seed_rmse, _rmse_rows(first2)])
        cell = (bhi - blo) / np.maximum(np.broadcast_to(np.asarray(lattice_n), (4,)) - 1, 1)
    return CalibrationResult(scene, H, x, rmse, seeds, seed_rmse, iters, rows.shape[0])


def calibration_groups(table, tides=None):
    """The bookkeeping of s0_2:286-343: the table with the result columns added, and the rows grouped by what makes
    a scene -- {(camera, time_string, sensor_width, easting, northing, image_width, image_height, H): [(index,
    tide or None)]}.  time_string: the image name up to its first dot.  With `tides` (a DataFrame with `date` and
    `depth_tide_ellipsoid`) the tide is looked up at the image time with the seconds zeroed and H = elevation -
    antenna_height - tide; without, H = elevation."""
    df = table.reindex(columns=table.columns.tolist() + ["H", "theta", "phi", "psi", "sigma", "rmse", "tide"])
    groups = {}
    for index, row in df.iterrows():
        time_string = str(row["image"]).split(".")[0]
        H, tide = row["elevation"], None
        if tides is not None:
            when = dt.datetime.strptime(time_string, "%Y%m%d-%H%M%S").replace(second=0)
            tide = float(tides.loc[tides["date"] == when]["depth_tide_ellipsoid"].iloc[0])
            H = H - row["antenna_height"] - tide
        key = (row["camera"], time_string, row["sensor_width"], row["easting"], row["northing"], row["image_width"],
               row["image_height"], H)
        groups.setdefault(key, []).append((index, tide))
    return df, groups


def group_boxes(df, members):
    """The rows' boxes in the layout `calibrate` takes."""
    return [[df.at[i, p + s] for p in _PARAMS for s in ("_min", "_max")] for i, _ in members]


def store_results(df, members, H, result):
    """s0_2:388-427: a row gets the result of its own midpoint seed, rounded to 5 decimals (H, rmse, tide: 2)."""
    for k, (index, tide) in enumerate(members):
        for j, p in enumerate(_PARAMS):
            df.at[index, p] = round(result.params[k, j], 5)
        df.at[index, "H"] = round(H, 2)
        df.at[index, "rmse"] = round(result.rmse[k], 2)
        df.at[index, "output_step"] = index + 1
        if tide is not None:
            df.at[index, "tide"] = round(tide, 2)


def drop_input_fields(df):
    for field in DEL_FIELDS:                          # s0_2:442-446
        if field in df.columns:
            del df[field]
    return df


def run_calibration(table, shorelines, waterline_xy, tides=None, ctx=None, **fit):
    """The body of the reference's run_calibration (s0_2:279-450) on a pandas DataFrame with the workbook's columns
    (camera, image, sensor_width, easting, northing, elevation, antenna_height, image_width, image_height and the
    eight *_min / *_max columns).  `shorelines[(camera, time_string)]` = (x, y) of that photo's digitised shoreline;
    `waterline_xy` (W, 2); `tides` as in calibration_groups.  Rows of one group are fitted by one `calibrate` call
    (`fit`: its keywords).  Adds the columns H, theta, phi, psi, sigma, rmse, tide, output_step, drops DEL_FIELDS,
    returns the table."""
    df, groups = calibration_groups(table, tides)
    own = ctx is None
    if own:
        ctx = Context(64, 64, n_slots=1, max_pts=1024)
    try:
        for (cam, time_string, sensor_width, E, N, imwidth, imheight, H), members in groups.items():
            x, y = shorelines[(cam, time_string)]
            with ShorelineScene(ctx, x, y, waterline_xy, imwidth, imheight, sensor_width, E, N) as scene:
                store_results(df, members, H, calibrate(scene, H, group_boxes(df, members), **fit))
    finally:
        if own:
            ctx.close()
    return drop_input_fields(df)

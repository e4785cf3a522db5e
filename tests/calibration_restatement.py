"""The calibration misfit of the reference (s0_2_camera_calibration.py: photo_to_utm 117-152, closest_node 231-238,
optimizefun_calibration 240-275) restated in plain numpy, one candidate at a time, independent of the package: the
yardstick of the CPU tests (pinned to the reference's own functions by tests/golden/calibration_golden.npz) and of the
GPU tests beyond the golden cases.

Per candidate: radians of the three angles, sigma scaled by imwidth / sensor_width, the direction vectors, the
projection with `den` formed once, then for every projected point dx * dx + dy * dy over all vertices (unfused), the
minimum, the square root.  np.min propagates NaN as the reference's np.min(dist_2 ** 0.5) does.
"""
import numpy as np


def project(theta, phi, psi, sigma, H, x, y, imwidth, imheight, sensor_width, E, N):
    """tx, ty (M,) of one candidate (degrees, sigma unscaled)."""
    theta, phi, psi = np.radians(theta), np.radians(phi), np.radians(psi)
    sigma = (imwidth / sensor_width) * sigma
    xi = x - imwidth / 2.0
    yi = y - imheight / 2.0
    st, ct, sp, cp, ss, cs = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi), np.sin(psi), np.cos(psi)
    X = (ct * cp, st * cp, sp)
    U = (st * cs - ct * sp * ss, -ct * cs - st * sp * ss, cp * ss)
    V = (-st * ss - ct * sp * cs, ct * ss - st * sp * cs, cp * cs)
    with np.errstate(all="ignore"):
        den = sigma * X[2] + xi * U[2] + yi * V[2]
        tx = H * (sigma * X[0] + xi * U[0] + yi * V[0]) / den
        ty = H * (sigma * X[1] + xi * U[1] + yi * V[1]) / den
        return tx + E, ty + N


def nearest(tx, ty, water, block=64):
    """(M,) distance of every (tx, ty) to the nearest vertex of water (W, 2)."""
    out = np.empty(tx.shape[0], np.float64)
    wx, wy = water[:, 0], water[:, 1]
    with np.errstate(all="ignore"):
        for a in range(0, tx.shape[0], block):
            dx = wx[None, :] - tx[a:a + block, None]
            dy = wy[None, :] - ty[a:a + block, None]
            out[a:a + block] = np.sqrt(np.min(dx * dx + dy * dy, axis=1))
    return out


def residuals_one(theta, phi, psi, sigma, H, x, y, imwidth, imheight, sensor_width, E, N, water):
    tx, ty = project(theta, phi, psi, sigma, H, x, y, imwidth, imheight, sensor_width, E, N)
    return nearest(tx, ty, water), tx, ty


class Scene:
    """The arguments of optimizefun_calibration that do not change during a fit; `evaluate` has the signature of
    ShorelineScene.residuals (arrays of P candidates -> (P, M))."""

    def __init__(self, x, y, water, imwidth, imheight, sensor_width, E, N):
        self.x, self.y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        self.water = np.asarray(water, np.float64)
        self.args = (imwidth, imheight, sensor_width, E, N)

    def _each(self, theta, phi, psi, sigma, H):
        cols = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, np.float64)) for a in (theta, phi, psi, sigma, H)))
        for t, p, s, g, h in zip(*cols):
            yield residuals_one(t, p, s, g, h, self.x, self.y, *self.args, self.water)

    def evaluate(self, theta, phi, psi, sigma, H):
        return np.array([r[0] for r in self._each(theta, phi, psi, sigma, H)])

    def project(self, theta, phi, psi, sigma, H):
        rows = list(self._each(theta, phi, psi, sigma, H))
        return np.array([r[1] for r in rows]), np.array([r[2] for r in rows])

    def meansq(self, theta, phi, psi, sigma, H):
        return np.array([np.mean(r[0] ** 2) for r in self._each(theta, phi, psi, sigma, H)])

    def rmse(self, theta, phi, psi, sigma, H):
        # the power of a numpy scalar, as s0_2:393 takes it (an array's ** 0.5 is sqrt and may differ in the last bit)
        with np.errstate(all="ignore"):
            return np.array([np.mean(r[0] ** 2) ** 0.5 for r in self._each(theta, phi, psi, sigma, H)])

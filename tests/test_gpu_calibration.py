"""Camera calibration on the device: the misfit kernels against the reference's own numbers (golden) and the numpy
restatement, bit for bit; the fit on the device against the same driver run on the restatement; the C ABI's checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

import calibration_restatement as R
import calibration_scenes as S
from iceberg_tracking_code_amd import Context, IcelkError, ShorelineScene, _lib, calibrate, run_calibration
from calibration_scenes import FIT, GOLDEN, fit_conditions, golden_scene, same_bits

pytestmark = pytest.mark.gpu


def device_scene(ctx, scene):
    return ShorelineScene(ctx, scene.x, scene.y, scene.water, *scene.args)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_residuals_and_projection_are_the_reference_bit_for_bit(ctx, name):
    g = np.load(GOLDEN)
    _, scene = golden_scene(g, name)
    cand = g[name + "_cand"].T
    with device_scene(ctx, scene) as dev:
        res = dev.residuals(*cand)
        tx, ty = dev.project(*cand)
        rmse = dev.rmse(*cand)
        chunked = dev.residuals(*cand, chunk=7)
    assert same_bits(res, g[name + "_res"]) and same_bits(res, scene.evaluate(*cand))
    assert same_bits(tx, g[name + "_tx"]) and same_bits(ty, g[name + "_ty"])
    assert same_bits(rmse, g[name + "_rmse"])
    assert same_bits(chunked, res)
    assert np.isnan(res).any() or name == "a"


# (M, W): every edge of numpy's pairwise sum (sequential below 8 terms, blocks of 128), W up to 2 * 10^4; the products
# are kept near 10^9 point pairs so that the restatement on the host stays within a minute
SHAPES = [(1, 20000), (7, 129), (8, 5000), (9, 20000), (127, 999), (128, 1000), (129, 1000), (180, 2000), (1000, 200)]


@pytest.mark.parametrize("M,W", SHAPES)
def test_rmse_matches_the_restatement_on_4096_candidates(ctx, M, W):
    rng = np.random.default_rng(1000 * M + W)
    cam = S.CAM
    x, y = rng.uniform(0, cam["imwidth"], M), rng.uniform(1300, cam["imheight"], M)
    true = np.array([201.4, 11.85, 1.27, 24.6])
    wx, wy = R.project(*true, S.H, rng.uniform(0, cam["imwidth"], W), rng.uniform(1300, cam["imheight"], W),
                       cam["imwidth"], cam["imheight"], cam["sensor_width"], cam["E"], cam["N"])
    scene = R.Scene(x, y, np.stack([wx, wy], 1), cam["imwidth"], cam["imheight"], cam["sensor_width"], cam["E"],
                    cam["N"])
    P = 4096
    cand = true + rng.normal(0, 1, (P, 4)) * np.array([4.0, 6.0, 1.5, 1.2])      # phi across 0: den changes sign
    cand[5, 0] = np.nan
    H = S.H + rng.normal(0, 0.5, P)
    with device_scene(ctx, scene) as dev:
        rmse = dev.rmse(*cand.T, H)
        chunked = dev.rmse(*cand.T, H, chunk=1000)
    assert same_bits(rmse, scene.rmse(*cand.T, H))
    assert same_bits(chunked, rmse) and np.isnan(rmse[5])


def test_lattice_is_the_rmse_in_product_order(ctx):
    sc = S.make(5, noise_px=1.0)
    lo, hi = S.union_box(sc["rows"])
    n = (4, 3, 3, 2)
    with device_scene(ctx, sc["scene"]) as dev:
        axes, cost = dev.lattice(list(zip(lo, hi)), n, S.H)
        axes2, cost2 = dev.lattice(list(zip(lo, hi)), n, S.H, chunk=5)
    assert cost.shape == n and all(same_bits(a, np.linspace(l, h, k)) for a, l, h, k in zip(axes, lo, hi, n))
    grid = np.array(list(itertools.product(*axes)))
    assert same_bits(cost.ravel(), sc["scene"].rmse(*grid.T, S.H)) and same_bits(cost2, cost)


@pytest.mark.parametrize("seed,noise", [(1, 0.0), (2, 0.0), (3, 0.0), (1, 1.0), (2, 1.0), (3, 1.0)])
def test_fit_on_the_device(ctx, seed, noise):
    """The same iterates, the same bits as the driver run on the restatement, and the conditions of the fit."""
    sc = S.make(seed, noise_px=noise)
    with device_scene(ctx, sc["scene"]) as dev:
        result = calibrate(dev, S.H, sc["rows"], **FIT)
        best = fit_conditions(result, dev, sc["true"], noise=bool(noise))
    host = calibrate(None, S.H, sc["rows"], evaluate=sc["scene"].evaluate, **FIT)
    assert same_bits(result.params, host.params) and same_bits(result.rmse, host.rmse)
    assert same_bits(result.seeds, host.seeds) and np.array_equal(result.iterations, host.iterations)
    assert result.best == host.best
    if noise:
        lo, hi = S.union_box(sc["rows"])
        scipy_best = S.scipy_best_rmse(sc["scene"], list(result.seeds) + [(lo + hi) / 2], lo, hi)
        print("best rmse", best, "scipy's best", scipy_best, "difference", best - scipy_best)
        assert best <= scipy_best + 0.01


def test_run_calibration_on_the_device(ctx):
    import pandas as pd
    sc = S.make(6)
    box = dict(zip([p + s for p in ("theta", "phi", "psi", "sigma") for s in ("_min", "_max")], sc["rows"].T))
    table = pd.DataFrame(dict(
        camera=["camA"] * 3, image=["20190724-101537.JPG"] * 3, imagefolder=["f"] * 3,
        sensor_width=S.CAM["sensor_width"], easting=S.CAM["E"], northing=S.CAM["N"], elevation=S.H,
        antenna_height=1.35, image_width=S.CAM["imwidth"], image_height=S.CAM["imheight"], **box))
    out = run_calibration(table, {("camA", "20190724-101537"): (sc["x"], sc["y"])}, sc["water"], ctx=ctx, **FIT)
    host = calibrate(None, S.H, sc["rows"], evaluate=sc["scene"].evaluate, **FIT)
    for k in range(3):
        assert [out.at[k, p] for p in ("theta", "phi", "psi", "sigma")] == [round(v, 5) for v in host.params[k]]
        assert out.at[k, "rmse"] == round(host.rmse[k], 2) and out.at[k, "H"] == round(S.H, 2)
    assert "theta_min" not in out.columns and list(out["output_step"]) == [1, 2, 3]
    assert getattr(ctx, "_calib_scene", None) is None


def test_scene_checks_and_abi_error_codes(ctx):
    lib = _lib.load()
    f64 = lambda a: a.ctypes.data_as(_lib.f64p)               # noqa: E731
    shore, water = np.zeros((3, 2)), np.ones((5, 2))
    cand, out = np.ones((2, 11)), np.zeros((2, 3))
    h = C.c_void_p()
    assert lib.icelk_create(0, 64, 64, 1, 1024, C.byref(h)) == _lib.OK
    try:
        # no scene yet
        assert lib.icelk_calib_residuals(h, f64(cand), 2, f64(out), None, None, None) == _lib.ESTATE
        assert lib.icelk_calib_cost(h, f64(cand), 2, f64(out), None) == _lib.ESTATE
        assert lib.icelk_calib_release(h) == _lib.OK
        for args in ((None, 3, f64(water), 5), (f64(shore), 3, None, 5), (f64(shore), 0, f64(water), 5),
                     (f64(shore), 3, f64(water), 0)):
            assert lib.icelk_calib_set(h, *args, 1.0, 2.0) == _lib.EARG
        bad = water.copy()
        bad[4, 1] = np.inf
        assert lib.icelk_calib_set(h, f64(shore), 3, f64(bad), 5, 1.0, 2.0) == _lib.EARG
        assert lib.icelk_calib_set(h, f64(shore), 3, f64(water), 5, 1.0, 2.0) == _lib.OK
        assert lib.icelk_calib_residuals(h, None, 2, f64(out), None, None, None) == _lib.EARG
        assert lib.icelk_calib_residuals(h, f64(cand), 2, None, None, None, None) == _lib.EARG
        assert lib.icelk_calib_residuals(h, f64(cand), 0, f64(out), None, None, None) == _lib.EARG
        assert lib.icelk_calib_cost(h, f64(cand), 2, None, None) == _lib.EARG
        # P * M must fit 31 bits: checked before anything is read or issued
        assert lib.icelk_calib_residuals(h, f64(cand), 0x7fffffff // 3 + 1, f64(out), None, None, None) == _lib.ECAP
        assert lib.icelk_calib_cost(h, f64(cand), 0x7fffffff // 3 + 1, f64(out), None) == _lib.ECAP
        ms = C.c_double(-1.0)
        assert lib.icelk_calib_residuals(h, f64(cand), 2, f64(out), None, None, C.byref(ms)) == _lib.OK
        assert ms.value >= 0.0
        # released: the state is gone; a second scene replaces the first
        assert lib.icelk_calib_release(h) == _lib.OK
        assert lib.icelk_calib_cost(h, f64(cand), 2, f64(out), None) == _lib.ESTATE
        assert lib.icelk_calib_set(h, f64(shore), 3, f64(water), 5, 1.0, 2.0) == _lib.OK
        assert lib.icelk_calib_set(h, f64(shore), 2, f64(water), 4, 1.0, 2.0) == _lib.OK
        # the cost kernel holds 4096 points
        big = np.zeros((4097, 2))
        assert lib.icelk_calib_set(h, f64(big), 4097, f64(water), 5, 1.0, 2.0) == _lib.OK
        assert lib.icelk_calib_cost(h, f64(cand), 2, f64(out), None) == _lib.ECAP
    finally:
        assert lib.icelk_destroy(h) == _lib.OK                 # frees the scene still set
    assert lib.icelk_calib_set(None, f64(shore), 3, f64(water), 5, 1.0, 2.0) == _lib.EARG
    # the Python side
    with pytest.raises(ValueError):
        ShorelineScene(ctx, [1.0, 2.0], [1.0, 2.0], [[0.0, np.nan]], 100, 100, 10.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        ShorelineScene(ctx, [1.0, 2.0], [1.0], [[0.0, 1.0]], 100, 100, 10.0, 0.0, 0.0)
    with ShorelineScene(ctx, [1.0, 2.0], [1.0, 2.0], [[0.0, 1.0]], 100, 100, 10.0, 0.0, 0.0):
        with pytest.raises(IcelkError):
            ShorelineScene(ctx, [1.0], [1.0], [[0.0, 1.0]], 100, 100, 10.0, 0.0, 0.0)
    own = ShorelineScene(None, [1.0, 2.0], [1.0, 2.0], [[0.0, 1.0]], 100, 100, 10.0, 0.0, 0.0)
    assert own.residuals(10.0, 5.0, 1.0, 20.0, 100.0).shape == (1, 2)
    own.close()
    assert isinstance(own.ctx, Context) and not own.ctx._h.value

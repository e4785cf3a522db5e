"""Per-cell standard deviation, median and MAD on the host: csrc/grid_stats.h through `icelk_grid_cell_stats_host` (the
library's host statement) and through tests/grid_stats_main.cpp (a program of its own), against numpy itself --
np.std(ddof=1), np.median, np.median(np.abs(a - np.median(a))) -- and against tests/grid_stats_restatement.py, bit for
bit; a NaN equals a NaN of any sign.  Then what carries the statistics to the files: `pack_cells` and
`combine_npzs(extra=...)`.  No GPU, no tolerance."""
import os

import numpy as np
import pytest

import day_grid_golden as G
import grid_stats_cases as K
import grid_stats_restatement as R
from iceberg_tracking_code_amd import grid_cell_stats_host, gridding, postprocess

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def segments():
    out = [("%s %d" % (K.family_of(n), n), K.values(K.family_of(n), n)) for n in K.LENGTHS]
    for family in sorted(K.FAMILIES):                       # every family at every strategy change of the sums and selects
        out += [("%s %d" % (family, n), K.values(family, n, seed=9)) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 128, 129,
                                                                              255, 256, 257, 1000, 8192, 8193)]
    out += [("special %d" % k, a) for k, a in enumerate(K.special_cases())]
    out.append(("empty", np.zeros(0)))
    return out


@pytest.fixture(scope="module")
def cases():
    segs = segments()
    return segs, [R.numpy_stats(a) for _, a in segs]


def test_host_statement_equals_numpy_and_restatement(cases):
    segs, want = cases
    wrong = []
    for (name, a), w in zip(segs, want):
        got = grid_cell_stats_host(a)
        if not K.same(got, w) or not K.same(R.cell_stats(a), w):
            wrong.append((name, got, R.cell_stats(a), w))
    assert not wrong, wrong[:5]


def test_the_rules_named_in_the_header():
    b = lambda x: np.float64(x).view(np.uint64)             # noqa: E731
    assert b(grid_cell_stats_host([-0.0])[1]) == b(0.0) == b(np.median(np.array([-0.0])))
    assert grid_cell_stats_host([1e308, 1e308])[1] == np.inf
    assert np.isnan(grid_cell_stats_host([-np.inf, np.inf])[1])
    assert np.isnan(grid_cell_stats_host([3.0])[0]) and grid_cell_stats_host([3.0])[1:] == (3.0, 0.0)
    assert all(np.isnan(x) for x in grid_cell_stats_host([]))
    for a in ([np.nan, 1.0, 2.0], [1.0, np.nan, 2.0], [1.0, 2.0, np.nan]):
        assert all(np.isnan(x) for x in grid_cell_stats_host(a))
    # two equal middle terms between unequal neighbours; and the upper middle one step above the lower
    assert grid_cell_stats_host([1.0, 5.0, 5.0, 9.0])[1] == 5.0 and grid_cell_stats_host([9.0, 1.0, 5.0, 7.0])[1] == 6.0


def test_cases_can_tell_a_wrong_rule():
    """The inputs decide: the standard deviation around a plainly summed mean, the median as a single middle term and the
    MAD around the mean each differ from numpy somewhere in the sweep."""
    segs = [a for _, a in segments() if len(a) >= 2 and np.isfinite(a).all()]
    with np.errstate(all="ignore"):
        assert any(np.sqrt(np.add.accumulate((a - np.add.accumulate(a)[-1] / len(a)) ** 2)[-1] / (len(a) - 1)) != np.std(a, ddof=1) for a in segs)
        assert any(np.sort(a)[len(a) // 2] != np.median(a) for a in segs)
        assert any(np.median(np.abs(a - np.mean(a))) != R.numpy_stats(a)[2] for a in segs)


def test_program_equals_numpy_and_its_select_equals_a_sort(cases, tmp_path):
    segs, want = cases
    exe = K.build(tmp_path)
    got, _ = K.run(exe, tmp_path, [a for _, a in segs])
    wrong = [name for (name, a), g, w in zip(segs, got, want) if not K.same(g[:3], w)]
    assert not wrong, wrong[:10]
    for (name, a), g in zip(segs, got):
        if len(a) and not np.isnan(a).any():
            # the select's total order: the sign bit first, so -0.0 lies below +0.0 (np.median cannot tell)
            bits = a.view(np.uint64)
            keys = np.sort(np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63)))
            lower = keys[len(a) // 2] if len(a) % 2 else keys[len(a) // 2 - 1]
            back = ~lower if lower >> np.uint64(63) == 0 else lower & np.uint64((1 << 63) - 1)
            assert g[3:4].view(np.uint64)[0] == back and g[4] == np.count_nonzero(keys <= lower), name


def test_program_under_sanitizers(tmp_path):
    """select_rank's histogram, the frame stack of the sums and every functor's index on buffers of exactly the segment's
    size: the program must exit clean."""
    exe = K.build(tmp_path, ["-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE)
    segs = [K.values(K.family_of(n), n) for n in K.LENGTHS] + K.special_cases() + [np.zeros(0)]
    _, stdout = K.run(exe, tmp_path, segs)
    assert stdout.splitlines()[-2] == "%d segments, %d terms" % (len(segs), sum(len(a) for a in segs)), stdout


# ---- pack_cells and combine_npzs -----------------------------------------------------------------------------------------

def hand_grid():
    """2 columns x 3 rows, five kept cells, as create_grid_across_fjord lists them"""
    rows, cols, sp = 3, 2, 100.0
    indices = [[0, 0], [0, 1], [0, 2], [1, 0], [1, 2]]
    polys = [[(i * sp, -j * sp), (i * sp + sp, -j * sp), (i * sp + sp, -j * sp - sp), (i * sp, -j * sp - sp)] for i, j in indices]
    centers = [[i * sp + 50.0, -j * sp - 50.0] for i, j in indices]
    grid = [polys, centers, indices, [50.0, -50.0], rows, cols]
    idx = np.array([i * rows + j for i, j in indices], np.int64)
    return grid, idx


def hand_results(seed):
    rng = np.random.default_rng(seed)
    cnt = np.array([9, 0, 6, 7, 3, 12], np.int32)
    mu, mv = rng.normal(size=6), rng.normal(size=6)
    stats = {k: rng.normal(size=6) for k in ("std_u", "std_v", "median_u", "median_v", "mad_u", "mad_v")}
    return cnt, mu, mv, np.hypot(mu, mv), stats


def test_pack_cells_with_and_without_statistics():
    grid, idx = hand_grid()
    cnt, mu, mv, sp, stats = hand_results(1)
    plain = gridding.pack_cells(grid, idx, cnt, mu, mv, sp, 5)
    assert sorted(plain) == sorted(["grid_id", "i", "j", "x", "y", "u", "v", "speed", "count", "measured", "not_measured", "counts_all"])
    full = gridding.pack_cells(grid, idx, cnt, mu, mv, sp, 5, stats=stats)
    assert sorted(full) == sorted(list(plain) + list(gridding.STATS_KEYS))
    for k in plain:                                          # today's keys: same values, dtypes and bytes
        a, b = np.asanyarray(plain[k]), np.asanyarray(full[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    kept = [c for c in idx if cnt[c] > 5]
    assert full["grid_id"] == [0, 2, 3, 4] and kept == [0, 2, 3, 5]
    for key, field in (("u_std", "std_u"), ("v_std", "std_v"), ("u_median", "median_u"), ("v_median", "median_v"),
                       ("u_mad", "mad_u"), ("v_mad", "mad_v")):
        assert np.asarray(full[key]).tobytes() == stats[field][kept].tobytes(), key
    assert np.asarray(full["speed_median"]).tobytes() == np.hypot(stats["median_u"], stats["median_v"])[kept].tobytes()


def window_file(folder, name, seed, with_stats):
    grid, idx = hand_grid()
    cnt, mu, mv, sp, stats = hand_results(seed)
    r = gridding.pack_cells(grid, idx, cnt, mu, mv, sp, 5, stats=stats if with_stats else None)
    r.update(grid_size=100, topleft=grid[3], rows=grid[4], cols=grid[5])
    keys = G.OUT_KEYS + (gridding.STATS_KEYS if with_stats else ())
    np.savez(os.path.join(folder, name), **{k: np.asanyarray(r[k]) for k in keys})
    return r


def test_combine_npzs_extra_fields(tmp_path):
    names = ["20220712_0600-0630_30min_100m.npz", "20220712_0630-0700_30min_100m.npz"]
    packed = [window_file(str(tmp_path), name, seed, True) for seed, name in enumerate(names)]
    plain = postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False)
    extra = ("u_median", "v_mad", "speed_median")
    cube = postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False, extra=extra)
    assert sorted(cube) == sorted(list(plain) + list(extra))
    assert sorted(plain) == sorted(["x", "y", "i", "j", "u", "v", "speed", "count", "time", "time_matlab"])
    for k in plain:
        assert plain[k].dtype == cube[k].dtype and plain[k].shape == cube[k].shape and plain[k].tobytes() == cube[k].tobytes(), k
    for name in extra:
        assert cube[name].shape == (3, 2, 2) and cube[name].dtype == np.float64
        for k, r in enumerate(packed):
            want = np.full((3, 2), np.nan)
            for i, j, val in zip(r["i"], r["j"], r[name]):
                want[j, i] = val
            assert K.same(cube[name][:, :, k], want) and np.isnan(want).sum() == 2, (name, k)
    # one raster, the default list unchanged, the extra rasters a dict behind it
    path = os.path.join(str(tmp_path), names[0])
    base = postprocess.velocities_to_regular_grid(path)
    more = postprocess.velocities_to_regular_grid(path, extra=("u_std",))
    assert len(base) == 12 and len(more) == 13 and list(more[12]) == ["u_std"]
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(base, more[:12]))
    assert more[12]["u_std"][0, 0] == packed[0]["u_std"][0]
    # saved beside the cube's own fields
    postprocess.combine_npzs(str(tmp_path), str(tmp_path), "cube_with_stats.npz", extra=("u_mad",))
    with np.load(os.path.join(str(tmp_path), "cube_with_stats.npz")) as z:
        assert sorted(z.files) == sorted(list(plain) + ["u_mad"])


def test_combine_npzs_missing_extra_field_raises(tmp_path):
    window_file(str(tmp_path), "20220712_0600-0630_30min_100m.npz", 0, True)
    window_file(str(tmp_path), "20220712_0630-0700_30min_100m.npz", 1, False)
    with pytest.raises(ValueError):
        postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False, extra=("u_median",))
    with pytest.raises(ValueError):
        postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False, extra=("no_such_field",))
    assert postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False)["u"].shape == (3, 2, 2)


def test_combine_npzs_default_on_the_golden_folder(tmp_path):
    """the s3 outputs of the golden day, rebuilt on disk: extra=() is the call without the keyword, array for array"""
    z = G.load()
    for name, arrays in G.outputs(z, 0):
        np.savez(os.path.join(str(tmp_path), name), **arrays)
    a = postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False)
    b = postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False, extra=())
    assert sorted(a) == sorted(b) == sorted(["x", "y", "i", "j", "u", "v", "speed", "count", "time", "time_matlab"])
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(ValueError):
        postprocess.combine_npzs(str(tmp_path), str(tmp_path), "unused", save=False, extra=("u_std",))

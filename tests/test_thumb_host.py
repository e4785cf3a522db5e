"""CPU: the inset photographs' host side (csrc/thumb_raster.h) -- icelk_thumb_size and icelk_thumb_host
against tests/thumb_restatement.py and against Pillow's Image.reduce, the choice of photo and its time against the
reference's expressions, the placement of the boxes, and icelk_map_overlay_insets_host against the map's restatement with a
numpy paste of thumbnail and label.  No GPU."""
import ctypes as C
import datetime as dt
import importlib.util
import os
import sys

import numpy as np
import pytest
from PIL import Image

import map_cases as mc
import thumb_cases as tc
import thumb_restatement as T

REFERENCE = "/root/reference"      # the project this one was modelled on, where a development container has it

# (W, H) -> (tw, th): the identity, every weight spanning two pixels, one pixel, a ratio that is no whole number, a whole
# one, and a row and a column that cross eight of the kernel's 256-column passes
SHAPES = [((67, 45), (67, 45)), ((67, 45), (66, 44)), ((67, 45), (1, 1)), ((67, 45), (9, 7)), ((64, 48), (8, 6)), ((2100, 9), (260, 1)),
          ((9, 2100), (1, 260))]


def _image(w, h, channels, seed):
    shape = (h, w) if channels == 1 else (h, w, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("src,size", SHAPES)
def test_thumb_host_equals_restatement(src, size, channels):
    from iceberg_tracking_code_amd import thumbnail_host
    a = _image(src[0], src[1], channels, 7 * src[0] + channels)
    want = T.reduce(a, size)
    got = thumbnail_host(a, size)
    assert got.shape == (size[1], size[0], 3) and np.array_equal(got, want)
    if size == src:
        assert np.array_equal(got, a if channels == 3 else np.repeat(a[..., None], 3, axis=2))
    # a stride larger than the row, on both sides
    wide = np.zeros((src[1], src[0] * channels + 13), np.uint8)
    wide[:, :src[0] * channels] = a.reshape(src[1], -1)
    view = wide[:, :src[0] * channels].reshape(a.shape)
    assert not view.flags.c_contiguous or src[1] == 1
    assert np.array_equal(thumbnail_host(view, size), want)
    from iceberg_tracking_code_amd import _lib
    out = np.full((size[1], 3 * size[0] + 5), 0xAA, np.uint8)
    rc = _lib.load().icelk_thumb_host(wide.ctypes.data_as(_lib.u8p), src[0], src[1], channels, wide.strides[0], size[0], size[1],
                                      out.ctypes.data_as(_lib.u8p), out.strides[0])
    assert rc == _lib.OK and np.array_equal(out[:, :3 * size[0]].reshape(size[1], size[0], 3), want) and (out[:, 3 * size[0]:] == 0xAA).all()


def test_thumb_host_refusals():
    from iceberg_tracking_code_amd import _lib, thumbnail_host
    lib = _lib.load()
    a = _image(16, 12, 3, 1)
    out = np.zeros((12, 16, 3), np.uint8)
    p, q = a.ctypes.data_as(_lib.u8p), out.ctypes.data_as(_lib.u8p)
    assert lib.icelk_thumb_host(p, 16, 12, 3, 48, 16, 12, q, 48) == _lib.OK
    for args in ((None, 16, 12, 3, 48, 8, 6, q, 48), (p, 16, 12, 3, 48, 8, 6, None, 48), (p, 16, 12, 2, 48, 8, 6, q, 48), (p, 16, 12, 3, 47, 8, 6, q, 48),
                 (p, 16, 12, 3, 48, 17, 6, q, 64), (p, 16, 12, 3, 48, 8, 13, q, 48), (p, 16, 12, 3, 48, 0, 6, q, 48), (p, 16, 12, 3, 48, 8, 0, q, 48),
                 (p, 16, 12, 3, 48, 8, 6, q, 23), (p, 0, 12, 3, 48, 8, 6, q, 48), (p, 65536, 12, 3, 1 << 20, 8, 6, q, 48)):
        assert lib.icelk_thumb_host(*args) == _lib.EARG, args
    with pytest.raises(ValueError):
        thumbnail_host(a, (17, 12))
    with pytest.raises(ValueError):
        thumbnail_host(a.astype(np.float32), (8, 6))


def test_thumb_size_both_branches_and_refusals():
    from iceberg_tracking_code_amd import _lib, thumbnail_size
    rng = np.random.default_rng(3)
    cases = [(4000, 3000, 280, 200), (4000, 3000, 280, 300), (3000, 4000, 280, 200), (10, 10, 50, 50), (67, 45, 67, 45), (100, 3, 1, 1),
             (3, 100, 1, 1), (65535, 1, 16384, 16384), (1, 65535, 16384, 16384), (65535, 65535, 16384, 1), (5184, 3456, 252, 168), (2, 65535, 16384, 16384)]
    cases += [tuple(int(v) for v in rng.integers(1, 6000, 4)) for _ in range(300)]
    first = second = 0
    for W, H, bw, bh in cases:
        tw, th = thumbnail_size(W, H, (bw, bh))
        assert (tw, th) == T.size(W, H, (bw, bh)), (W, H, bw, bh)
        assert 1 <= tw <= min(W, bw) and 1 <= th <= min(H, bh)
        if max(1, (2 * min(bw, W) * H + W) // (2 * W)) > bh:
            second += 1
        else:
            first += 1
    assert first > 50 and second > 50
    assert thumbnail_size(10, 10, (50, 50)) == (10, 10)                     # fits unreduced: never enlarged
    assert thumbnail_size(4000, 3000, (1, 1)) == (1, 1)
    tw, th = C.c_int(7), C.c_int(7)
    lib = _lib.load()
    for args in ((0, 10, 5, 5), (10, 0, 5, 5), (65536, 10, 5, 5), (10, 65536, 5, 5), (10, 10, 0, 5), (10, 10, 5, 0), (10, 10, 16385, 5),
                 (10, 10, 5, 16385), (10, 10, -1, 5)):
        assert lib.icelk_thumb_size(*args, C.byref(tw), C.byref(th)) == _lib.EARG and (tw.value, th.value) == (7, 7)
        with pytest.raises(ValueError):
            thumbnail_size(args[0], args[1], args[2:])
    assert lib.icelk_thumb_size(10, 10, 5, 5, None, C.byref(th)) == _lib.EARG


@pytest.mark.parametrize("f", (2, 3, 4, 5, 6, 7, 8, 16))
def test_whole_number_factors_against_pillow_reduce(f):
    """An outside pin: for the factors 2, 4, 8 and 16 Image.reduce rounds the exact mean as the rule does; for 3, 5, 6 and 7
    it multiplies by a rounded reciprocal and may differ by one."""
    from iceberg_tracking_code_amd import thumbnail_host
    w, h = 11 * f, 7 * f
    for channels in (1, 3):
        a = _image(w, h, channels, 100 + f)
        ours = thumbnail_host(a, (11, 7))
        pil = np.asarray(Image.fromarray(a).reduce(f))
        if channels == 1:
            pil = np.repeat(pil[..., None], 3, axis=2)
        d = np.abs(ours.astype(int) - pil.astype(int)).max()
        print("factor", f, "channels", channels, "largest difference", d)
        assert d == 0 if f in (2, 4, 8, 16) else d <= 1


# ---- the choice of photo, its time, the boxes ----------------------------------------------------------------------------------
def _photo_tree(root, photos):
    for day, stamp in photos:
        folder = os.path.join(str(root), day)
        os.makedirs(folder, exist_ok=True)
        open(os.path.join(folder, stamp + ".jpg"), "wb").close()


def _reference_closest():
    path = os.path.join(REFERENCE, "imports", "tracking_misc.py")
    if not os.path.exists(path):
        return None
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location("reference_tracking_misc", path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module.return_closest_image
    except Exception:                                                        # a library the reference imports is missing
        return None
    finally:
        sys.path.remove(os.path.dirname(path))


# (folder, name): the folders are days in Alaska, eight hours behind the names' clock, which is the target's
PHOTOS = [("20190724", "20190724-091000"), ("20190724", "20190724-092000"), ("20190724", "20190724-093000"), ("20190724", "20190724-094000"),
          ("20190723", "20190724-075500"), ("20190724", "20190724-080459"), ("20190724", "20190724-092400")]
TARGETS = [dt.datetime(2019, 7, 24, 9, 14, 59), dt.datetime(2019, 7, 24, 9, 22, 0), dt.datetime(2019, 7, 24, 9, 15, 1), dt.datetime(2019, 7, 24, 9, 45, 0),
           dt.datetime(2019, 7, 24, 9, 44, 59, 999999), dt.datetime(2019, 7, 24, 9, 35, 1), dt.datetime(2019, 7, 24, 8, 0, 0), dt.datetime(2019, 7, 24, 8, 0, 1),
           dt.datetime(2019, 7, 24, 7, 59, 0), dt.datetime(2019, 7, 24, 9, 5, 0, 500000)]


def _expected(root, target):
    """the rule written out: the folder of Alaska's day, the nearest stamp, strictly less than 300 s, a tie to the earlier"""
    folder = (target - dt.timedelta(hours=8)).strftime("%Y%m%d")
    times = sorted(dt.datetime.strptime(s, "%Y%m%d-%H%M%S") for day, s in PHOTOS if day == folder)
    if not times:
        return None
    best = min(times, key=lambda t: (abs(t - target), t))
    return os.path.join(str(root), folder, best.strftime("%Y%m%d-%H%M%S.jpg")) if abs((target - best).total_seconds()) < 300 else None


def test_closest_image(tmp_path):
    from iceberg_tracking_code_amd import closest_image
    _photo_tree(tmp_path, PHOTOS)
    open(os.path.join(str(tmp_path), "20190724", "notes.jpg"), "wb").close()           # a name that does not parse is skipped
    open(os.path.join(str(tmp_path), "20190724", "20190724-09150x.jpg"), "wb").close()
    got = [closest_image(str(tmp_path), t) for t in TARGETS]
    assert got == [_expected(tmp_path, t) for t in TARGETS]
    assert got[0].endswith("091000.jpg") and got[1].endswith("092000.jpg") and got[2].endswith("092000.jpg")   # 09:22:00: a tie, the earlier
    assert got[3] is None and got[4].endswith("094000.jpg")                              # exactly 300 s away is not used; a microsecond less is
    assert got[6].endswith("080459.jpg") and got[8].endswith(os.path.join("20190723", "20190724-075500.jpg"))   # the folder is the local day
    assert closest_image(str(tmp_path), TARGETS[0], max_timediff=1) is None
    assert closest_image(str(tmp_path / "nowhere"), TARGETS[0]) is None                  # the reference raises
    os.makedirs(str(tmp_path / "empty" / "20190724"))
    assert closest_image(str(tmp_path / "empty"), TARGETS[0]) is None


def test_closest_image_against_the_reference(tmp_path):
    ref = _reference_closest()
    if ref is None:
        pytest.skip("the reference's imports/tracking_misc.py is not on this machine, or does not import here")
    from iceberg_tracking_code_amd import closest_image
    _photo_tree(tmp_path, PHOTOS)
    for t in TARGETS:
        if t == TARGETS[1]:
            continue                                                                     # the tie: the reference takes glob's order
        want = ref(str(tmp_path), t, 300)
        assert closest_image(str(tmp_path), t) == (None if want == -99 else want), t


def test_photo_time():
    from iceberg_tracking_code_amd import day_grid
    day = dt.datetime(2019, 7, 24)
    cams = [dict(name="a", correction=12.5), dict(name="b", correction=-40.0)]
    windows = [(day + dt.timedelta(hours=9), day + dt.timedelta(hours=9.5)), (day + dt.timedelta(hours=9.5), day + dt.timedelta(hours=10))]
    plan = day_grid.DayPlan(day, 0.5, 300, windows, cams, [])
    for ps in (1, 2):                # start_datetime_corr of the LAST camera + dt.timedelta(hours = time_window / 2.0)
        assert day_grid.photo_time(plan, 1, ps) == windows[1][0] - dt.timedelta(seconds=-40.0) + dt.timedelta(hours=0.25)
    full = day_grid.DayPlan(day, 24.0, 300, [(day + dt.timedelta(hours=9), day + dt.timedelta(hours=14))], cams, [])
    lo, hi = day + dt.timedelta(hours=9), day + dt.timedelta(hours=14, minutes=30)
    assert day_grid.photo_time(full, 0, 1, lo, hi) == lo + (hi - lo) / 2
    assert day_grid.photo_time(full, 0, 2, lo, hi) == full.windows[0][0] + dt.timedelta(seconds=40.0) + dt.timedelta(hours=12)


@pytest.mark.parametrize("width", (240, 1400))
def test_map_insets_boxes(width):
    from iceberg_tracking_code_amd import map_insets, map_layout, thumbnail_size
    for ps in (1, 2):
        layout = map_layout((0, 9000 if ps == 2 else 6500, 0, 5000), width, ps)
        W, H, k = layout["width"], layout["height"], layout["scale"]
        sizes = [(4000, 3000), None, (3000, 4000), (64, 48)]
        got = map_insets(layout, ps, sizes)
        assert got[1] is None and len(got) == 4
        for n, (size, place) in enumerate(zip(sizes, got)):
            if size is None:
                continue
            left, bottom, bw, bh = ((3 * W) // 100, H - ((6 + 20 * n) * H) // 100, (18 * W) // 100, (18 * H) // 100) if ps == 2 else \
                ((6 * W) // 100, H - (6 * H) // 100, (20 * W) // 100, (20 * H) // 100)
            tw, th = thumbnail_size(size[0], size[1], (bw, bh))
            assert place["box"] == (bw, bh) and place["size"] == (tw, th) == T.size(size[0], size[1], (bw, bh))
            assert place["at"] == (left, bottom - th)                               # anchor='SW'
            assert place["label_at"] == (left + (5 * tw) // 100, bottom - th + (15 * th) // 100 - 7 * k)
            assert 0 <= place["at"][0] and place["at"][0] + tw <= W and 0 <= place["at"][1] and place["at"][1] + th <= H
            # the figure fractions, within a pixel
            fx, fy = (0.03, 0.06 + 0.2 * n) if ps == 2 else (0.06, 0.06)
            assert abs(left - fx * W) < 1 and abs((H - bottom) - fy * H) < 1 and abs(bw - (0.18 if ps == 2 else 0.2) * W) < 1
    with pytest.raises(ValueError):
        map_insets(map_layout((0, 9000, 0, 5000), width, 2), 2, [(64, 48)] * 5)
    assert len(map_insets(map_layout((0, 6500, 0, 5000), width, 1), 1, [(64, 48)] * 5)) == 5


# ---- the host statement of the map with insets ----------------------------------------------------------------------------------
@pytest.mark.parametrize("width,views", [(64, 1), (64, 2), (160, 1), (160, 2)])
def test_overlay_host_with_insets(width, views):
    from iceberg_tracking_code_amd import map_overlay_host
    pic, base = mc.case(width, views, 0)
    assert np.array_equal(map_overlay_host(dict(pic, insets=[])), base)
    assert np.array_equal(map_overlay_host(pic), base)
    seen = set()
    for name, insets in tc.inset_cases(width, pic["height"]).items():
        want = T.paste(base, insets)
        got = map_overlay_host(dict(pic, insets=insets))
        assert np.array_equal(got, want), (name, np.argwhere((got != want).any(axis=2))[:5])
        assert not np.array_equal(want, base)
        seen.add(want.tobytes())
    assert len(seen) == 5                                                           # the two orders of the overlap differ


def test_overlay_host_insets_refusals():
    from iceberg_tracking_code_amd import _lib, map_overlay_host
    pic, _ = mc.case(64, 1, 0)
    H = pic["height"]
    px = np.zeros((9, 13, 3), np.uint8)
    ok = dict(index=0, at=(64 - 13, H - 9), label=(0, 0, "OK"), pixels=px)
    map_overlay_host(dict(pic, insets=[ok] * 8))
    for bad in ([ok] * 9, [dict(ok, at=(64 - 12, H - 9))], [dict(ok, at=(64 - 13, H - 8))], [dict(ok, at=(-1, 0))], [dict(ok, at=(0, -1))],
                [dict(ok, label=(0, 0, "under_score"))], [dict(ok, label=(0, 0, "1" * 49))], [dict(ok, index=8)], [dict(ok, index=-1)],
                [dict(ok, label=((1 << 20) + 1, 0, "far"))], [dict(ok, label=(0, -(1 << 20) - 1, "far"))]):
        with pytest.raises(ValueError):
            map_overlay_host(dict(pic, insets=bad))
    map_overlay_host(dict(pic, insets=[dict(ok, label=(1 << 20, -(1 << 20), "1" * 48))]))
    with pytest.raises(_lib.IcelkError):                                           # an index without a thumbnail
        map_overlay_host(dict(pic, insets=[dict(ok, pixels=None)]))

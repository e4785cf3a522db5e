"""GPU: the cameras' photographs in the velocity map (k_map_inset behind icelk_map_draw_insets, the resident thumbnails of
icelk_map_inset_set_file / _pixels) against the map's restatement with a numpy paste and Pillow's writer --
every byte --, the resident set's states, the call's independence of the other working sets, and the day driver's
`photos=`."""
import ctypes as C
import datetime as dt
import io
import os

import numpy as np
import pytest
from PIL import Image

import day_grid_golden as G
import map_cases as mc
import map_restatement as R
import plot_cases as pc
import thumb_cases as tc
import thumb_restatement as T

pytestmark = pytest.mark.gpu


def _pillow(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def _bare(insets):
    return [{k: v for k, v in q.items() if k != "pixels"} for q in insets]


def _set_all(ctx, insets):
    for q in insets:
        assert ctx.map_inset_set(q["index"], q["pixels"]) == (q["pixels"].shape[1], q["pixels"].shape[0])


@pytest.fixture()
def ictx(ctx):
    """the session's context without resident insets, before and after"""
    ctx.map_inset_release()
    yield ctx
    ctx.map_inset_release()


@pytest.mark.parametrize("width,views", tc.PICTURES)
def test_map_draw_with_insets_equals_restatement_and_pillow(ictx, width, views):
    pic, base = mc.case(width, views, 0)
    plain = ictx.map_draw(pic)
    assert plain == _pillow(base, 90)
    for name, insets in tc.inset_cases(width, pic["height"]).items():
        want = T.paste(base, insets)
        _set_all(ictx, insets)
        for q in (90, 75) if name == "corners" else (90,):
            data, rgb = ictx.map_draw(dict(pic, quality=q, insets=_bare(insets)), want_rgb=True)
            assert np.array_equal(rgb, want), (name, q, np.argwhere((rgb != want).any(axis=2))[:5])
            assert data == _pillow(want, q), (name, q)
        assert ictx.map_draw(dict(pic, insets=_bare(insets))) == _pillow(want, 90)   # without the R G B
        assert ictx.map_draw(pic) == plain                                           # and the plain picture between them
        assert ictx.map_draw(dict(pic, insets=[])) == plain


def _photo(seed=3, size=(64, 48), **kw):
    return jc_encode(pc.frame(size[0], size[1], seed=seed), pc.frame(size[0], size[1], seed=seed + 1), pc.frame(size[0], size[1], seed=seed + 2), **kw)


def jc_encode(r, g, b, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.stack([r, g, b], 2)).save(buf, "JPEG", **dict(dict(quality=90), **kw))
    return buf.getvalue()


def test_set_file_and_set_pixels_give_the_same_picture(ictx):
    from iceberg_tracking_code_amd import thumbnail_host, thumbnail_size
    pic, base = mc.case(160, 2, 0)
    photo = _photo()
    rgb = np.asarray(Image.open(io.BytesIO(photo)).convert("RGB"))
    size = thumbnail_size(64, 48, (30, 30))
    assert size == (30, 23)
    assert ictx.map_inset_set(0, photo, (30, 30)) == size                           # decoded and reduced on the device
    thumb = thumbnail_host(rgb, size)
    assert ictx.map_inset_set(1, thumb) == size                                      # uploaded ready
    assert ictx.map_inset_set(2, rgb, (30, 30)) == size                              # reduced on the host, then uploaded
    want = T.paste(base, [dict(at=(5, 60), label=(7, 62, "CAM"), pixels=T.reduce(rgb, size))])
    files = set()
    for index in (0, 1, 2):
        data, got = ictx.map_draw(dict(pic, insets=[dict(index=index, at=(5, 60), label=(7, 62, "CAM"))]), want_rgb=True)
        assert np.array_equal(got, want), index
        files.add(data)
    assert files == {_pillow(want, 90)}
    # a progressive file: the device refuses it, Pillow and the host statement take over
    prog = _photo(progressive=True)
    assert ictx.map_inset_set(3, prog, (30, 30)) == size
    want = T.paste(base, [dict(at=(5, 60), label=None, pixels=T.reduce(np.asarray(Image.open(io.BytesIO(prog)).convert("RGB")), size))])
    assert np.array_equal(ictx.map_draw(dict(pic, insets=[dict(index=3, at=(5, 60), label=None)]), want_rgb=True)[1], want)
    with pytest.raises(ValueError):
        ictx.map_inset_set(0, photo)                                                 # a file needs a box
    with pytest.raises(ValueError):
        ictx.map_inset_set(8, thumb)
    with pytest.raises(ValueError):
        ictx.map_inset_set(0, b"no jpeg", (30, 30))


def test_states_replacement_and_refusals(ictx):
    from iceberg_tracking_code_amd import Context, _lib, map_descriptor, map_inset_array
    pic, base = mc.case(64, 1, 0)
    H = pic["height"]
    a, b = (np.random.default_rng(k).integers(0, 256, s, dtype=np.uint8) for k, s in ((1, (9, 13, 3)), (2, (5, 21, 3))))
    one = [dict(index=4, at=(10, 10), label=(11, 11, "A"))]
    with pytest.raises(_lib.IcelkError) as e:                                        # nothing resident yet
        ictx.map_draw(dict(pic, insets=one))
    assert e.value.code == _lib.ESTATE
    ictx.map_inset_set(4, a)
    first = ictx.map_draw(dict(pic, insets=one), want_rgb=True)
    assert np.array_equal(first[1], T.paste(base, [dict(one[0], pixels=a)]))
    with pytest.raises(_lib.IcelkError) as e:                                        # another index holds nothing
        ictx.map_draw(dict(pic, insets=[dict(one[0], index=5)]))
    assert e.value.code == _lib.ESTATE
    ictx.map_inset_set(4, b)                                                         # replacing an index
    second = ictx.map_draw(dict(pic, insets=one), want_rgb=True)
    assert np.array_equal(second[1], T.paste(base, [dict(one[0], pixels=b)])) and second[0] != first[0]
    # n_insets = 0 gives icelk_map_draw's bytes; refusals write nothing
    plain = ictx.map_draw(pic)
    n = C.c_uint64(77)
    buf = np.full(len(plain) + 64, 0xAA, np.uint8)

    def call(insets, count=None, cap=buf.size, handle=ictx):
        d, keep = map_descriptor(pic)
        arr, m = map_inset_array(insets)
        return handle._lib.icelk_map_draw_insets(handle._h, C.byref(d), arr, m if count is None else count, None, 0, C.c_void_p(buf.ctypes.data), cap, C.byref(n))
    assert call([]) == _lib.OK and buf[:n.value].tobytes() == plain and n.value == len(plain)
    assert ictx._lib.icelk_map_draw_insets(ictx._h, C.byref(map_descriptor(pic)[0]), None, 0, None, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)) == _lib.OK
    assert buf[:n.value].tobytes() == plain
    buf[:] = 0xAA
    n.value = 77
    fits = dict(index=4, at=(64 - 21, H - 5), label=None)
    for bad, code in (([dict(fits, at=(64 - 20, H - 5))], _lib.EARG), ([dict(fits, at=(64 - 21, H - 4))], _lib.EARG), ([dict(fits, at=(-1, 0))], _lib.EARG),
                      ([dict(fits, index=8)], _lib.EARG), ([dict(fits, index=-1)], _lib.EARG), ([dict(fits, index=0)], _lib.ESTATE),
                      ([dict(fits, label=(0, 0, "a_b"))], _lib.EARG), ([dict(fits, label=(0, 0, "1" * 49))], _lib.EARG),
                      ([dict(fits, label=((1 << 20) + 1, 0, "x"))], _lib.EARG), ([dict(fits, label=(0, -(1 << 20) - 1, "x"))], _lib.EARG)):
        assert call(bad) == code, bad
    assert call([fits], count=9) == _lib.EARG and call([fits], count=-1) == _lib.EARG
    assert ictx._lib.icelk_map_draw_insets(ictx._h, C.byref(map_descriptor(pic)[0]), None, 1, None, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)) == _lib.EARG
    assert n.value == 77 and (buf == 0xAA).all()
    assert call([fits], cap=10) == _lib.ECAP and n.value > 10 and (buf == 0xAA).all()   # and the repeat
    assert call([fits]) == _lib.OK
    want = T.paste(base, [dict(fits, pixels=b)])
    assert buf[:n.value].tobytes() == _pillow(want, 90)
    with pytest.raises(ValueError):
        ictx.map_draw(dict(pic, insets=[fits] * 9))
    for args in ((4, None, 3, 3, 9), (4, b.ctypes.data_as(_lib.u8p), 0, 3, 9), (4, b.ctypes.data_as(_lib.u8p), 3, 16385, 9), (4, b.ctypes.data_as(_lib.u8p), 21, 5, 62),
                 (8, b.ctypes.data_as(_lib.u8p), 21, 5, 63)):
        assert ictx._lib.icelk_map_inset_set_pixels(ictx._h, *args) == _lib.EARG
    photo = _photo()
    for index, tw, th in ((8, 10, 10), (0, 65, 10), (0, 10, 49), (0, 0, 10)):
        assert ictx._lib.icelk_map_inset_set_file(ictx._h, index, photo, len(photo), tw, th) == _lib.EARG
    assert ictx.map_draw(dict(pic, insets=one), want_rgb=True)[0] == second[0]      # what the index held, it holds
    ictx.map_inset_release()
    with pytest.raises(_lib.IcelkError) as e:
        ictx.map_draw(dict(pic, insets=one))
    assert e.value.code == _lib.ESTATE
    ictx.map_inset_release()                                                         # releasing nothing is fine
    assert ictx.map_draw(pic) == plain
    # a fresh handle: freed with the handle that still holds thumbnails
    with Context(64, 48, n_slots=1, max_pts=64) as fresh:
        with pytest.raises(_lib.IcelkError):
            fresh.map_draw(dict(pic, insets=one))
        fresh.map_inset_set(4, photo, (20, 20))
        fresh.map_inset_set(7, a)
        assert fresh.map_draw(dict(pic, insets=one))


def test_insets_beside_the_other_working_sets(ictx):
    """the thumbnail's decode uses the synchronous decoder's buffers and the map's working set is its own: a segment picture, a
    re-save and a crop job give the same files with maps with insets drawn, and photos made resident, in between as without"""
    w, h, width = pc.SHAPES[0]
    gray, tracks, stamp, _ = pc.case(w, h, width, 3)
    photo3 = np.stack([pc.frame(160, 120, seed=5), pc.frame(160, 120, seed=6), pc.frame(160, 120, seed=7)], 2)
    source = _pillow(photo3, 92)
    pic, base = mc.case(96, 2, 1)
    inset = dict(index=0, at=(3, 30), label=(4, 31, "UAS7"))
    small = _photo()
    want = T.paste(base, [dict(inset, pixels=T.reduce(np.asarray(Image.open(io.BytesIO(small)).convert("RGB")), (20, 15)))])
    ictx.upload_gray(0, gray)

    def with_insets(quality=90):
        assert ictx.map_inset_set(0, small, (20, 20)) == (20, 15)
        assert ictx.map_draw(dict(pic, quality=quality, insets=[inset])) == _pillow(want, quality)

    def others(draw):
        out = []
        ticket = ictx.jpeg_crop_start(source, crop=(8, 8, 120, 100), quality=75)
        if draw:
            with_insets()
        out.append(ictx.plot_tracks(0, tracks, width, stamp, 85))
        ictx.jpeg_resave_rgb(photo3, 80)
        if draw:
            with_insets()
        out.append(ictx.jpeg_resave_file())
        out.append(ictx.map_draw(pic))
        if draw:
            with_insets(60)
        out.append(ictx.map_draw(pic))
        out.append(ictx.jpeg_crop_finish(ticket)[0])
        out.append(ictx.plot_tracks(0, tracks, width, stamp, 85))
        return out
    without, with_maps = others(False), others(True)
    assert without == with_maps and all(len(f) > 100 for f in without)
    assert without[2] == without[3] == _pillow(base, 90)
    assert np.array_equal(ictx.download_level(0, 0), gray)


# ---- the day driver ----------------------------------------------------------------------------------------------------
WIDTH, QUALITY, VMAX = 240, 85, 0.3
# seconds from a window's photo time to the camera's photo; windows without an entry have none.  camB's photo of window 5
# is exactly 300 s away and must not be used; camC has no folder at all; camE has photos and no tracks; camD no row
OFFSETS = {"camA": {0: 100, 2: 100, 4: 100, 8: 100}, "camB": {3: -299, 4: -299, 5: 300, 7: -299, 9: -299}, "camC": {}, "camE": {w: 0 for w in range(10)}}


@pytest.fixture(scope="module")
def day(tmp_path_factory):
    from iceberg_tracking_code_amd import day_grid
    z = G.load()
    root = tmp_path_factory.mktemp("inset_day")
    G.build_tree(z, str(root / "in"))
    camnames, schedule, drifts, fjord, day, grid_size, thr = G.args(z)
    fx, fy = fjord["x"], fjord["y"]
    cameras = [dict(camera=c, start_day=20190701, end_day=20190831, easting=float(fx.min() + 300.0 + 700.0 * k), northing=float(fy.min() + 150.0 + 500.0 * k))
               for k, c in enumerate(camnames) if c != "camD"]
    plan = day_grid.plan_day(camnames, str(root / "in"), "utm", schedule, drifts, day, 0.5, grid_size)
    assert plan.cameras[-1]["name"] == "camE" and plan.cameras[-1]["correction"] == 0 and len(plan.windows) == 10
    photos = root / "photos"
    OFFSETS["camC"] = {3: 10, 8: 10}
    seed = 0
    for cam, offsets in OFFSETS.items():
        if cam == "camC":
            continue
        for w, off in offsets.items():
            when = day_grid.photo_time(plan, w, 1) + dt.timedelta(seconds=off)
            folder = photos / cam / (when - dt.timedelta(hours=8)).strftime("%Y%m%d")
            folder.mkdir(parents=True, exist_ok=True)
            seed += 1
            (folder / when.strftime("%Y%m%d-%H%M%S.jpg")).write_bytes(_photo(seed=10 * seed, subsampling=seed % 3))
    # camC: its folder of the day is there and holds what is no photo of the day's
    (photos / "camC" / "20190724").mkdir(parents=True)
    (photos / "camC" / "20190724" / "readme.jpg").write_bytes(b"")
    for w in (3, 8):
        when = day_grid.photo_time(plan, w, 1) + dt.timedelta(seconds=10)
        (photos / "camC" / "20190724" / when.strftime("%Y%m%d-%H%M%S.jpg")).write_bytes(_photo(seed=500 + w, size=(48, 64)))
    return dict(z=z, root=root, args=(camnames, str(root / "in"), "utm"), schedule=schedule, drifts=drifts, fjord=fjord, day=day, grid_size=grid_size,
                thr=thr, cameras=cameras, photos=str(photos), plan=plan)


def _run(ctx, d, out, time_window, **kw):
    from iceberg_tracking_code_amd import utm_to_gridded_utm
    target = d["root"] / out
    target.mkdir()
    got = utm_to_gridded_utm(*d["args"], str(target), d["schedule"], d["drifts"], d["fjord"], d["day"], time_window, d["grid_size"], d["thr"], ctx=ctx, **kw)
    return target, got


def _files(path):
    out = {}
    for name in sorted(os.listdir(str(path))):
        with open(os.path.join(str(path), name), "rb") as f:
            out[name] = f.read()
    return out


def _window_vectors(d, plan, w):
    """s3's selection restated with numpy (camera by camera, hour by hour, time >= start & time < end): what the all-vectors
    panel draws -- x, y, u * interval, v * interval, speed -- and the cameras that selected something"""
    z = d["z"]
    files = {(str(z["in_%02d_cam" % k]), str(z["in_%02d_name" % k])[:13]): k for k in range(int(z["in_n"]))}
    parts, cams = [], []
    for cam in plan.cameras:
        n_before = len(parts)
        for hour in cam["hours"][w]:
            k = files.get((cam["name"], hour.strftime("%Y%m%d_%H00")))
            if k is None:
                continue
            a = {key: z["in_%02d_%s" % (k, key)].astype(np.float64) for key in ("x", "y", "u", "v", "speed", "time")}
            m = (a["time"] >= cam["lo"][w]) & (a["time"] < cam["hi"][w])
            interval = float(str(z["in_%02d_name" % k]).split("_")[2].split("s")[0])
            parts.append(np.column_stack([a["x"][m], a["y"][m], a["u"][m] * interval, a["v"][m] * interval, a["speed"][m]]))
        if sum(len(p) for p in parts[n_before:]):
            cams.append(cam["name"])
    return np.concatenate(parts) if parts else np.zeros((0, 5)), cams


@pytest.mark.parametrize("plot_switch", (1, 2))
def test_day_driver_puts_the_photographs_in(ictx, day, plot_switch):
    from iceberg_tracking_code_amd import _lib, closest_image, day_grid, map_insets, map_layout, map_name, map_picture, map_strings, map_view
    d, plan = day, day["plan"]
    kw = dict(plot_switch=plot_switch, speedthreshold_cbar=VMAX, cameras=d["cameras"], out_width=WIDTH, quality=QUALITY)
    target, got = _run(ictx, d, "photos_%d" % plot_switch, 0.5, plots=str(d["root"] / ("plots_photos_%d" % plot_switch)), photos=d["photos"], **kw)
    plain, want = _run(ictx, d, "plain_%d" % plot_switch, 0.5, plots=str(d["root"] / ("plots_plain_%d" % plot_switch)), **kw)
    bare, _ = _run(ictx, d, "bare_%d" % plot_switch, 0.5)
    # the .npz files do not change
    assert [n for n, _ in got] == [n for n, _ in want] == [n for n, _ in G.outputs(d["z"], 0)]
    assert _files(target) == _files(plain) == _files(bare) and len(_files(target)) == 10
    pictures, plain_pictures = _files(d["root"] / ("plots_photos_%d" % plot_switch)), _files(d["root"] / ("plots_plain_%d" % plot_switch))
    assert sorted(pictures) == sorted(plain_pictures) and len(pictures) == 10
    names = [c["name"] for c in plan.cameras]
    positions = [(r["easting"], r["northing"]) for r in d["cameras"]]
    by_name = dict(got)
    layout = map_layout(map_view(d["fjord"], plot_switch), WIDTH, plot_switch)
    counts = []
    for w, (start, end) in enumerate(plan.windows):
        a = by_name["{}-{}_30min_{}m.npz".format(start.strftime("%Y%m%d_%H%M"), end.strftime("%H%M"), d["grid_size"])]
        vectors, cams = _window_vectors(d, plan, w)
        when = start + dt.timedelta(minutes=15)                                      # the last scheduled camera, camE, has no drift
        assert when == day_grid.photo_time(plan, w, plot_switch)
        chosen = [closest_image(os.path.join(d["photos"], cam), when) for cam in cams]
        if w == 5:
            assert "camB" in cams and chosen[cams.index("camB")] is None and os.path.exists(os.path.join(d["photos"], "camB", "20190724", "20190724-115000.jpg"))
        if plot_switch == 1:                                                         # the last camera that has a photo, in the one box
            last = [k for k, p in enumerate(chosen) if p is not None][-1:]
            cams, chosen = [cams[k] for k in last], [chosen[k] for k in last]
        rgbs = [None if p is None else np.asarray(Image.open(p).convert("RGB")) for p in chosen]
        places = map_insets(layout, plot_switch, [None if r is None else (r.shape[1], r.shape[0]) for r in rgbs])
        insets = [dict(at=p["at"], label=(p["label_at"][0], p["label_at"][1], cam), pixels=T.reduce(r, T.size(r.shape[1], r.shape[0], p["box"])))
                  for cam, r, p in zip(cams, rgbs, places) if p is not None]
        counts.append(len(insets))
        name = os.path.basename(map_name("", start, end))
        if not insets:
            assert pictures[name] == plain_pictures[name], name                      # no photo: the picture plots= alone writes
            continue
        _, all_cams = _window_vectors(d, plan, w)
        strings = map_strings(d["day"], start, end, all_cams, d["grid_size"])
        pic = map_picture(d["fjord"], d["grid_size"], a["measured"], a["not_measured"], a["x"], a["y"], a["u"], a["v"], a["speed"], strings,
                          cameras=positions, label=positions[0], n_camnames=len(names), plot_switch=plot_switch, vectors=vectors,
                          speedthreshold_cbar=VMAX, out_width=WIDTH, quality=QUALITY)
        assert pictures[name] == _pillow(T.paste(R.render(pic), insets), QUALITY), name
        assert pictures[name] != plain_pictures[name]
    # w: 0 A, 1 none, 2 A, 3 B and C (one map: C), 4 A and B (one map: B), 5 none (300 s), 6 none, 7 B, 8 A and C, 9 B
    assert counts == ([1, 0, 1, 1, 1, 0, 0, 1, 1, 1] if plot_switch == 1 else [1, 0, 1, 2, 2, 0, 0, 1, 2, 1])
    with pytest.raises(_lib.IcelkError):                                             # the insets of the day are gone from the handle again
        ictx.map_draw(dict(pic, insets=[dict(index=0, at=(0, 0), label=None)]))


def test_day_driver_photos_keyword(ictx, day, monkeypatch):
    from iceberg_tracking_code_amd import Context
    with pytest.raises(ValueError):
        _run(ictx, day, "photos_without_plots", 0.5, photos=day["photos"])
    # the full day draws too (one map: the middle of the rounded first and last selected times)
    plots = str(day["root"] / "plots_full")
    _run(ictx, day, "full", 24.0, plots=plots, photos=day["photos"], cameras=day["cameras"], out_width=WIDTH)
    assert os.listdir(plots) == ["20190724_0900-1400.jpg"]
    # photos=None calls nothing new
    called = []
    for name in ("map_inset_set", "map_inset_release", "jpeg_thumb_file"):
        monkeypatch.setattr(Context, name, lambda self, *a, **k: called.append(a))
    real = ictx._lib

    class Watch:
        def __getattr__(self, name):
            if name.startswith("icelk_map_inset") or name in ("icelk_map_draw_insets", "icelk_jpeg_thumb_file", "icelk_thumb_host", "icelk_thumb_size",
                                                               "icelk_map_overlay_insets_host"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ictx, "_lib", Watch())
    target, got = _run(ictx, day, "default", 0.5, plots=str(day["root"] / "plots_default"), cameras=day["cameras"], out_width=WIDTH)
    assert len(got) == 10 and not called

"""GPU: the velocity map rasterised and coded on the device (csrc/k_map.hip, abi_map.hip) against the numpy
restatement and Pillow's writer -- every byte --, its determinism under contended atomics, the group filter on resident
arrows, its refusals, its independence of the other JPEG working sets, and the day driver's `plots=`."""
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

pytestmark = pytest.mark.gpu


def _pillow(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


@pytest.mark.parametrize("width,views,variant", mc.CASES)
def test_map_draw_equals_restatement_and_pillow(ctx, width, views, variant):
    pic, want = mc.case(width, views, variant)
    for q in (75, 90, 100) if variant == 0 else (90,):
        data, rgb = ctx.map_draw(dict(pic, quality=q), want_rgb=True)
        assert np.array_equal(rgb, want), (q, np.argwhere((rgb != want).any(axis=2))[:5])
        assert data == _pillow(want, q), q
        assert Image.open(io.BytesIO(data)).size == (width, (3 * width) // 4)
    assert ctx.map_draw(pic) == _pillow(want, 90)                                    # without the R G B


def _crowd(n=20000, width=96):
    """n arrows of random colours, half of them heaped on one spot"""
    height, base = mc.views_of(width, 1)
    _, _, vw, vh = base[0]["view"]
    rng = np.random.default_rng(17)
    centre = (mc.X0 + mc.M * vw / 2, mc.Y0 + mc.M * vh / 2)
    at = np.where(rng.random((n, 1)) < 0.5, rng.normal(centre, 40.0, (n, 2)), rng.uniform((mc.X0 - 100, mc.Y0 - 100), (mc.X0 + mc.M * vw + 100, mc.Y0 + mc.M * vh + 100), (n, 2)))
    arrows = np.column_stack([at, rng.normal(0, 120.0, (n, 2)), rng.uniform(0, 0.6, n)])
    panel = dict(base[0], arrows=arrows, pivot="tail", width=15.0, alpha=0.75, vmax=0.5)
    return dict(width=width, height=height, quality=90, table=mc.table(), texts=[(2, 1, "20000 arrows")], panels=[panel])


def test_determinism_under_contention(ctx):
    pic = _crowd()
    want = R.render(pic)
    _, top, count = R.planes(pic)
    assert count.max() > 500 and len(np.unique(top)) > 500                            # contended, and many colours on top
    a = ctx.map_draw(pic, want_rgb=True)
    b = ctx.map_draw(pic, want_rgb=True)
    assert np.array_equal(a[1], want)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[0] == _pillow(want, 90)


def test_group_filter_on_resident_arrows(ctx):
    from iceberg_tracking_code_amd import _lib
    pic, want_all = mc.case(96, 1, 0)
    arrows = pic["panels"][0]["arrows"]
    group = (np.arange(len(arrows)) % 3).astype(np.int32)
    resident = dict(pic, panels=[dict({k: v for k, v in pic["panels"][0].items() if k != "arrows"}, resident=True)])
    with pytest.raises(_lib.IcelkError) as e:                                        # nothing resident yet
        ctx.map_draw(resident)
    assert e.value.code == _lib.ESTATE
    ctx.map_arrows_set(arrows, group)
    try:
        files = {}
        for g in (0, 1, 2, -1, 5):
            p = dict(resident, panels=[dict(resident["panels"][0], group=g)])
            data, rgb = ctx.map_draw(p, want_rgb=True)
            assert np.array_equal(rgb, R.render(p, arrows, group)), g
            assert data == _pillow(rgb, 90)
            files[g] = data
        assert np.array_equal(ctx.map_draw(dict(resident, panels=[dict(resident["panels"][0], group=-1)]), want_rgb=True)[1], want_all)
        assert len(set(files.values())) == 5
        for g in (0, 1, 2, -1, 5):                                                   # drawing the others changed none of them
            assert ctx.map_draw(dict(resident, panels=[dict(resident["panels"][0], group=g)])) == files[g]
        # both panels of one picture from the one upload: all of them on the left, one group on the right
        two, _ = mc.case(160, 2, 0)
        panels = [dict({k: v for k, v in q.items() if k != "arrows"}, resident=True, group=g) for q, g in zip(two["panels"], (-1, 1))]
        p2 = dict(two, panels=panels)
        assert np.array_equal(ctx.map_draw(p2, want_rgb=True)[1], R.render(p2, arrows, group))
        # a set without groups: one group cannot be asked for
        ctx.map_arrows_set(arrows)
        with pytest.raises(_lib.IcelkError) as e:
            ctx.map_draw(dict(resident, panels=[dict(resident["panels"][0], group=1)]))
        assert e.value.code == _lib.ESTATE
        assert np.array_equal(ctx.map_draw(resident, want_rgb=True)[1], want_all)
    finally:
        ctx.map_arrows_release()
    with pytest.raises(_lib.IcelkError):
        ctx.map_draw(resident)
    ctx.map_arrows_release()                                                         # releasing nothing is fine


def test_capacity_arguments_and_state(ctx):
    from iceberg_tracking_code_amd import Context, _lib, map_descriptor
    pic, want = mc.case(64, 2, 0)
    whole = _pillow(want, 90)
    n = C.c_uint64(0)
    buf = np.full(len(whole) + 16, 0xAA, np.uint8)

    def call(cap, handle=ctx, change=None, length=n):
        d, keep = map_descriptor(pic)
        if change:
            change(d)
        return handle._lib.icelk_map_draw(handle._h, C.byref(d), None, 0, C.c_void_p(buf.ctypes.data), cap, C.byref(length) if length is not None else None)
    assert call(len(whole) - 1) == _lib.ECAP and n.value == len(whole) and (buf == 0xAA).all()
    assert call(0) == _lib.ECAP and n.value == len(whole)
    assert call(len(whole)) == _lib.OK and n.value == len(whole) and buf[:len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAA).all()
    # refused before anything is enqueued, nothing written
    buf[:] = 0xAA
    n.value = 77
    cams = np.zeros((9, 2))
    for change in (lambda d: setattr(d, "quality", 0), lambda d: setattr(d, "quality", 101), lambda d: setattr(d, "width", 63),
                   lambda d: setattr(d, "n_texts", 17), lambda d: setattr(d.text[2], "text", b"12h30_"), lambda d: setattr(d.text[2], "text", b"1" * 49),
                   lambda d: (setattr(d.panel[0], "cameras", cams.ctypes.data), setattr(d.panel[0], "n_cameras", 9)),
                   lambda d: setattr(d.panel[1], "x0", d.panel[0].x0), lambda d: setattr(d.panel[1], "w", d.width), lambda d: setattr(d, "n_panels", 3),
                   lambda d: setattr(d.panel[0], "n_arrows", (1 << 27) + 1), lambda d: setattr(d, "table", None)):
        assert call(buf.size, change=change) == _lib.EARG
    assert call(buf.size, length=None) == _lib.EARG
    assert ctx._lib.icelk_map_draw(ctx._h, None, None, 0, None, 0, C.byref(n)) == _lib.EARG
    assert ctx._lib.icelk_map_draw(None, None, None, 0, None, 0, C.byref(n)) == _lib.EARG
    assert call(buf.size, change=lambda d: setattr(d.panel[0], "resident", 1)) == _lib.ESTATE
    assert n.value == 77 and (buf == 0xAA).all()
    with pytest.raises(ValueError):
        ctx.map_draw(dict(pic, quality=0))
    with pytest.raises(ValueError):
        ctx.map_arrows_set(np.zeros((3, 5)), np.zeros(2, np.int32))
    assert ctx._lib.icelk_map_arrows_set(ctx._h, None, None, 3) == _lib.EARG
    assert ctx._lib.icelk_map_arrows_set(ctx._h, None, None, -1) == _lib.EARG
    # a fresh handle: the working set is allocated at the first picture, and freed with the handle that still holds arrows
    with Context(64, 48, n_slots=1, max_pts=64) as fresh:
        assert call(buf.size, handle=fresh, change=lambda d: setattr(d.panel[0], "resident", 1)) == _lib.ESTATE and (buf == 0xAA).all()
        assert fresh.map_draw(pic) == whole
        fresh.map_arrows_set(np.zeros((0, 5)))
        assert fresh.map_draw(dict(pic, panels=[dict(pic["panels"][0], resident=True)] + pic["panels"][1:]))
        fresh.map_arrows_set(pic["panels"][0]["arrows"])


def test_map_beside_segment_picture_and_crop_job(ctx):
    """the map's working set is its own: a segment picture, a re-save and a crop job give the same files with maps drawn in
    between as without"""
    w, h, width = pc.SHAPES[0]
    gray, tracks, stamp, _ = pc.case(w, h, width, 3)
    photo = np.stack([pc.frame(160, 120, seed=5), pc.frame(160, 120, seed=6), pc.frame(160, 120, seed=7)], 2)
    source = _pillow(photo, 92)
    pic, want = mc.case(96, 2, 1)
    ctx.upload_gray(0, gray)

    def others(draw):
        out = []
        ticket = ctx.jpeg_crop_start(source, crop=(8, 8, 120, 100), quality=75)
        if draw:
            assert ctx.map_draw(pic) == _pillow(want, 90)
        out.append(ctx.plot_tracks(0, tracks, width, stamp, 85))
        ctx.jpeg_resave_rgb(photo, 80)
        if draw:
            assert ctx.map_draw(pic) == _pillow(want, 90)
        out.append(ctx.jpeg_resave_file())
        if draw:
            assert ctx.map_draw(dict(pic, quality=60)) == _pillow(want, 60)
        out.append(ctx.jpeg_crop_finish(ticket)[0])
        out.append(ctx.plot_tracks(0, tracks, width, stamp, 85))
        return out
    without, with_maps = others(False), others(True)
    assert without == with_maps and all(len(f) > 100 for f in without)
    assert np.array_equal(ctx.download_level(0, 0), gray)


# ---- the day driver ----------------------------------------------------------------------------------------------------
WIDTH, QUALITY, VMAX = 240, 85, 0.3


@pytest.fixture(scope="module")
def day(tmp_path_factory):
    z = G.load()
    root = tmp_path_factory.mktemp("map_day")
    G.build_tree(z, str(root / "in"))
    camnames, schedule, drifts, fjord, day, grid_size, thr = G.args(z)
    fx, fy = fjord["x"], fjord["y"]
    cameras = [dict(camera=c, start_day=20190701, end_day=20190831, easting=float(fx.min() + 300.0 + 700.0 * k), northing=float(fy.min() + 150.0 + 500.0 * k))
               for k, c in enumerate(camnames) if c != "camD"]                      # camD has two rows in the schedule: no camera drawn either
    return dict(z=z, root=root, args=(camnames, str(root / "in"), "utm"), schedule=schedule, drifts=drifts, fjord=fjord, day=day, grid_size=grid_size,
                thr=thr, cameras=cameras)


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
    """s3's selection restated with numpy (camera by camera, hour by hour, time >= start & time < end), with what the
    all-vectors panel draws: x, y, u * interval, v * interval, speed; and the cameras that selected something"""
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
def test_day_driver_writes_the_maps(ctx, day, plot_switch):
    from iceberg_tracking_code_amd import day_grid, map_name, map_picture, map_strings
    d = day
    kw = dict(plots=str(d["root"] / ("plots_%d" % plot_switch)), plot_switch=plot_switch, speedthreshold_cbar=VMAX, cameras=d["cameras"], out_width=WIDTH,
              quality=QUALITY)
    target, got = _run(ctx, d, "with_%d" % plot_switch, 0.5, **kw)
    plain, want = _run(ctx, d, "without_%d" % plot_switch, 0.5)
    # the .npz files do not change
    assert [n for n, _ in got] == [n for n, _ in want] == [n for n, _ in G.outputs(d["z"], 0)]
    assert _files(target) == _files(plain) and len(_files(target)) == 10
    # one picture per written window, named as the reference names it
    pictures = _files(kw["plots"])
    assert sorted(pictures) == sorted(n.split("_30min")[0] + ".jpg" for n, _ in got)
    plan = day_grid.plan_day(d["args"][0], d["args"][1], d["args"][2], d["schedule"], d["drifts"], d["day"], 0.5, d["grid_size"])
    names = [c["name"] for c in plan.cameras]
    assert names == ["camA", "camB", "camC", "camE"]
    positions = [(r["easting"], r["northing"]) for r in d["cameras"]]
    by_name = dict(got)
    seen_vectors = 0
    for w, (start, end) in enumerate(plan.windows):
        npz = "{}-{}_30min_{}m.npz".format(start.strftime("%Y%m%d_%H%M"), end.strftime("%H%M"), d["grid_size"])
        if npz not in by_name:
            continue
        a = by_name[npz]
        vectors, cams = _window_vectors(d, plan, w)
        seen_vectors += len(vectors)
        strings = map_strings(d["day"], start, end, cams, d["grid_size"])
        pic = map_picture(d["fjord"], d["grid_size"], a["measured"], a["not_measured"], a["x"], a["y"], a["u"], a["v"], a["speed"], strings,
                          cameras=positions, label=positions[0], n_camnames=len(names), plot_switch=plot_switch, vectors=vectors,
                          speedthreshold_cbar=VMAX, out_width=WIDTH, quality=QUALITY)
        assert len(pic["panels"]) == plot_switch and pic["width"] == WIDTH
        name = os.path.basename(map_name(kw["plots"], start, end))
        assert pictures[name] == _pillow(R.render(pic), QUALITY), name
        assert Image.open(io.BytesIO(pictures[name])).size == (WIDTH, pic["height"])
    assert seen_vectors > 5000
    # the arrows of the day are gone from the handle again
    from iceberg_tracking_code_amd import _lib
    with pytest.raises(_lib.IcelkError):
        ctx.map_draw(dict(pic, panels=[dict(pic["panels"][-1], resident=True)]))


def test_day_driver_full_day_name(ctx, day):
    d = day
    plots = str(d["root"] / "plots_full")
    target, got = _run(ctx, d, "with_full", 24.0, plots=plots, plot_switch=2, cameras=d["cameras"], out_width=WIDTH)
    assert [n for n, _ in got] == ["20190724_0900-1400_full_day_300m.npz"]
    assert os.listdir(plots) == ["20190724_0900-1400.jpg"]
    im = Image.open(os.path.join(plots, "20190724_0900-1400.jpg"))
    assert im.size[0] == WIDTH
    with pytest.raises(ValueError):
        _run(ctx, d, "bad_switch", 24.0, plots=plots, plot_switch=3)


def test_day_driver_default_runs_nothing_new(ctx, day, monkeypatch):
    from iceberg_tracking_code_amd import Context
    called = []
    for name in ("map_draw", "map_arrows_set", "map_arrows_release"):
        monkeypatch.setattr(Context, name, lambda self, *a, **k: called.append(a))
    real = ctx._lib

    class Watch:
        def __getattr__(self, name):
            if name.startswith("icelk_map_"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ctx, "_lib", Watch())
    target, got = _run(ctx, day, "default", 0.5)
    assert len(got) == 10 and not called
    assert sorted(os.listdir(str(target))) == sorted(n for n, _ in got)             # the .npz files and nothing else

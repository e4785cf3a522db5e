"""GPU: the movie of the pictures (csrc/k_resize.hip, abi_movie.hip, movie.py).  The scaler on the device
against its host statement on every case of the host list -- one tap and 1025 taps, enlargement and reduction, a skipped
pass on either axis, widths that are no multiples of 4 --; the frame of a picture, file and R G B, against the host
statements; the cached tables, the short file buffer, the picture calls left as they were; and the drivers' `movie=`."""
import ctypes as C
import datetime as dt
import io
import os

import numpy as np
import pytest
from PIL import Image

import day_grid_golden as G
import map_cases as mc
import movie_restatement as R
import plot_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fill", R.FILLS)
@pytest.mark.parametrize("src,dst", R.CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d in R.CASES])
def test_resize_rgb_equals_the_host_statement(ctx, src, dst, fill):
    from iceberg_tracking_code_amd import resize_host
    rgb = R.pixels(src, fill)
    got = ctx.resize_rgb(rgb, dst)
    assert got.shape == (dst[1], dst[0], 3)
    want = resize_host(rgb, dst)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]


def test_resize_rgb_identity_strides_and_refusals(ctx):
    from iceberg_tracking_code_amd import resize_host
    rgb = R.pixels((37, 23), "random")
    assert np.array_equal(ctx.resize_rgb(rgb, (37, 23)), rgb)                         # both passes skipped
    wide = R.pixels((39, 23), "random")[:, :37]                                       # rows 117 bytes apart
    assert np.array_equal(ctx.resize_rgb(wide, (64, 48)), resize_host(wide, (64, 48)))
    for size in ((0, 4), (4, 16385)):
        with pytest.raises(ValueError):
            ctx.resize_rgb(rgb, size)


def test_picture_frame_before_any_picture():
    from iceberg_tracking_code_amd import Context, _lib
    with Context(64, 48, n_slots=1, max_pts=64) as fresh:
        with pytest.raises(_lib.IcelkError) as e:
            fresh.picture_frame((48, 32))
        assert e.value.code == _lib.ESTATE
        with pytest.raises(_lib.IcelkError):
            fresh.picture_size()


def _plot(ctx, want_rgb=True):
    gray, tracks, stamp, _ = pc.case(64, 48, 24, 3)
    ctx.upload_gray(0, gray)
    return ctx.plot_tracks(0, tracks, 24, stamp, 85, want_rgb=want_rgb)


def _map(ctx, want_rgb=True, format="jpeg"):
    return ctx.map_draw(mc.picture(96, 2, 1), want_rgb=want_rgb, format=format)


@pytest.mark.parametrize("draw", [_plot, _map], ids=["plot_tracks", "map_draw"])
@pytest.mark.parametrize("quality", [75, 90])
def test_frame_of_a_picture_equals_the_host(ctx, draw, quality):
    from iceberg_tracking_code_amd import frame_host, movie_size, resize_host
    before = draw(ctx, want_rgb=False)
    data, rgb = draw(ctx)
    assert data == before
    h, w = rgb.shape[:2]
    assert ctx.picture_size() == (w, h)
    for size in (movie_size(w, h, 160), movie_size(w, h, 0), (w + 3, h)):             # larger; its own width; one pass skipped
        frame, frame_rgb = ctx.picture_frame(size, quality, want_rgb=True)
        assert np.array_equal(frame_rgb, resize_host(rgb, size)), size
        assert frame == frame_host(rgb, size, quality), size
        assert ctx.picture_frame(size, quality) == frame                               # again, without the R G B: cached tables
    # the picture calls return what they returned before, and the frame of the same picture is the same
    again, rgb_again = draw(ctx)
    assert again == data and np.array_equal(rgb_again, rgb)
    assert ctx.picture_frame(movie_size(w, h, 160), quality) == frame_host(rgb, movie_size(w, h, 160), quality)


def test_frame_after_a_png_map_is_the_jpeg_forms(ctx):
    from iceberg_tracking_code_amd import movie_size
    _, rgb = _map(ctx)
    size = movie_size(rgb.shape[1], rgb.shape[0], 200)
    want = ctx.picture_frame(size, 90, want_rgb=True)
    _, rgb_png = _map(ctx, format="png")
    got = ctx.picture_frame(size, 90, want_rgb=True)
    assert np.array_equal(rgb_png, rgb) and got[0] == want[0] and np.array_equal(got[1], want[1])


def test_frame_short_buffer_then_the_repeat(ctx):
    from iceberg_tracking_code_amd import _lib, frame_host
    _, rgb = _plot(ctx)
    size = (48, 32)
    whole = frame_host(rgb, size, 90)
    n = C.c_uint64(0)
    buf = np.full(len(whole) + 16, 0xAA, np.uint8)

    def call(cap):
        return ctx._lib.icelk_picture_frame(ctx._h, size[0], size[1], 90, None, 0, C.c_void_p(buf.ctypes.data), cap, C.byref(n))
    for cap in (len(whole) - 1, 0):
        n.value = 0
        assert call(cap) == _lib.ECAP and n.value == len(whole) and (buf == 0xAA).all(), cap
    assert call(len(whole)) == _lib.OK and n.value == len(whole)
    assert buf[:len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAA).all()
    # refusals: a null length, a side outside the limits, a quality outside 1 .. 100, a short R G B stride
    small = np.zeros((32, 48, 3), np.uint8)
    ptr = small.ctypes.data_as(_lib.u8p)
    assert ctx._lib.icelk_picture_frame(ctx._h, 48, 32, 90, None, 0, None, 0, None) == _lib.EARG
    assert ctx._lib.icelk_picture_frame(ctx._h, 16385, 32, 90, None, 0, None, 0, C.byref(n)) == _lib.EARG
    assert ctx._lib.icelk_picture_frame(ctx._h, 48, 32, 101, None, 0, None, 0, C.byref(n)) == _lib.EARG
    assert ctx._lib.icelk_picture_frame(ctx._h, 48, 32, 90, ptr, 3 * 48 - 1, None, 0, C.byref(n)) == _lib.EARG


def test_movie_writer_on_the_device_equals_the_host(ctx, tmp_path):
    from iceberg_tracking_code_amd import MovieWriter, frame_host, read_avi
    _, plot_rgb = _plot(ctx)
    other = R.pixels((24, 18), "random")
    with MovieWriter(tmp_path / "m.avi", width=64) as mv:
        mv.add_picture(ctx)
        mv.add_rgb(other, ctx=ctx)
        mv.add_rgb(other)
    got = read_avi(tmp_path / "m.avi")
    assert (got["width"], got["height"], got["fps"]) == (64, 48, 8)
    assert got["frames"] == [frame_host(plot_rgb, (64, 48), 90), frame_host(other, (64, 48), 90), frame_host(other, (64, 48), 90)]


# ---- the drivers ------------------------------------------------------------------------------------------------------
T, DTS = 2, 60
FP = dict(maxCorners=300, qualityLevel=0.007, minDistance=8, blockSize=10)
LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))


def _files(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name), "rb") as f:
            out[name] = f.read()
    return out


def test_folder_driver_writes_the_movie(synth, tmp_path):
    """seven photos of 320 x 240 a minute apart: three segments of track_len 2, three pictures, three frames"""
    from iceberg_tracking_code_amd import movie_size, read_avi, track_image_sequence
    grays, _ = synth.sequence(320, 240, 7, seed=35, max_step_px=2.0)
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    (tmp_path / "photos").mkdir()
    names = []
    for k, g in enumerate(grays):
        name = str(tmp_path / "photos" / ((t0 + dt.timedelta(seconds=k * DTS)).strftime("%Y%m%d-%H%M%S") + ".jpg"))
        Image.fromarray(np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)).save(name, quality=92)
        names.append(name)

    def run(tag, **kw):
        dst = str(tmp_path / tag)
        os.makedirs(dst)
        out = track_image_sequence(names, dst, T, DTS, feature_params=FP, lk_params=LK, decode_threads=2, plots=str(tmp_path / (tag + "_plots")),
                                   plot_width=300, **kw)
        return out, _files(dst), _files(str(tmp_path / (tag + "_plots")))
    got, npz, plots = run("with", movie=True)
    want, npz_plain, plots_plain = run("without")
    avi = "tracks_oblique_%dsec.avi" % (T * DTS)
    assert sorted(plots) == sorted(list(plots_plain) + [avi]) and len(plots_plain) == 3
    assert {k: v for k, v in plots.items() if k != avi} == plots_plain                 # the pictures do not change
    assert npz == npz_plain and len(got) == len(want) == 3
    film = read_avi(str(tmp_path / "with_plots" / avi))
    assert film["fps"] == 8 and len(film["frames"]) == 3
    size = movie_size(300, 225)                                                        # the pictures are 300 x 225
    assert (film["width"], film["height"]) == size == (2000, 1504)
    for frame, picture in zip(film["frames"], [plots_plain[k] for k in sorted(plots_plain)]):
        im = Image.open(io.BytesIO(frame))
        assert im.format == "JPEG" and im.size == size
        assert Image.open(io.BytesIO(picture)).size == (300, 225)
    # a path of the caller's, and a writer of the caller's that stays open
    from iceberg_tracking_code_amd import MovieWriter
    mine = MovieWriter(tmp_path / "mine.avi", width=320)
    run("writer", movie=mine)
    assert mine.frames == 3 and not mine._closed
    mine.close()
    assert read_avi(tmp_path / "mine.avi")["width"] == 320
    assert "tracks_oblique_120sec.avi" not in os.listdir(str(tmp_path / "writer_plots"))


@pytest.fixture(scope="module")
def golden_day(tmp_path_factory):
    z = G.load()
    root = tmp_path_factory.mktemp("movie_day")
    G.build_tree(z, str(root / "in"))
    camnames, schedule, drifts, fjord, day, grid_size, thr = G.args(z)
    cameras = [dict(camera=c, start_day=20190701, end_day=20190831, easting=float(fjord["x"].min() + 300.0 + 700.0 * k),
                    northing=float(fjord["y"].min() + 150.0 + 500.0 * k)) for k, c in enumerate(camnames) if c != "camD"]
    return dict(root=root, args=(camnames, str(root / "in"), "utm", None, schedule, drifts, fjord), day=day, tail=(0.5, grid_size, thr),
                kw=dict(plot_switch=2, speedthreshold_cbar=0.3, cameras=cameras, out_width=240))


def _day(ctx, d, tag, **kw):
    from iceberg_tracking_code_amd import utm_to_gridded_utm
    target = d["root"] / tag
    target.mkdir()
    a = list(d["args"])
    a[3] = str(target)
    got = utm_to_gridded_utm(*a, d["day"], *d["tail"], ctx=ctx, plots=str(d["root"] / (tag + "_plots")), **d["kw"], **kw)
    return got, _files(str(target)), _files(str(d["root"] / (tag + "_plots")))


@pytest.mark.parametrize("plot_format", ["jpeg", "png"])
def test_day_driver_writes_the_movie(ctx, golden_day, plot_format):
    from iceberg_tracking_code_amd import movie_size, read_avi
    got, npz, plots = _day(ctx, golden_day, "with_" + plot_format, movie=True, plot_format=plot_format)
    want, npz_plain, plots_plain = _day(ctx, golden_day, "without_" + plot_format, plot_format=plot_format)
    avi = "velocities_utm_30min.avi"
    assert sorted(plots) == sorted(list(plots_plain) + [avi]) and len(plots_plain) == 10
    assert {k: v for k, v in plots.items() if k != avi} == plots_plain and npz == npz_plain
    film = read_avi(str(golden_day["root"] / ("with_%s_plots" % plot_format) / avi))
    w, h = Image.open(io.BytesIO(plots_plain[sorted(plots_plain)[0]])).size
    assert film["fps"] == 8 and len(film["frames"]) == 10 and (film["width"], film["height"]) == movie_size(w, h) and w == 240
    for frame in film["frames"]:
        im = Image.open(io.BytesIO(frame))
        assert im.format == "JPEG" and im.size == movie_size(w, h)
    if plot_format == "png":                                                           # the format changes nothing about the frames
        jpeg_film = golden_day["root"] / "with_jpeg_plots" / avi
        if jpeg_film.exists():
            assert read_avi(str(jpeg_film))["frames"] == film["frames"]


def test_days_driver_writes_one_movie(ctx, golden_day):
    from iceberg_tracking_code_amd import MovieWriter, read_avi, utm_to_gridded_utm_days
    d = golden_day
    target, plots = d["root"] / "days", d["root"] / "days_plots"
    target.mkdir()
    a = list(d["args"])
    a[3] = str(target)
    days = [d["day"], d["day"] + dt.timedelta(days=60), d["day"]]                      # the day, an unscheduled one, the day again
    mine = MovieWriter(d["root"] / "days.avi", width=320)
    got = utm_to_gridded_utm_days(days, *a, *d["tail"], ctx=ctx, plots=str(plots), movie=mine, **d["kw"])
    assert len(got) == 20 and mine.frames == 20 and not mine._closed
    mine.close()
    film = read_avi(str(d["root"] / "days.avi"))
    assert len(film["frames"]) == 20 and film["frames"][:10] == film["frames"][10:] and film["width"] == 320
    assert not [n for n in os.listdir(str(plots)) if n.endswith(".avi")]
    # True: one file with the reference's name, over all the days
    target2 = d["root"] / "days_true"
    target2.mkdir()
    a[3] = str(target2)
    utm_to_gridded_utm_days(days[:2], *a, *d["tail"], ctx=ctx, plots=str(d["root"] / "days_true_plots"), movie=True, **d["kw"])
    assert len(read_avi(str(d["root"] / "days_true_plots" / "velocities_utm_30min.avi"))["frames"]) == 10

"""GPU: the segment picture rasterised and coded on the device (csrc/k_plot.hip, abi_plot.hip) against the
numpy restatement and Pillow's writer -- every byte --, its determinism under contended atomics, its edge cases, the
segment forms on a live tracker and the folder driver's `plots=`."""
import ctypes as C
import datetime as dt
import io
import os

import numpy as np
import pytest
from PIL import Image

import plot_cases as pc
import plot_restatement as R

pytestmark = pytest.mark.gpu


def _pillow(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


@pytest.fixture(scope="module")
def wide():
    """a handle for the 4000 x 8 frame, which the session's 1024 x 768 handle does not take"""
    from iceberg_tracking_code_amd import Context
    c = Context(4000, 8, n_slots=1, max_pts=64)
    yield c
    c.close()


@pytest.mark.parametrize("vertices", pc.VERTICES)
@pytest.mark.parametrize("w,h,width", pc.SHAPES)
def test_plot_tracks_equals_restatement_and_pillow(ctx, wide, w, h, width, vertices):
    c = wide if w > 1024 else ctx
    gray, tracks, stamp, want = pc.case(w, h, width, vertices)
    c.upload_gray(0, gray)
    for q in (75, 90, 100):
        data, rgb = c.plot_tracks(0, tracks, width, stamp, q, want_rgb=True)
        assert np.array_equal(rgb, want), (q, np.argwhere((rgb != want).any(axis=2))[:5])
        assert data == _pillow(want, q), q
        assert Image.open(io.BytesIO(data)).size == R.size(w, h, width)
    assert c.plot_tracks(0, tracks, width, stamp, 90) == _pillow(want, 90)          # without the R G B
    assert np.array_equal(c.download_level(0, 0), gray)                             # the slot's frame is untouched


def test_determinism_under_contention(ctx):
    w, h, width, n = 256, 192, 96, 20000
    rng = np.random.default_rng(11)
    gray = pc.frame(w, h, seed=3)
    start = np.where(rng.random((n, 1)) < 0.5, rng.normal((128, 96), 6, (n, 2)), rng.uniform((-20, -20), (w + 20, h + 20), (n, 2)))
    tracks = (start[:, None, :] + np.cumsum(rng.normal(0, 9, (n, 3, 2)), axis=1)).astype(np.float32)
    want = R.overlay(gray, tracks, width, "11:11")
    lines, dots = R.counts(gray.shape, tracks, width)
    assert lines.max() > 200 and dots.max() > 200                                   # contended
    ctx.upload_gray(1, gray)
    a = ctx.plot_tracks(1, tracks, width, "11:11", 90, want_rgb=True)
    b = ctx.plot_tracks(1, tracks, width, "11:11", 90, want_rgb=True)
    assert np.array_equal(a[1], want)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[0] == _pillow(want, 90)


def test_edge_cases(ctx):
    from iceberg_tracking_code_amd import Context, _lib
    w, h, width = pc.SHAPES[0]
    gray, tracks, stamp, want = pc.case(w, h, width, 3)
    ctx.upload_gray(2, gray)
    wo, ho = R.size(w, h, width)
    # no tracks: the bare background
    data, rgb = ctx.plot_tracks(2, np.zeros((0, 2, 2), np.float32), width, "", 90, want_rgb=True)
    assert np.array_equal(rgb, np.repeat(R.background(gray, wo, ho)[..., None], 3, axis=2)) and data == _pillow(rgb, 90)
    # a short buffer: ICELK_ECAP with the size, nothing written; the repeated call succeeds
    whole = _pillow(want, 90)
    n = C.c_uint64(0)
    buf = np.full(len(whole) + 16, 0xAA, np.uint8)
    t = np.ascontiguousarray(tracks)

    def call(cap, quality=90, width=width, text=stamp.encode(), slot=2, handle=ctx):
        return handle._lib.icelk_plot_tracks(handle._h, slot, t.ctypes.data_as(_lib.f32p), len(t), t.shape[1], width, text, quality, None, 0,
                                             C.c_void_p(buf.ctypes.data), cap, C.byref(n))
    assert call(len(whole) - 1) == _lib.ECAP and n.value == len(whole) and (buf == 0xAA).all()
    assert call(0) == _lib.ECAP and n.value == len(whole)
    assert call(len(whole)) == _lib.OK and n.value == len(whole) and buf[:len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAA).all()
    # refused before anything is enqueued, nothing written
    buf[:] = 0xAA
    n.value = 77
    for kw in (dict(quality=0), dict(quality=101), dict(width=7), dict(text=b"12h30"), dict(text=b"1" * 49), dict(slot=3), dict(slot=-1)):
        assert call(buf.size, **kw) == _lib.EARG, kw
    assert n.value == 77 and (buf == 0xAA).all()
    with pytest.raises(ValueError):
        ctx.plot_tracks(2, tracks, width, stamp, 0)
    with pytest.raises(ValueError):
        ctx.plot_tracks(2, np.zeros((4, 18, 2), np.float32), width)
    # an empty slot
    with Context(64, 48, n_slots=2, max_pts=64) as fresh:
        assert call(buf.size, slot=0, handle=fresh) == _lib.ESTATE and (buf == 0xAA).all()
        with pytest.raises(_lib.IcelkError) as e:
            fresh.plot_tracks(0, tracks, width)
        assert e.value.code == _lib.ESTATE
        with pytest.raises(_lib.IcelkError):
            fresh.plot_tracks(0, tracks, width, want_rgb=True)


FP = dict(maxCorners=300, qualityLevel=0.007, minDistance=8, blockSize=10)
LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))


def test_seg_plot_on_a_live_tracker():
    from iceberg_tracking_code_amd import SegmentTracker, _lib
    trk = SegmentTracker(320, 240, 2, feature_params=FP, lk_params=LK)
    try:
        with pytest.raises(RuntimeError):
            trk.plot_closed()
        assert trk.push_synth(0, 0, seed=5) is None
        with pytest.raises(RuntimeError):
            trk.plot_closed()
        with pytest.raises(_lib.IcelkError) as e:                  # a current segment, but none closed yet
            trk.ctx.seg_plot(trk.cur, closed=True)
        assert e.value.code == _lib.ESTATE
        assert trk.push_synth(300, -200, seed=5) is None
        # the current segment before the switch: two vertices so far
        tracks, _ = trk.ctx.seg_read()
        assert tracks.shape[1] == 2 and len(tracks) > 50
        got = trk.ctx.seg_plot(trk.cur, False, 320, "10:00", 90, want_rgb=True)
        want = trk.ctx.plot_tracks(trk.cur, tracks, 320, "10:00", 90, want_rgb=True)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        assert np.array_equal(got[1], R.overlay(trk.ctx.download_level(trk.cur, 0), tracks, 320, "10:00"))
        # the push that returns the segment
        seg = trk.push_synth(600, -400, seed=5)
        assert seg is not None and seg[1].shape[1] == 3 and len(seg[1]) > 50
        for width in (320, 200):
            assert trk.plot_closed(width, "20190714-123005 120/60", 85) == trk.ctx.plot_tracks(trk.cur, seg[1], width, "20190714-123005 120/60", 85)
        assert trk.plot_closed() == trk.ctx.plot_tracks(trk.cur, seg[1])
        assert np.array_equal(trk.ctx.seg_read(closed=True)[0], seg[1])          # the closed segment is still what it was
        assert trk.push_synth(900, -600, seed=5) is None
        with pytest.raises(RuntimeError):
            trk.plot_closed()
    finally:
        trk.close()


# ---- the folder driver ------------------------------------------------------------------------------------------------
T, DTS = 2, 60
FOLDER_CROP = (3, 5, 6, 7)
POLY = [(20, 30), (300, 25), (310, 225), (150, 200), (15, 230)]
MODES = dict(pil=dict(decoder="pil"),
             pipeline=dict(decoder="device", huffman="device", pipeline=True),
             resave_crops=dict(resave="reference"))


@pytest.fixture(scope="module")
def folder(synth, tmp_path_factory):
    """nine photos of 320 x 240, a minute apart but for five minutes between the fifth and the sixth: of the four segments
    of track_len 2 the third breaks the time-gap rule"""
    d = tmp_path_factory.mktemp("plots")
    grays, _ = synth.sequence(320, 240, 9, seed=35, max_step_px=2.0)
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    os.makedirs(str(d / "photos"))
    names = []
    for k, g in enumerate(grays):
        rgb = np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)
        name = (t0 + dt.timedelta(seconds=k * DTS + (240 if k >= 5 else 0))).strftime("%Y%m%d-%H%M%S") + ".jpg"
        Image.fromarray(rgb).save(str(d / "photos" / name), quality=92)
        names.append(str(d / "photos" / name))
    return dict(dir=d, names=names)


def _track(names, dst, **kw):
    from iceberg_tracking_code_amd import track_image_sequence
    os.makedirs(dst, exist_ok=True)
    left, top = FOLDER_CROP[:2]
    return track_image_sequence(names, dst, T, DTS, crop=FOLDER_CROP, mask_polygon=(POLY, left, top), feature_params=FP, lk_params=LK,
                                decode_threads=2, **kw)


def _files(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
def test_folder_driver_writes_the_plots(ctx, folder, mode):
    d, names = folder["dir"], folder["names"]
    kw = dict(MODES[mode])
    kw_plain = dict(kw)
    plots = str(d / ("plots_" + mode))
    if mode == "resave_crops":
        kw["save_crops"], kw_plain["save_crops"] = str(d / "crops_with"), str(d / "crops_without")
    got = _track(names, str(d / ("with_" + mode)), plots=plots, plot_width=300, plot_quality=80, **kw)
    want = _track(names, str(d / ("without_" + mode)), **kw_plain)
    # tracks and .npz files do not change
    assert len(got) == len(want) == 3
    for (pg, tg, qg), (pw, tw, qw) in zip(got, want):
        assert os.path.basename(pg) == os.path.basename(pw) and len(tw) > 10
        assert np.array_equal(tg, tw) and np.array_equal(qg, qw)
        zg, zw = np.load(pg, allow_pickle=False), np.load(pw, allow_pickle=False)
        assert sorted(zg.files) == sorted(zw.files)
        for key in zg.files:
            assert np.array_equal(zg[key], zw[key]), key
    if mode == "resave_crops":
        a, b = _files(kw["save_crops"]), _files(kw_plain["save_crops"])
        assert len(a) == 9 and a == b                    # the plot's working set is its own
    # one file per saved segment, named after the segment's last photo; none for the segment with the gap
    last = [names[2], names[4], names[8]]
    bases = [os.path.splitext(os.path.basename(p))[0] for p in last]
    assert sorted(os.listdir(plots)) == sorted("%s_%dsec.jpg" % (b, T * DTS) for b in bases)
    pictures = _files(plots)
    for path, base, (_, tracks, _) in zip(last, bases, got):
        ctx.upload_bgr(0, np.array(Image.open(path)), 4, FOLDER_CROP, kw.get("resave"))
        mine = ctx.plot_tracks(0, tracks, 300, "%s %d/%d" % (base, T * DTS, DTS), 80)
        assert pictures["%s_%dsec.jpg" % (base, T * DTS)] == mine, base
        im = Image.open(io.BytesIO(mine))
        assert im.size == (300, R.size(311, 228, 300)[1])


def test_folder_driver_default_runs_nothing_new(folder, monkeypatch):
    from iceberg_tracking_code_amd import Context
    called = []
    monkeypatch.setattr(Context, "seg_plot", lambda self, *a, **k: called.append(a))
    monkeypatch.setattr(Context, "plot_tracks", lambda self, *a, **k: called.append(a))
    out = str(folder["dir"] / "default")
    got = _track(folder["names"], out)
    assert len(got) == 3 and not called
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p, _, _ in got)     # the .npz files and nothing else

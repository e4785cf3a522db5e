"""GPU: the stabilising stage (csrc/k_stab.hip) against the host statement of its rules (icelk_stab_tracks_host), bit for bit:
the catalogue of stab_cases.py through `stabilize_tracks`, and segments tracked on the device through `Context.seg_stabilize`,
a stabilising `SegmentTracker` and `track_image_sequence`, against the statement run on the oracle loop's segments."""
import datetime as dt
import os

import numpy as np
import pytest

import stab_cases as K
from test_stab_host import assert_same, bits

pytestmark = pytest.mark.gpu

W, H, T = 320, 240, 2
CAMERA = ((0, 0), (296, -168), (-832, 640), (80, 112), (0, 768))          # 1/256 px
ICE = (-300, 100)                                                          # 1/256 px per frame
FP = dict(maxCorners=100000, qualityLevel=0.01, minDistance=6, blockSize=5)
LK = dict(winSize=(21, 21), maxLevel=2, criteria=(3, 20, 0.03))


@pytest.mark.parametrize("name", K.names())
def test_device_equals_the_host_statement(name, ctx):
    from iceberg_tracking_code_amd import stabilize_tracks, stabilize_tracks_host
    _, t, flags, params, _ = K.case(name)
    got = stabilize_tracks(ctx, t, flags, **params)
    assert_same(got, stabilize_tracks_host(t, flags, **params), name)
    assert np.array_equal(got["anchors"], flags)


def test_device_refusals(ctx):
    from iceberg_tracking_code_amd import stabilize_tracks
    t, f = np.zeros((4, 3, 2), np.float32), np.ones(4, bool)
    for bad in (dict(threshold=0.0), dict(rounds=17), dict(min_anchors=1), dict(min_spread=-1.0), dict(start_gate=float("nan"))):
        with pytest.raises(ValueError):
            stabilize_tracks(ctx, t, f, **bad)
    r = stabilize_tracks(ctx, np.zeros((0, 2, 2), np.float32), np.zeros(0, bool))
    assert r["tracks"].shape == (0, 2, 2) and r["status"].tolist() == [1] and r["n_anchors"] == 0


@pytest.fixture(scope="module")
def frames(synth):
    left = np.arange(W)[None, :] < 112
    return [np.ascontiguousarray(np.where(left, synth.frame(W, H, cx, cy, seed=11), synth.frame(W, H, cx + ICE[0] * t, cy + ICE[1] * t, seed=29)))
            for t, (cx, cy) in enumerate(CAMERA)]


@pytest.fixture(scope="module")
def anchor_mask():
    return np.where(np.arange(W)[None, :] < 100, 255, 0).astype(np.uint8).repeat(H, axis=0)


def expected_segments(orc, frames, anchor_mask, track_len):
    """The host statement on the segments of the reference-shaped loop run on the oracle: (first, dict, quality, raw tracks)"""
    from iceberg_tracking_code_amd import anchor_flags, stabilize_tracks_host
    from reference_loops import OracleCv, run_reference_loop
    out = []
    for first, tracks, quality in run_reference_loop(frames, track_len, FP, LK, cv=OracleCv(orc)):
        raw = np.asarray(tracks, np.float32).reshape(len(tracks), -1, 2)
        out.append((first, stabilize_tracks_host(raw, anchor_flags(raw, anchor_mask)), np.asarray(quality, np.float32).reshape(len(raw), -1), raw))
    return out


@pytest.fixture(scope="module")
def want(orc, frames, anchor_mask):
    segs = expected_segments(orc, frames, anchor_mask, T)
    assert len(segs) == 2
    for _, r, _, raw in segs:
        # what keeps the test honest: the anchors carry a model at every vertex
        assert len(raw) > 500 and r["n_anchors"] > 250 and (r["status"] == 0).all() and (r["inliers"] >= 250).all()
        assert np.abs(r["motion"][:, 2:]).max() > 0.25 and not np.array_equal(r["tracks"], raw)
    return segs


@pytest.fixture()
def seg_ctx(frames):
    from iceberg_tracking_code_amd import Context
    c = Context(W, H, n_slots=len(frames), max_pts=1 << 14)
    for i, f in enumerate(frames):
        c.upload_gray(i, f)
    yield c
    c.close()


def assert_segment(got, first, quality, want_seg):
    w_first, w, w_quality, _ = want_seg
    assert first == w_first
    assert_same(got, w, first)
    assert np.array_equal(got["anchors"], w["anchors"]) and np.array_equal(bits(quality), bits(w_quality))


def test_seg_stabilize_after_plain_pushes(seg_ctx, frames, anchor_mask, want):
    from iceberg_tracking_code_amd import SegmentTracker
    trk = SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx)
    seg_ctx.stab_set_anchor_mask(anchor_mask)
    got = []
    trk.on_close = lambda first, closed: got.append((first, closed, seg_ctx.seg_stabilize(closed=closed)))
    plain = [s for s in (trk.push_slot(i, True) for i in range(len(frames))) if s is not None]
    assert [c for _, c, _ in got] == [False, False] and len(plain) == 2
    for (first, _, r), w, (p_first, p_tracks, p_quality) in zip(got, want, plain):
        assert_segment(r, first, r["trackquality"], w)
        # the push itself read the raw table: the stage changes nothing it is not asked for
        assert p_first == first and np.array_equal(bits(p_tracks), bits(w[3])) and np.array_equal(bits(p_quality), bits(w[2]))
    seg_ctx.stab_set_anchor_mask(None)


def test_stabilising_tracker_returns_corrected_segments(seg_ctx, frames, anchor_mask, want):
    from iceberg_tracking_code_amd import SegmentTracker
    trk = SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, anchor_mask=anchor_mask, stabilize=True)
    n = 0
    for i in range(len(frames)):
        seg = trk.push_slot(i, True)
        if seg is None:
            continue
        first, tracks, quality = seg
        assert_segment(dict(trk.last_stabilization, tracks=tracks), first, quality, want[n])
        n += 1
    assert n == 2


def test_seg_stabilize_closed_after_a_joint_launch(seg_ctx, frames, anchor_mask, want):
    from iceberg_tracking_code_amd import SegmentTracker
    trk = SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx)
    seg_ctx.stab_set_anchor_mask(anchor_mask)
    got = []
    trk.on_close = lambda first, closed: got.append((first, closed, seg_ctx.seg_stabilize(closed=closed, model="translation")))
    for i in range(len(frames)):
        assert trk.push_slot(i, False, *[i + k if i + k < len(frames) else None for k in range(1, 7)]) is None
    trk.flush()
    assert [c for _, c, _ in got] == [True, False] and trk.pairs_launched == 4
    for (first, _, r), w in zip(got, want):
        assert_segment(r, first, r["trackquality"], w)


def test_track_len_three(orc, seg_ctx, frames, anchor_mask):
    from iceberg_tracking_code_amd import SegmentTracker
    (w,) = expected_segments(orc, frames, anchor_mask, 3)
    assert w[3].shape[1] == 4 and (w[1]["status"] == 0).all() and (w[1]["inliers"] >= 250).all()
    trk = SegmentTracker(W, H, 3, FP, LK, ctx=seg_ctx, anchor_mask=anchor_mask, stabilize=dict(model="similarity", min_spread=16.0))
    segs = [s for s in (trk.push_slot(i, True) for i in range(len(frames))) if s is not None]
    assert len(segs) == 1
    from iceberg_tracking_code_amd import stabilize_tracks_host
    sim = stabilize_tracks_host(w[3], w[1]["anchors"], model="similarity", min_spread=16.0)
    assert (sim["status"] == 0).all()
    assert_segment(dict(trk.last_stabilization, tracks=segs[0][1]), segs[0][0], segs[0][2], (w[0], sim, w[2], w[3]))


def test_refusals(seg_ctx, frames, anchor_mask):
    from iceberg_tracking_code_amd import IcelkError, SegmentTracker
    trk = SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx)
    for i in range(4):
        trk.push_slot(i, False)
    with pytest.raises(IcelkError, match="icelk error -5"):
        seg_ctx.seg_stabilize()
    seg_ctx.stab_set_anchor_mask(anchor_mask)
    with pytest.raises(ValueError):
        seg_ctx.seg_stabilize(rounds=0)
    assert seg_ctx.seg_stabilize()["tracks"].shape[1] == 2      # the segment of frame 2 and its one pair so far
    seg_ctx.stab_set_anchor_mask(None)
    with pytest.raises(IcelkError, match="icelk error -5"):
        seg_ctx.seg_stabilize()
    # a mask of another size than the frame
    for bad in (anchor_mask[:, :-1], anchor_mask[:-1], anchor_mask.T):
        with pytest.raises(ValueError):
            SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, anchor_mask=bad, stabilize=True)
    with pytest.raises(ValueError):
        seg_ctx.stab_set_anchor_mask(np.ones((H + 1, W), np.uint8))     # larger than the handle's frames
    with pytest.raises(ValueError):
        SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, stabilize=True)
    with pytest.raises(ValueError):
        SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, anchor_mask=anchor_mask)
    with pytest.raises((ValueError, TypeError)):
        SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, anchor_mask=anchor_mask, stabilize=dict(model="affine"))


def test_detector_mask_is_joined_with_the_anchor_mask(seg_ctx, anchor_mask):
    from iceberg_tracking_code_amd import SegmentTracker
    water = np.where(np.arange(W)[None, :] >= 160, 255, 0).astype(np.uint8).repeat(H, axis=0)
    SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, mask=water, anchor_mask=anchor_mask, stabilize=True)
    joined = seg_ctx.download_mask()
    assert np.array_equal(joined != 0, (water != 0) | (anchor_mask != 0))
    poly = [(160, 0), (W, 0), (W, H), (160, H)]
    SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, mask_polygon=(poly, 0, 0))
    alone = seg_ctx.download_mask()
    SegmentTracker(W, H, T, FP, LK, ctx=seg_ctx, mask_polygon=(poly, 0, 0), anchor_mask=anchor_mask, stabilize=True)
    assert np.array_equal(seg_ctx.download_mask() != 0, (alone != 0) | (anchor_mask != 0)) and (alone != 0).sum() > 1000
    seg_ctx.stab_set_anchor_mask(None)


def test_track_image_sequence(frames, anchor_mask, tmp_path):
    from PIL import Image
    from iceberg_tracking_code_amd import anchor_flags, stabilize_tracks_host, track_image_sequence
    src = tmp_path / "photos"
    src.mkdir()
    names = []
    for k, g in enumerate(frames):
        p = src / ((dt.datetime(2019, 7, 24, 10, 0, 0) + dt.timedelta(seconds=60 * k)).strftime("%Y%m%d-%H%M%S") + ".jpg")
        Image.fromarray(np.stack([g, g, g], 2)).save(p, quality=95)
        names.append(str(p))

    def same_arrays(a, b):
        """two .npz files hold the same arrays bit for bit (their zip containers carry the time they were written)"""
        za, zb = np.load(a, allow_pickle=False), np.load(b, allow_pickle=False)
        return za.files == zb.files and all(za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes()
                                            for k in za.files)

    def run(sub, **kw):
        d = tmp_path / sub
        d.mkdir()
        return d, track_image_sequence(names, str(d), T, 60, feature_params=FP, lk_params=LK, decode_threads=2, **kw)

    d_plain, plain = run("plain")
    d_off, _ = run("off", anchor_mask=None, stabilize=None)
    d_stab, stab = run("stab", anchor_mask=anchor_mask, stabilize=True)
    d_pipe, _ = run("pipe", anchor_mask=anchor_mask, stabilize=True, decoder="device", huffman="device", pipeline=True)
    d_plots, _ = run("plots", anchor_mask=anchor_mask, stabilize=dict(rounds=8), plots=str(tmp_path / "pictures"))
    files = sorted(os.listdir(d_plain))
    assert len(files) == 2 and all(sorted(os.listdir(d)) == files for d in (d_off, d_stab, d_pipe, d_plots))
    assert len(os.listdir(tmp_path / "pictures")) == 2
    for f, (_, raw, raw_q), (path, tracks, quality) in zip(files, plain, stab):
        # with the option off the files are what they were
        assert same_arrays(d_plain / f, d_off / f)
        assert sorted(np.load(d_plain / f).files) == ["trackquality", "tracks"]
        z = np.load(d_stab / f, allow_pickle=False)
        assert sorted(z.files) == sorted(["tracks", "trackquality", "anchor_tracks", "anchor_trackquality", "camera_motion", "camera_inliers",
                                          "camera_rms", "camera_status"])
        flags = anchor_flags(raw, anchor_mask)
        w = stabilize_tracks_host(raw, flags)
        assert flags.sum() > 200 and (w["status"] == 0).all() and (w["inliers"] >= 200).all()
        # no anchor rows in `tracks`; `tracks` plus `anchor_tracks` is the stabilised table
        assert np.array_equal(bits(z["tracks"]), bits(w["tracks"][~flags])) and np.array_equal(bits(z["anchor_tracks"]), bits(w["tracks"][flags]))
        assert np.array_equal(bits(z["trackquality"]), bits(raw_q[~flags])) and np.array_equal(bits(z["anchor_trackquality"]), bits(raw_q[flags]))
        assert not anchor_flags(z["tracks"], anchor_mask).any() and anchor_flags(z["anchor_tracks"], anchor_mask).all()
        assert np.array_equal(bits(z["camera_motion"]), bits(w["motion"])) and np.array_equal(z["camera_inliers"], w["inliers"])
        assert np.array_equal(bits(z["camera_rms"]), bits(w["rms"])) and np.array_equal(z["camera_status"], w["status"])
        assert os.path.basename(path) == f and np.array_equal(bits(tracks), bits(z["tracks"])) and np.array_equal(bits(quality), bits(z["trackquality"]))
        # the same files from the pipelined driver and beside the pictures
        for d in (d_pipe, d_plots):
            assert same_arrays(d / f, d_stab / f), d

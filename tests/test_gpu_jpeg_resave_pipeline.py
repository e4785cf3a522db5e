"""GPU: the re-save ahead of the frame in the tracker and in the folder driver -- `SegmentTracker.prefetch_jpeg(resave=)`
against `push_jpeg(resave=)`, and `track_image_sequence(pipeline=True, resave_ahead=True, resave=, save_crops=)` against the
same options without the pipeline, against Pillow's crop folder and against the two-pass route.  8 photos of 320 x 240, crop
(3, 5, 6, 7), one photo progressive (it goes through PIL) and two with comments.  Every comparison is equality."""
import datetime as dt
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_resave_cases as rc

pytestmark = pytest.mark.gpu

T, DTS = 2, 60
FOLDER_CROP = (3, 5, 6, 7)
POLY = [(20, 30), (300, 25), (310, 225), (150, 200), (15, 230)]
FP = dict(maxCorners=300, qualityLevel=0.007, minDistance=8, blockSize=10)
LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
DEVICE = dict(decoder="device", huffman="device")


def _track(names, dst, **kw):
    from iceberg_tracking_code_amd import track_image_sequence
    os.makedirs(dst, exist_ok=True)
    left, top = FOLDER_CROP[:2]
    return track_image_sequence(names, dst, T, DTS, mask_polygon=(POLY, left, top), feature_params=FP, lk_params=LK, decode_threads=2, **kw)


@pytest.fixture(scope="module")
def folder(synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("resave_pipeline")
    grays, _ = synth.sequence(320, 240, 8, seed=33, max_step_px=2.0)
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    os.makedirs(str(d / "photos"))
    os.makedirs(str(d / "cropped"))
    names, cropped = [], {}
    for k, g in enumerate(grays):
        rgb = np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)
        name = (t0 + dt.timedelta(seconds=k * DTS)).strftime("%Y%m%d-%H%M%S") + ".jpg"
        kw = dict(comment=b"photo %d" % k) if k in (1, 3) else {}
        Image.fromarray(rgb).save(str(d / "photos" / name), quality=92, progressive=(k == 3), **kw)
        rc.reference_crop_resave(str(d / "photos" / name), str(d / "cropped" / name), FOLDER_CROP)
        names.append(str(d / "photos" / name))
        with open(str(d / "cropped" / name), "rb") as f:
            cropped[name] = f.read()
    return dict(dir=d, names=names, cropped=cropped)


def _same(got, want):
    assert len(got) == len(want) >= 3
    for (pg, tg, qg), (pw, tw, qw) in zip(got, want):
        assert os.path.basename(pg) == os.path.basename(pw) and len(tw) > 10
        assert tg.shape == tw.shape and np.array_equal(tg, tw) and np.array_equal(qg, qw)
        zg, zw = np.load(pg, allow_pickle=False), np.load(pw, allow_pickle=False)
        assert np.array_equal(zg["tracks"], zw["tracks"]) and np.array_equal(zg["trackquality"], zw["trackquality"])


def test_p1_tracker_fed_by_prefetch_jpeg_with_resave(folder, tmp_path):
    from iceberg_tracking_code_amd.tracker import SegmentTracker
    from iceberg_tracking_code_amd.jpeg import source_comment
    left, top, right, bottom = FOLDER_CROP
    w, h = 320 - left - right, 240 - top - bottom
    files = []
    for p in folder["names"]:
        with open(p, "rb") as f:
            files.append(f.read())
    usable = [k for k in range(len(files)) if k != 3]              # the progressive one is not the device decoder's
    out_dir = tmp_path / "crops"
    os.makedirs(str(out_dir))

    def run(prefetch):
        trk = SegmentTracker(w, h, T, feature_params=FP, lk_params=LK, mask_polygon=(POLY, left, top), n_slots=6)
        segs = []
        try:
            if not prefetch:
                for k in usable:
                    segs.append(trk.push_jpeg(files[k], crop=FOLDER_CROP, resave="reference"))
            else:
                fed = 0
                for n in range(len(usable)):
                    while fed < len(usable) and fed - n < trk.n_slots - 2:
                        k = usable[fed]
                        name = os.path.basename(folder["names"][k])
                        trk.prefetch_jpeg(files[k], crop=FOLDER_CROP, resave="reference",
                                          crop_file=str(out_dir / name) if fed % 2 == 1 else None, comment=source_comment(files[k]))
                        fed += 1
                    segs.append(trk.push_prefetched())
        finally:
            trk.close()
        return segs

    want, got = run(False), run(True)
    assert sum(s is not None for s in want) >= 2
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    written = sorted(os.listdir(str(out_dir)))
    assert written == sorted(os.path.basename(folder["names"][k]) for k in usable[1::2])
    for name in written:
        with open(str(out_dir / name), "rb") as f:
            assert f.read() == folder["cropped"][name], name


def test_p2_driver_one_pass(folder, monkeypatch):
    from iceberg_tracking_code_amd import crop_image_sequence
    from iceberg_tracking_code_amd.tracker import SegmentTracker
    d = folder["dir"]
    crops = str(d / "crops_one_pass")
    writes = []
    original = SegmentTracker._write_crop

    def counting(crop_file, data):
        if crop_file is not None:
            writes.append(os.path.basename(crop_file))
        original(crop_file, data)
    monkeypatch.setattr(SegmentTracker, "_write_crop", staticmethod(counting))
    got = _track(folder["names"], str(d / "out_one_pass"), crop=FOLDER_CROP, pipeline=True, resave_ahead=True, resave="reference",
                 save_crops=crops, startlist=(0, 1), **DEVICE)
    assert sorted(writes) == sorted(folder["cropped"]), "every file is written once"
    assert sorted(os.listdir(crops)) == sorted(folder["cropped"])
    for name, want in folder["cropped"].items():
        with open(os.path.join(crops, name), "rb") as f:
            assert f.read() == want, name
    monkeypatch.undo()
    serial = _track(folder["names"], str(d / "out_serial"), crop=FOLDER_CROP, pipeline=False, resave="reference",
                    save_crops=str(d / "crops_serial"), startlist=(0, 1), **DEVICE)
    _same(got, serial)
    plain = _track(folder["names"], str(d / "out_plain"), crop=FOLDER_CROP, pipeline=True, startlist=(0, 1), **DEVICE)
    assert len(plain) == len(got)
    assert any(tg.shape != tp.shape or not np.array_equal(tg, tp) for (_, tg, _), (_, tp, _) in zip(got, plain)), \
        "the re-save changed no vertex: the option would not matter"
    # the two-pass route: the crop pass writes the folder, a pipelined run reads it back
    target = str(d / "two_pass_crops")
    done = crop_image_sequence(folder["names"], target, crop=FOLDER_CROP, in_flight=3)
    two_pass = _track([p for p, _, _ in done], str(d / "out_two_pass"), pipeline=True, startlist=(0, 1), **DEVICE)
    _same(got, two_pass)
    # without save_crops: the same tracks, nothing written
    bare = _track(folder["names"], str(d / "out_bare"), crop=FOLDER_CROP, pipeline=True, resave_ahead=True, resave=75, startlist=(0, 1), **DEVICE)
    _same(bare, got)


def _files(folder):
    out = []
    for p in folder["names"]:
        with open(p, "rb") as f:
            out.append(f.read())
    return out


def test_p3_failed_file_is_replaced_and_abort_drops_jobs(folder, tmp_path):
    """Frame 1 arrives cut in its scan: the file's index takes it, so the job starts and the error comes out of
    `push_prefetched`; `replace_prefetched_bgr(resave=, crop_file=, comment=)` fills the slot and writes the crop's file.
    Then `abort()` with three re-save jobs in flight, two of them with a file wanted: it returns the frames consumed, writes
    no file for the dropped frames, leaves their slots free for new jobs, and pushing continues.  What continuing must give:
    `abort` abandons only work begun ahead, the next detection frame starts its detection when it arrives, and the
    tracker's results are those of the serial order in every case (`SegmentTracker._step`) -- so the segments of the serial
    `push_jpeg(resave=)` run over the same frames."""
    import io
    from iceberg_tracking_code_amd.jpeg import source_comment
    from iceberg_tracking_code_amd.tracker import SegmentTracker
    left, top, right, bottom = FOLDER_CROP
    w, h = 320 - left - right, 240 - top - bottom
    files = _files(folder)
    usable = [k for k in range(len(files)) if k != 3]              # 7 frames; the progressive one is not the device decoder's
    names = [os.path.basename(folder["names"][k]) for k in usable]
    out_dir = tmp_path / "crops"
    os.makedirs(str(out_dir))
    make = lambda: SegmentTracker(w, h, T, feature_params=FP, lk_params=LK, mask_polygon=(POLY, left, top), n_slots=6)
    trk = make()
    try:
        want = [s for s in (trk.push_jpeg(files[k], crop=FOLDER_CROP, resave="reference") for k in usable) if s is not None]
    finally:
        trk.close()
    assert len(want) == 3
    trk = make()
    try:
        got, replaced = [], []
        for n in range(4):
            k = usable[n]
            kw = dict(crop=FOLDER_CROP, resave="reference", crop_file=str(out_dir / names[n]), comment=source_comment(files[k]))
            trk.prefetch_jpeg(files[k][:len(files[k]) // 2] if n == 1 else files[k], **kw)
            try:
                seg = trk.push_prefetched()
            except ValueError:
                replaced.append(n)
                assert not os.path.exists(kw["crop_file"])
                trk.replace_prefetched_bgr(np.array(Image.open(io.BytesIO(files[k]))), **kw)
                seg = trk.push_prefetched()
            if seg is not None:
                got.append(seg)
        assert replaced == [1]
        for n in range(4):
            with open(str(out_dir / names[n]), "rb") as f:
                assert f.read() == folder["cropped"][names[n]], names[n]
        for n in (4, 5, 6):
            trk.prefetch_jpeg(files[usable[n]], crop=FOLDER_CROP, resave="reference",
                              crop_file=None if n == 5 else str(out_dir / names[n]), comment=None)
        assert trk.abort() == 4
        assert sorted(os.listdir(str(out_dir))) == sorted(names[:4])
        # the slots are nobody's any more: each takes a new job, whose file is right
        for n, s in zip((4, 5, 6), list(trk.prefetched)):
            trk.ctx.upload_jpeg_file_async(s, files[usable[n]], 4, FOLDER_CROP, resave="reference", crop_file=True)
            assert trk.ctx.jpeg_async_finish_file(s, None)[0] == folder["cropped"][names[n]], names[n]
        for n in (4, 5, 6):                                         # their frames are in the slots: pushing continues
            seg = trk.push_prefetched()
            if seg is not None:
                got.append(seg)
        assert sorted(os.listdir(str(out_dir))) == sorted(names[:4])    # the dropped frames' files are never written
    finally:
        trk.close()
    assert [g[0] for g in got] == [s[0] for s in want]
    for a, b in zip(got, want):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_p4_driver_replaces_a_file_that_fails_at_finish(folder, monkeypatch):
    """one photo's bytes reach the driver cut in the scan (the pool's read is patched; the file on disk is whole, so PIL
    has the word afterwards): the job starts, fails at `push_prefetched`, and the driver's `replace_prefetched_bgr` gets
    the options the photo was handed with -- same tracks, same crop folder"""
    from iceberg_tracking_code_amd import sequence
    from iceberg_tracking_code_amd.tracker import SegmentTracker
    d = folder["dir"]
    bad = folder["names"][5]
    real_load = sequence._load

    def load(path, kind, with_comment):
        got = real_load(path, kind, with_comment)
        if path != bad or kind != "bytes":
            return got
        data, comment = got if with_comment else (got, None)
        assert isinstance(data, bytes)
        data = data[:len(data) // 2]
        return (data, comment) if with_comment else data
    calls = []
    real_replace = SegmentTracker.replace_prefetched_bgr

    def replace(self, frame, **kw):
        calls.append(kw)
        return real_replace(self, frame, **kw)
    monkeypatch.setattr(sequence, "_load", load)
    monkeypatch.setattr(SegmentTracker, "replace_prefetched_bgr", replace)
    crops = str(d / "crops_damaged")
    got = _track(folder["names"], str(d / "out_damaged"), crop=FOLDER_CROP, pipeline=True, resave_ahead=True, resave="reference",
                 save_crops=crops, **DEVICE)
    monkeypatch.undo()
    assert len(calls) == 1, calls
    assert calls[0]["resave"] == 75 and calls[0]["crop"] == FOLDER_CROP and calls[0]["crop_file"] == os.path.join(crops, os.path.basename(bad))
    assert sorted(os.listdir(crops)) == sorted(folder["cropped"])
    for name, want in folder["cropped"].items():
        with open(os.path.join(crops, name), "rb") as f:
            assert f.read() == want, name
    whole = _track(folder["names"], str(d / "out_whole"), crop=FOLDER_CROP, pipeline=True, resave_ahead=True, resave="reference", **DEVICE)
    _same(got, whole)

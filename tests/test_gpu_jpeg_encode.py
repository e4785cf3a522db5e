"""GPU: the JPEG writer's entropy coder on the device (csrc/k_jpeg_enc.hip) against the host statement and Pillow's files --
images at the sizes where the kernels change path, hand-made coefficients at the coder's edges, the file of the three
re-saved uploads, the folder driver's `save_crops` -- and its determinism.  Every comparison is equality of bytes."""
import ctypes as C
import datetime as dt
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_cases as ec
import jpeg_resave_cases as rc

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/icelk_internal.h): count and pack take kJpegEncGroup = 64 blocks per workgroup, the prefix sum
# kJpegEncScanPass = 1024 groups per pass of its loop, so 65536 blocks; a 4:2:0 MCU has 6 blocks.
#   3 x 3         1 MCU
#   200 x 9       a single row of 13 MCUs, 78 blocks: the second workgroup holds 14
#   176 x 16      11 MCUs = 66 blocks: the first MCU whose blocks (60 .. 65) straddle the 64 of a workgroup; 65 is not a
#                 multiple of 6, 66 is the least block count above 64
#   528 x 5296    33 x 331 = 10923 MCUs = 65538 blocks = 1025 groups: the least count above a single pass of the scan
#   640 x 480     1200 MCUs
SIZES = ((3, 3), (200, 9), (176, 16), (528, 5296), (640, 480))
CONTENTS = (("noise", 100), ("noise", 1), ("zeros", 100), ("stripes", 95), ("smooth", 75))


def _first_difference(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d" % (len(a), len(b), k)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_d1_resave_bytes_equal_host_and_pillow(ctx, size):
    from iceberg_tracking_code_amd import resave_bytes, resave_coefficients
    w, h = size
    i = resave_coefficients(np.zeros((h, w, 3), np.uint8)).info
    blocks = 6 * i.mcus_x * i.mcus_y
    assert blocks == {(3, 3): 6, (200, 9): 78, (176, 16): 66, (528, 5296): 65538, (640, 480): 7200}[size]
    for kind, quality in CONTENTS:
        rgb = rc.content(kind, w, h, seed=7)
        got = resave_bytes(rgb, quality, ctx=ctx)
        host = resave_bytes(rgb, quality)
        assert got == host, (size, kind, quality, _first_difference(got, host))
        assert got == rc.pillow_save(rgb, quality), (size, kind, quality)


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_d2_hand_made_coefficients(ctx, name):
    from iceberg_tracking_code_amd import encode_jpeg
    j = ec.CASES[name]()
    got, host = encode_jpeg(j, ctx=ctx), encode_jpeg(j)
    assert got == host, _first_difference(got, host)
    assert ec.segments(got)[1] == ec.segments(ec.writer_file(j))[1]
    assert encode_jpeg(j, comment=b"a comment", ctx=ctx) == encode_jpeg(j, comment=b"a comment")


def test_d2_errors_and_other_layouts(ctx):
    from iceberg_tracking_code_amd import _lib, encode_jpeg, read_jpeg
    for make in (ec.ac_without_code, ec.dc_without_code, ec.with_restarts):
        with pytest.raises(ValueError) as host:
            encode_jpeg(make())
        with pytest.raises(ValueError) as dev:
            encode_jpeg(make(), ctx=ctx)
        assert dev.value.code == host.value.code and type(dev.value) is type(host.value)
    # a coefficient without a code: nothing is written; a short buffer: ICELK_ECAP and the length
    n = C.c_uint64(0)
    buf = np.full(1 << 16, 0xAA, np.uint8)
    bad, good = ec.ac_without_code(), ec.dc_staircase()
    call = lambda j, cap: ctx._lib.icelk_jpeg_encode_coefficients(ctx._h, C.byref(j.info), j.coef_ptr, None, 0, C.c_void_p(buf.ctypes.data), cap,
                                                                  C.byref(n))
    assert call(bad, buf.size) == _lib.EARG and (buf == 0xAA).all()
    whole = encode_jpeg(good)
    assert call(good, len(whole) - 1) == _lib.ECAP and n.value == len(whole) and (buf == 0xAA).all()
    assert call(good, len(whole)) == _lib.OK and buf[:len(whole)].tobytes() == whole
    # the layouts the re-save never makes: 4:4:4, 4:2:2 and gray files of Pillow's, coded again on the device
    for mode, subsampling in (("RGB", 0), ("RGB", 1), ("RGB", 2), ("L", None)):
        kw = {} if subsampling is None else {"subsampling": subsampling}
        f = ec.pillow_file(mode, (99, 131), quality=85, **kw)
        got = encode_jpeg(read_jpeg(f), ctx=ctx)
        assert got == f, (mode, subsampling, _first_difference(got, f))


@pytest.fixture(scope="module")
def photo(tmp_path_factory):
    """a photo file with a comment, its decoded pixels, and the file of the reference's re-saved crop (camtools.py:64-104)"""
    d = tmp_path_factory.mktemp("encode")
    src, dst = str(d / "20190801-120000.jpg"), str(d / "cropped.jpg")
    Image.fromarray(rc.content("smooth", *rc.PHOTO_SIZE, seed=3)).save(src, "JPEG", quality=90, subsampling=2, comment=b"camera 7")
    rc.reference_crop_resave(src, dst, rc.CROP)
    with open(src, "rb") as f:
        data = f.read()
    with open(dst, "rb") as f:
        cropped = f.read()
    return dict(data=data, pixels=np.array(Image.open(src)), file=cropped)


def test_d3_file_of_the_three_uploads(ctx, photo):
    from iceberg_tracking_code_amd import Context, _lib, read_jpeg, source_comment
    comment = source_comment(photo["data"])
    assert comment == b"camera 7"
    uploads = (lambda s: ctx.upload_bgr(s, photo["pixels"], 4, rc.CROP, resave="reference"),
               lambda s: ctx.upload_jpeg(s, read_jpeg(photo["data"]), 4, rc.CROP, resave="reference"),
               lambda s: ctx.upload_jpeg_file(s, photo["data"], 4, rc.CROP, resave="reference"))
    for k, upload in enumerate(uploads):
        upload(k)
        gray = ctx.download_level(k, 0)
        got = ctx.jpeg_resave_file(comment)
        assert got == photo["file"], (k, _first_difference(got, photo["file"]))
        assert ctx.jpeg_resave_file(comment) == got                  # twice: the same bytes
        assert np.array_equal(ctx.download_level(k, 0), gray)        # the slot's frame is untouched
        assert ctx.jpeg_resave_file() == got[:20] + got[20 + 4 + len(comment):]   # no comment: no COM segment
    # a buffer too small: ICELK_ECAP with the length, and the call can be repeated
    n = C.c_uint64(0)
    buf = np.zeros(len(photo["file"]), np.uint8)
    call = lambda cap: ctx._lib.icelk_jpeg_resave_encode(ctx._h, comment, len(comment), C.c_void_p(buf.ctypes.data), cap, C.byref(n))
    assert call(100) == _lib.ECAP and n.value == len(photo["file"])
    assert call(buf.size) == _lib.OK and buf.tobytes() == photo["file"]
    with Context(64, 64, n_slots=2, max_pts=64) as fresh:
        assert fresh._lib.icelk_jpeg_resave_encode(fresh._h, None, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)) == _lib.ESTATE
        with pytest.raises(_lib.IcelkError) as e:
            fresh.jpeg_resave_file()
        assert e.value.code == _lib.ESTATE


# ---- D4: the folder driver -------------------------------------------------------------------------------------------
T, DTS = 2, 60
FOLDER_CROP = (3, 5, 6, 7)
POLY = [(20, 30), (300, 25), (310, 225), (150, 200), (15, 230)]
FP = dict(maxCorners=300, qualityLevel=0.007, minDistance=8, blockSize=10)
LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))


def _track(names, dst, **kw):
    from iceberg_tracking_code_amd import track_image_sequence
    os.makedirs(dst, exist_ok=True)
    left, top = FOLDER_CROP[:2]
    return track_image_sequence(names, dst, T, DTS, mask_polygon=(POLY, left, top), feature_params=FP, lk_params=LK, decode_threads=2, **kw)


@pytest.fixture(scope="module")
def folder(synth, tmp_path_factory):
    """7 photos of 320 x 240 -- one saved progressive (it goes through PIL), two with a comment, the progressive one among
    them -- and the files the reference's crop step writes for them"""
    d = tmp_path_factory.mktemp("folder")
    grays, _ = synth.sequence(320, 240, 7, seed=33, max_step_px=2.0)
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


@pytest.mark.parametrize("mode", ["pil", "device", "device_huffman"])
def test_d4_folder_driver_writes_the_target_folder(folder, mode, monkeypatch):
    from iceberg_tracking_code_amd.tracker import SegmentTracker
    kw = dict(pil=dict(decoder="pil"), device=dict(decoder="device"), device_huffman=dict(decoder="device", huffman="device"))[mode]
    d = folder["dir"]
    written = []
    write = SegmentTracker._write_crop
    monkeypatch.setattr(SegmentTracker, "_write_crop", staticmethod(lambda path, data: (written.append(path), write(path, data))[1]))
    crops = str(d / ("crops_" + mode))
    got = _track(folder["names"], str(d / ("out_crops_" + mode)), crop=FOLDER_CROP, resave="reference", startlist=(0, 1), save_crops=crops, **kw)
    want = _track(folder["names"], str(d / ("out_plain_" + mode)), crop=FOLDER_CROP, resave="reference", startlist=(0, 1), **kw)
    assert sorted(os.listdir(crops)) == sorted(folder["cropped"])
    for name, data in folder["cropped"].items():
        with open(os.path.join(crops, name), "rb") as f:
            mine = f.read()
        assert mine == data, (name, _first_difference(mine, data))
    paths = [p for p in written if p is not None]
    assert len(paths) == len(set(paths)) == len(folder["names"])     # once per photo, whatever startlist visits
    assert len(got) == len(want) >= 3
    for (pg, tg, qg), (pw, tw, qw) in zip(got, want):
        assert os.path.basename(pg) == os.path.basename(pw) and len(tw) > 10
        assert np.array_equal(tg, tw) and np.array_equal(qg, qw)
        zg, zw = np.load(pg, allow_pickle=False), np.load(pw, allow_pickle=False)
        assert sorted(zg.files) == sorted(zw.files)
        for key in zg.files:
            assert np.array_equal(zg[key], zw[key]), key


def test_d4_refused_combinations(folder):
    from iceberg_tracking_code_amd import SegmentTracker
    never = str(folder["dir"] / "never")
    with pytest.raises(ValueError):
        _track(folder["names"], never, crop=FOLDER_CROP, save_crops=never)
    with pytest.raises(ValueError):
        _track(folder["names"], never, crop=FOLDER_CROP, decoder="device", huffman="device", pipeline=True, save_crops=never)
    with pytest.raises(ValueError):
        _track(folder["names"], never, crop=FOLDER_CROP, decoder="device", huffman="device", pipeline=True, resave="reference", save_crops=never)
    trk = SegmentTracker(314, 235, T, feature_params=FP, lk_params=LK)
    try:
        with pytest.raises(ValueError):
            trk.push_bgr(np.zeros((235, 314, 3), np.uint8), crop_file=os.path.join(never, "x.jpg"))
        with pytest.raises(ValueError):
            trk.push_jpeg(b"", crop_file=os.path.join(never, "x.jpg"))
    finally:
        trk.close()
    assert not os.path.exists(never) or not os.listdir(never)


def test_d5_same_bytes_run_to_run_and_after_a_larger_file(ctx):
    from iceberg_tracking_code_amd import resave_bytes
    small, large = rc.content("noise", 99, 131, seed=1), rc.content("noise", 640, 480, seed=2)
    a = resave_bytes(small, 100, ctx=ctx)
    b = resave_bytes(large, 100, ctx=ctx)
    assert resave_bytes(large, 100, ctx=ctx) == b
    assert resave_bytes(small, 100, ctx=ctx) == a                     # the buffers still hold the larger file's tail
    assert resave_bytes(small, 100, ctx=ctx) == a == resave_bytes(small, 100)
    assert b == resave_bytes(large, 100)

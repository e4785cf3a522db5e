"""GPU: the reference's lossy re-save of the crop on the device (csrc/k_jpeg_fwd.hip, then the decoder's kernels with the
re-save's tables) against Pillow -- coefficients, pixels, the three uploads, the folder driver -- and the defaults left
as they were.  Every comparison is exact equality."""
import ctypes as C
import datetime as dt
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_resave_cases as rc

pytestmark = pytest.mark.gpu

KINDS = ("noise", "smooth", "stripes")


def _pillow(rgb):
    """(Pillow's file for rgb, `read_jpeg` of it)"""
    from iceberg_tracking_code_amd import read_jpeg
    data = rc.pillow_save(rgb)
    return data, read_jpeg(data)


@pytest.mark.parametrize("size", rc.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_g1_device_coefficients_equal_pillows(ctx, size):
    w, h = size
    for kind in KINDS:
        rgb = rc.content(kind, w, h, seed=1)
        _, want = _pillow(rgb)
        got = ctx.jpeg_resave_device_coefficients(rgb)
        assert got.shape == want.coef.shape, (size, kind)
        assert np.array_equal(got, want.coef), (size, kind, int(np.count_nonzero(got != want.coef)))


def test_g1_other_quality_and_strided_rows(ctx):
    from iceberg_tracking_code_amd import read_jpeg
    big = rc.content("noise", 120, 70, seed=2)
    view = big[2:69, 7:106]                                 # 99 x 67, rows 360 bytes apart
    for q in (50, 95, 100):
        want = read_jpeg(rc.pillow_save(np.ascontiguousarray(view), q))
        coef = np.empty(want.coef.size, np.int16)
        ctx._ck(ctx._lib.icelk_jpeg_resave_device_coefficients(ctx._h, view.ctypes.data_as(C.POINTER(C.c_uint8)), 99, 67, view.strides[0], q,
                                                               C.c_void_p(coef.ctypes.data), coef.size))
        assert np.array_equal(coef, want.coef), q


@pytest.mark.parametrize("size", rc.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_g2_resave_rgb_equals_pillows_pixels(ctx, size):
    from iceberg_tracking_code_amd import resave_rgb
    w, h = size
    for kind in KINDS:
        rgb = rc.content(kind, w, h, seed=3)
        want = rc.pillow_open(rc.pillow_save(rgb))
        got = resave_rgb(rgb, ctx=ctx)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (size, kind, int(np.count_nonzero(got != want)))
    rgb = rc.content("smooth", w, h, seed=4)
    assert np.array_equal(resave_rgb(rgb, 90, ctx=ctx), rc.pillow_open(rc.pillow_save(rgb, 90)))


@pytest.fixture(scope="module")
def photo(tmp_path_factory):
    """a photo file, its decoded pixels, and the pixels of the reference's re-saved crop (camtools.py:64-104, call for call)"""
    d = tmp_path_factory.mktemp("resave")
    src, dst = str(d / "20190801-120000.jpg"), str(d / "cropped.jpg")
    data = rc.photo_file()
    with open(src, "wb") as f:
        f.write(data)
    rc.reference_crop_resave(src, dst, rc.CROP)
    return dict(data=data, pixels=np.array(Image.open(src)), resaved=np.array(Image.open(dst)))


@pytest.mark.parametrize("variant", [3, 4])
def test_g3_the_three_uploads(ctx, photo, variant):
    from iceberg_tracking_code_amd import read_jpeg
    ctx.upload_bgr(0, photo["resaved"], variant)
    want = ctx.download_level(0, 0)
    left, top, right, bottom = rc.CROP
    assert want.shape == (rc.PHOTO_SIZE[1] - top - bottom, rc.PHOTO_SIZE[0] - left - right)
    ctx.upload_bgr(1, photo["pixels"], variant, rc.CROP, resave="reference")
    got = ctx.download_level(1, 0)
    assert got.shape == want.shape and np.array_equal(got, want), ("upload_bgr", int(np.count_nonzero(got != want)))
    ctx.upload_jpeg(2, read_jpeg(photo["data"]), variant, rc.CROP, resave="reference")
    got = ctx.download_level(2, 0)
    assert got.shape == want.shape and np.array_equal(got, want), ("upload_jpeg", int(np.count_nonzero(got != want)))
    ctx.upload_jpeg_file(1, photo["data"], variant, rc.CROP, resave="reference")
    got = ctx.download_level(1, 0)
    assert got.shape == want.shape and np.array_equal(got, want), ("upload_jpeg_file", int(np.count_nonzero(got != want)))
    ctx.upload_jpeg_file(2, photo["data"], variant, rc.CROP, resave=75)      # the quality spelled out
    assert np.array_equal(ctx.download_level(2, 0), want)
    # the option matters: the slot differs from the one the plain upload leaves
    ctx.upload_bgr(0, photo["pixels"], variant, rc.CROP)
    assert not np.array_equal(ctx.download_level(0, 0), want)


# ---- G4: the folder driver -------------------------------------------------------------------------------------------
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
def folders(synth, tmp_path_factory):
    """8 photos of 320 x 240 (one saved progressive: it goes through PIL), Pillow's re-saved crops of them under the same
    names, and the tracks of the plain run on the originals"""
    d = tmp_path_factory.mktemp("folder")
    w, h, n = 320, 240, 8
    grays, _ = synth.sequence(w, h, n, seed=33, max_step_px=2.0)
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    os.makedirs(str(d / "photos"))
    os.makedirs(str(d / "cropped"))
    names, cropped = [], []
    for k, g in enumerate(grays):
        rgb = np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)
        name = (t0 + dt.timedelta(seconds=k * DTS)).strftime("%Y%m%d-%H%M%S") + ".jpg"
        Image.fromarray(rgb).save(str(d / "photos" / name), quality=92, progressive=(k == 3))
        rc.reference_crop_resave(str(d / "photos" / name), str(d / "cropped" / name), FOLDER_CROP)
        names.append(str(d / "photos" / name))
        cropped.append(str(d / "cropped" / name))
    plain = _track(names, str(d / "out_plain"), crop=FOLDER_CROP)
    return dict(dir=d, names=names, cropped=cropped, plain=plain)


@pytest.mark.parametrize("mode", ["pil", "device", "device_huffman"])
def test_g4_folder_driver(folders, mode):
    kw = dict(pil=dict(decoder="pil"), device=dict(decoder="device"), device_huffman=dict(decoder="device", huffman="device"))[mode]
    d = folders["dir"]
    got = _track(folders["names"], str(d / ("out_resave_" + mode)), crop=FOLDER_CROP, resave="reference", **kw)
    want = _track(folders["cropped"], str(d / ("out_cropped_" + mode)), **kw)
    assert len(got) == len(want) == len(folders["plain"]) >= 3
    differs = False
    for (pg, tg, qg), (pw, tw, qw), (pp, tp, qp) in zip(got, want, folders["plain"]):
        assert os.path.basename(pg) == os.path.basename(pw) == os.path.basename(pp)
        assert len(tw) > 10
        assert tg.shape == tw.shape and np.array_equal(tg, tw) and np.array_equal(qg, qw)
        zg, zw = np.load(pg, allow_pickle=False), np.load(pw, allow_pickle=False)
        assert np.array_equal(zg["tracks"], zw["tracks"]) and np.array_equal(zg["trackquality"], zw["trackquality"])
        differs |= tg.shape != tp.shape or not np.array_equal(tg, tp)
    assert differs, "the re-save changed no vertex: the option would not matter"


def test_g4_pipeline_with_resave_is_refused(folders):
    with pytest.raises(ValueError):
        _track(folders["names"], str(folders["dir"] / "never"), crop=FOLDER_CROP, decoder="device", huffman="device", pipeline=True,
               resave="reference")
    with pytest.raises(ValueError):
        _track(folders["names"], str(folders["dir"] / "never"), crop=FOLDER_CROP, resave="best")


# ---- G5 ------------------------------------------------------------------------------------------------------------------
def test_g5_defaults_unchanged(ctx, photo):
    from iceberg_tracking_code_amd import read_jpeg
    left, top, right, bottom = rc.CROP
    h, w = photo["pixels"].shape[:2]
    ctx.upload_bgr(0, np.ascontiguousarray(photo["pixels"][top:h - bottom, left:w - right]), 4)
    want = ctx.download_level(0, 0)
    ctx.upload_bgr(1, photo["pixels"], 4, rc.CROP, resave=None)
    assert np.array_equal(ctx.download_level(1, 0), want)
    ctx.upload_jpeg(2, read_jpeg(photo["data"]), 4, rc.CROP, resave=None)
    assert np.array_equal(ctx.download_level(2, 0), want)
    ctx.upload_jpeg_file(1, photo["data"], 4, rc.CROP, resave=None)
    assert np.array_equal(ctx.download_level(1, 0), want)
    ctx.upload_jpeg_file(2, photo["data"], 4, rc.CROP)
    assert np.array_equal(ctx.download_level(2, 0), want)


def test_g5_rejected_calls_leave_the_handle_working(ctx, photo):
    from iceberg_tracking_code_amd import _lib, read_jpeg
    from iceberg_tracking_code_amd._lib import IcelkError
    lib, px, data, j = ctx._lib, np.ascontiguousarray(photo["pixels"]), photo["data"], read_jpeg(photo["data"])
    h, w = px.shape[:2]
    u8 = px.ctypes.data_as(C.POINTER(C.c_uint8))
    narrow = (0, 0, w - 2, 0)                               # leaves a crop 2 pixels wide
    for q in (0, 101):
        assert lib.icelk_upload_bgr_resave(ctx._h, 0, u8, w, h, px.strides[0], 4, q) == _lib.EARG
        assert lib.icelk_upload_jpeg_resave(ctx._h, 0, C.byref(j.info), j.coef_ptr, 4, 0, 0, 0, 0, q) == _lib.EARG
        assert lib.icelk_upload_jpeg_file_resave(ctx._h, 0, data, len(data), 4, 0, 0, 0, 0, q) == _lib.EARG
        assert lib.icelk_jpeg_resave_rgb(ctx._h, u8, w, h, px.strides[0], q, u8, px.strides[0]) == _lib.EARG
    assert lib.icelk_upload_bgr_resave(ctx._h, 0, u8, 2, h, px.strides[0], 4, 75) == _lib.EARG
    assert lib.icelk_upload_jpeg_resave(ctx._h, 0, C.byref(j.info), j.coef_ptr, 4, *narrow, 75) == _lib.EARG
    assert lib.icelk_upload_jpeg_file_resave(ctx._h, 0, data, len(data), 4, *narrow, 75) == _lib.EARG
    assert lib.icelk_upload_bgr_resave(ctx._h, 99, u8, w, h, px.strides[0], 4, 75) == _lib.EARG       # no such slot
    assert lib.icelk_upload_bgr_resave(ctx._h, 0, u8, w, h, px.strides[0], 5, 75) == _lib.EARG        # no such gray variant
    for bad in (0, 101, "best"):
        with pytest.raises(ValueError):
            ctx.upload_bgr(0, px, 4, rc.CROP, resave=bad)
    with pytest.raises((ValueError, IcelkError)):
        ctx.upload_jpeg(0, j, 4, narrow, resave="reference")
    ctx.upload_bgr(0, photo["resaved"], 4)
    want = ctx.download_level(0, 0)
    ctx.upload_jpeg_file(1, data, 4, rc.CROP, resave="reference")
    assert np.array_equal(ctx.download_level(1, 0), want)

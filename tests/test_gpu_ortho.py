"""The orthophoto on the device (k_ortho_fill, k_ortho_add: csrc/k_ortho.hip) against the host statement, every byte of
rgb and cover, on the cases of tests/ortho_cases.py; the mosaic's rules, the three ways a source reaches the kernel, the
files the picture writer makes of the mosaic, the movie frame, the sequence driver and the refusals."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import ortho_cases as K
from iceberg_tracking_code_amd import (IcelkError, UnsupportedJpeg, _lib, frame_host, movie_size, ortho_coords_host, orthophoto, orthophoto_host,
                                       orthophoto_sequence, read_avi, read_world_file)
from iceberg_tracking_code_amd.orthophoto import opts_struct, raster_struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    """the host statement of every case, computed once"""
    return {c["name"]: orthophoto_host(c["views"], c["raster"], **c["opts"]) for c in K.CASES}


def same(got, want):
    assert got["cover"].shape == want["cover"].shape and got["rgb"].shape == want["rgb"].shape
    assert np.array_equal(got["cover"], want["cover"]), int(np.count_nonzero(got["cover"] != want["cover"]))
    assert np.array_equal(got["rgb"], want["rgb"]), int(np.count_nonzero(got["rgb"] != want["rgb"]))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c["name"])
def test_device_equals_the_host_statement(ctx, host, case):
    want = host[case["name"]]
    K.check_main(case, want["cover"])
    got = orthophoto(ctx, case["views"], case["raster"], format="png", **case["opts"])
    same(got, want)
    # the PNG holds exactly these pixels
    assert np.array_equal(np.array(Image.open(io.BytesIO(got["file"]))), want["rgb"])


def test_mosaic_rules(ctx, host):
    views = K.BY_NAME["mosaic"]["views"]
    a = orthophoto(ctx, views, K.MOSAIC_RASTER)
    same(a, host["mosaic"])
    order = [2, 0, 1]
    b = orthophoto(ctx, [views[k] for k in order], K.MOSAIC_RASTER)
    hb = orthophoto_host([views[k] for k in order], K.MOSAIC_RASTER)
    same(b, hb)
    # equal where no distances tie: the cameras' true distances from every pixel's centre, seen or not
    d2 = np.stack([ortho_coords_host(v[0], K.MOSAIC_RASTER, (v[1].shape[1], v[1].shape[0]))["d2"] for v in views])
    free = ~((d2[0] == d2[1]) | (d2[0] == d2[2]) | (d2[1] == d2[2]))
    assert free.mean() > 0.99
    relabel = np.array([0] + [order[k] + 1 for k in range(3)], np.uint8)
    assert np.array_equal(relabel[b["cover"]][free], a["cover"][free]) and np.array_equal(b["rgb"][free], a["rgb"][free])
    # the same camera under two indices: the first stays everywhere
    ctx.ortho_begin(K.FOOT)
    ctx.ortho_add(K.RGB[0], 4, K.RGB[1])
    once = ctx.ortho_write()
    ctx.ortho_add(K.RGB[0], 9, K.RGB[1])
    twice = ctx.ortho_write()
    assert set(np.unique(once["cover"])) == {0, 5} and np.array_equal(twice["cover"], once["cover"]) and np.array_equal(twice["rgb"], once["rgb"])
    assert np.array_equal(once["rgb"], host["foot_rgb"]["rgb"])
    # the camera that looks up changes nothing
    ctx.ortho_add(K.UP[0], 0, K.UP[1])
    again = ctx.ortho_write()
    assert np.array_equal(again["cover"], once["cover"]) and np.array_equal(again["rgb"], once["rgb"])


def _jpeg(img, **kw):
    return jc.encode(img, **kw)


@pytest.mark.parametrize("kind", ["444", "420", "gray"])
@pytest.mark.parametrize("forced_host_huffman", [False, True], ids=["device", "host_huffman"])
def test_jpeg_file_equals_pillows_pixels(ctx, kind, forced_host_huffman):
    cam = K.RGB[0]
    img = K.photo(96, 64, 1 if kind == "gray" else 3)
    data = _jpeg(img, quality=90) if kind == "gray" else _jpeg(img, quality=90, subsampling=0 if kind == "444" else 2)
    pixels = jc.pil_decode(data)
    assert pixels.shape == img.shape
    want = orthophoto_host([(cam, pixels)], K.FOOT)
    assert 0.1 < K.seen_fraction(want["cover"]) < 0.9
    ctx.jpeg_huff_config(max_hops=1, max_rounds=1) if forced_host_huffman else ctx.jpeg_huff_config()
    try:
        got = orthophoto(ctx, [(cam, data)], K.FOOT)
        assert (ctx.jpeg_huff_stats()["fallback"] != 0) == forced_host_huffman
    finally:
        ctx.jpeg_huff_config()
    same(got, want)
    same(orthophoto(ctx, [(cam, pixels)], K.FOOT), want)


def test_progressive_file_is_refused_and_the_driver_falls_back(ctx, tmp_path):
    buf = io.BytesIO()
    Image.fromarray(K.RGB[1]).save(buf, "JPEG", quality=92, progressive=True)
    data = buf.getvalue()
    cam = K.RGB[0].struct()
    ctx.ortho_begin(K.FOOT)
    assert ctx._lib.icelk_ortho_add_jpeg_file(ctx._h, C.byref(cam), 0, data, len(data)) == _lib.EUNSUP
    with pytest.raises(UnsupportedJpeg):
        ctx.ortho_add(K.RGB[0], 0, data)
    assert not ctx.ortho_write()["cover"].any()   # the refused file left the mosaic as begun
    path = tmp_path / "progressive.jpg"
    path.write_bytes(data)
    want = orthophoto_host([(K.RGB[0], jc.pil_decode(data))], K.FOOT)
    same(orthophoto(ctx, [(K.RGB[0], data)], K.FOOT), want)
    same(orthophoto(ctx, [(K.RGB[0], str(path))], K.FOOT), want)


def test_slot_equals_pixels(ctx, host):
    cam, gray = K.GRAY
    ctx.upload_gray(1, gray)
    case = K.BY_NAME["foot_fill"]
    same(orthophoto(ctx, [(cam, ("slot", 1))], case["raster"], **case["opts"]), host["foot_fill"])
    same(orthophoto(ctx, [(cam, gray)], case["raster"], **case["opts"]), host["foot_fill"])
    # the slot is still what it was, and a new frame enters it afterwards as ever
    assert np.array_equal(ctx.download_level(1, 0), gray)
    ctx.upload_gray(1, np.ascontiguousarray(gray[::-1]))
    flipped = orthophoto(ctx, [(cam, ("slot", 1))], case["raster"], **case["opts"])
    same(flipped, orthophoto_host([(cam, np.ascontiguousarray(gray[::-1]))], case["raster"], **case["opts"]))


@pytest.mark.parametrize("quality", [90, 35])
def test_jpeg_is_pillows_file(ctx, host, quality):
    got = orthophoto(ctx, [K.RGB], K.FOOT, format="jpeg", quality=quality)
    same(got, host["foot_rgb"])
    buf = io.BytesIO()
    Image.fromarray(host["foot_rgb"]["rgb"]).save(buf, "JPEG", quality=quality)
    assert got["file"] == buf.getvalue()


def test_strides_capacity_and_the_movie_frame(ctx, host):
    want = host["odd_67x45"]
    case = K.BY_NAME["odd_67x45"]
    h, w = want["cover"].shape
    ctx.ortho_begin(case["raster"])
    ctx.ortho_add(case["views"][0][0], 0, case["views"][0][1])
    rgb, cover = np.full((h, 3 * w + 11), 0xA5, np.uint8), np.full((h, w + 5), 0x5A, np.uint8)
    u8 = _lib.u8p
    n = C.c_uint64(0)
    small = np.full(64, 0xEE, np.uint8)
    call = lambda out, cap: ctx._lib.icelk_ortho_write(ctx._h, 1, 0, rgb.ctypes.data_as(u8), rgb.strides[0], cover.ctypes.data_as(u8),   # noqa: E731
                                                       cover.strides[0], out, cap, C.byref(n))
    assert call(small.ctypes.data, small.size) == _lib.ECAP and n.value > small.size and (small == 0xEE).all()
    assert call(None, 0) == _lib.ECAP
    big = np.zeros(n.value, np.uint8)
    need = n.value
    assert call(big.ctypes.data, big.size) == _lib.OK and n.value == need   # the repeat
    assert np.array_equal(rgb[:, :3 * w].reshape(h, w, 3), want["rgb"]) and (rgb[:, 3 * w:] == 0xA5).all()
    assert np.array_equal(cover[:, :w], want["cover"]) and (cover[:, w:] == 0x5A).all()
    assert np.array_equal(np.array(Image.open(io.BytesIO(big.tobytes()))), want["rgb"])
    # the picture writer saw the mosaic last: the movie frame is made of it
    assert ctx.picture_size() == (w, h)
    size = movie_size(w, h, 160)
    assert ctx.picture_frame(size, 90) == frame_host(want["rgb"], size, 90)
    # and the mosaic is still there
    same(ctx.ortho_write(), want)


def test_sequence_writes_pictures_world_files_and_a_movie(ctx, host, tmp_path):
    views = K.BY_NAME["mosaic"]["views"]
    frames = [("20190724-1000", views), ("20190724-1010", views[:2]), ("20190724-1020", views[1:])]
    written = orthophoto_sequence(frames, str(tmp_path), K.MOSAIC_RASTER, movie=True, ctx=ctx)
    assert [p.rsplit("/", 1)[1] for p in written] == ["20190724-1000_ortho.png", "20190724-1010_ortho.png", "20190724-1020_ortho.png", "ortho_35m.avi"]
    wants = [orthophoto_host(v, K.MOSAIC_RASTER)["rgb"] for _, v in frames]
    for path, want in zip(written, wants):
        assert np.array_equal(np.array(Image.open(path)), want)
        x0, y0, res = read_world_file(open(path[:-3] + "pgw").read())
        assert (x0, y0, res) == (K.MOSAIC_RASTER["x0"], K.MOSAIC_RASTER["y0"], K.MOSAIC_RASTER["res"])
    film = read_avi(written[-1])
    h, w = wants[0].shape[:2]
    size = movie_size(w, h, 2000)
    assert len(film["frames"]) == 3 and film["frames"][0] == frame_host(wants[0], size, 90)
    jpegs = orthophoto_sequence(frames[:1], str(tmp_path), K.MOSAIC_RASTER, format="jpeg", ctx=ctx)
    assert [p.rsplit("/", 1)[1] for p in jpegs] == ["20190724-1000_ortho.jpg"] and (tmp_path / "20190724-1000_ortho.jgw").exists()


def test_refusals_leave_the_handle_working(host):
    from iceberg_tracking_code_amd import Context
    c = Context(128, 96, n_slots=2, max_pts=1024)
    try:
        L, h = c._lib, c._h
        cam, img = K.RGB[0].struct(), K.RGB[1]
        n = C.c_uint64(0)
        file = np.full(1 << 16, 0xEE, np.uint8)
        rgb = np.full((120, 360), 0xA5, np.uint8)
        add = lambda index=0, p=img.ctypes.data, ch=3, stride=img.strides[0], cm=C.byref(cam): L.icelk_ortho_add_pixels(   # noqa: E731
            h, cm, index, p, 96, 64, ch, stride)
        write = lambda fmt=1, ln=C.byref(n): L.icelk_ortho_write(h, fmt, 90, rgb.ctypes.data_as(_lib.u8p), rgb.strides[0], None, 0,   # noqa: E731
                                                                file.ctypes.data, file.size, ln)
        # before a begin
        assert add() == _lib.ESTATE and write() == _lib.ESTATE
        assert L.icelk_ortho_add_jpeg_file(h, C.byref(cam), 0, b"\xff\xd8", 2) == _lib.ESTATE
        assert L.icelk_ortho_add_slot(h, C.byref(cam), 0, 0) == _lib.ESTATE   # an empty slot
        with pytest.raises(IcelkError):
            c.ortho_write()
        # a raster that cannot be begun
        for bad in (dict(res=0.0), dict(res=-2.0), dict(x0=np.nan), dict(res=np.inf), dict(width=0), dict(height=16385), dict(width=16385)):
            r = raster_struct(dict(K.FOOT, **bad))
            assert L.icelk_ortho_begin(h, C.byref(r), None) == _lib.EARG, bad
        assert L.icelk_ortho_begin(h, None, None) == _lib.EARG
        o = opts_struct()
        o.sampling = 2
        r = raster_struct(K.FOOT)
        assert L.icelk_ortho_begin(h, C.byref(r), C.byref(o)) == _lib.EARG
        assert add() == _lib.ESTATE   # none of them began anything
        # begun: what an add and a write refuse
        c.ortho_begin(K.FOOT)
        assert add(index=255) == _lib.EARG and add(index=-1) == _lib.EARG and add(p=None) == _lib.EARG and add(cm=None) == _lib.EARG
        assert add(ch=2) == _lib.EARG and add(stride=3 * 96 - 1) == _lib.EARG
        assert L.icelk_ortho_add_slot(h, C.byref(cam), 0, 7) == _lib.EARG and L.icelk_ortho_add_slot(h, C.byref(cam), 0, 1) == _lib.ESTATE
        assert L.icelk_ortho_add_jpeg_file(h, C.byref(cam), 255, b"\xff\xd8", 2) == _lib.EARG
        assert write(ln=None) == _lib.EARG and write(fmt=2) == _lib.EARG
        assert (file == 0xEE).all() and (rgb == 0xA5).all()   # no refusal touched an output buffer
        # the handle works afterwards
        assert add() == _lib.OK
        same(c.ortho_write("png"), host["foot_rgb"])
        # a JPEG needs three pixels of width: refused by the write, while the PNG and the pixels are there
        c.ortho_begin(K.BY_NAME["one_pixel"]["raster"])
        c.ortho_add(K.RGB[0], 0, K.RGB[1])
        with pytest.raises(ValueError):
            c.ortho_write("jpeg")
        same(c.ortho_write("png"), host["one_pixel"])
        # another kind of picture ends the mosaic
        c.ortho_begin(K.FOOT)
        c.upload_gray(0, K.photo(96, 64, 1))
        c.plot_tracks(0, np.zeros((0, 2, 2), np.float32), width=96)
        assert add() == _lib.ESTATE and write() == _lib.ESTATE
        c.ortho_begin(K.FOOT)
        assert add() == _lib.OK
        same(c.ortho_write(), host["foot_rgb"])
    finally:
        c.close()

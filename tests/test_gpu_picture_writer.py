"""The picture writer that the segment picture and the velocity map share (csrc/abi_picture.hip): one
handle drawing both kinds in turn on the one working set, the short file buffer for the PNG map, the refusals in front of
the first allocation, and -- without a GPU -- the helper of context.py that offers a file buffer.  The references are
Pillow's writer and the host statements (plot_overlay_host, map_overlay_host, encode_png_host)."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import map_cases as mc
import plot_cases as pc

gpu = pytest.mark.gpu

FRAME = (45, 27)       # of the segment picture: at width 9 a 9 x 5 picture, at width 40 one of 40 x 24
MAP_HEIGHT = 33        # 64 x 33 is a multiple of four pixels; 65 x 33 = 2145 leaves one for the byte-by-byte tail


def _pillow(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def _map(width):
    """one panel of map_cases in a picture width x 33"""
    vw, vh = width - 12, MAP_HEIGHT - 9
    base = dict(view=(2, 5, vw, vh), bar=(4 + vw, 4), limits=(mc.X0, mc.X0 + mc.M * vw, mc.Y0, mc.Y0 + mc.M * vh))
    return dict(width=width, height=MAP_HEIGHT, quality=90, table=mc.table(), texts=mc.texts_of(width, MAP_HEIGHT),
                panels=[mc.panel_of(base, *mc.VARIANTS[0][0])])


def _small_context():
    from iceberg_tracking_code_amd import Context
    return Context(64, 48, n_slots=1, max_pts=64)


def _draw(c, step):
    """(file, R G B) of ("plot", width) | ("jpeg", width) | ("png", width) on handle c, whose slot 0 holds the frame"""
    kind, width = step
    if kind == "plot":
        _, tracks, stamp, _ = pc.case(*FRAME, width, 5)
        return c.plot_tracks(0, tracks, width, stamp, 85, want_rgb=True)
    return c.map_draw(_map(width), want_rgb=True, format=kind)


def _want(step):
    """(file, R G B) by the host statements and Pillow"""
    from iceberg_tracking_code_amd import encode_png_host, map_overlay_host, plot_overlay_host
    kind, width = step
    if kind == "plot":
        gray, tracks, stamp, _ = pc.case(*FRAME, width, 5)
        rgb = plot_overlay_host(gray, tracks, width, stamp)
        return _pillow(rgb, 85), rgb
    rgb = map_overlay_host(_map(width))
    return (encode_png_host(rgb) if kind == "png" else _pillow(rgb, 90)), rgb


@gpu
def test_one_handle_alternating_pictures():
    """pixels per picture: 960, 2145, 2112, 45, 2112 -- the shared R G B and coefficients grow at the second call and are
    larger than the picture at the third and fourth; the fifth follows the smallest"""
    steps = [("plot", 40), ("jpeg", 65), ("png", 64), ("plot", 9), ("jpeg", 64)]
    gray = pc.case(*FRAME, 9, 5)[0]
    with _small_context() as one:
        one.upload_gray(0, gray)
        got = [_draw(one, s) for s in steps]
    for step, (data, rgb) in zip(steps, got):
        want_data, want_rgb = _want(step)
        assert rgb.shape == want_rgb.shape and np.array_equal(rgb, want_rgb), step
        assert data == want_data, step
        with _small_context() as fresh:
            fresh.upload_gray(0, gray)
            again = _draw(fresh, step)
        assert data == again[0] and np.array_equal(rgb, again[1]), step
    assert got[0][1].shape == (24, 40, 3) and got[3][1].shape == (5, 9, 3) and got[1][1].shape == (MAP_HEIGHT, 65, 3)


@gpu
def test_png_map_short_buffer(ctx):
    from iceberg_tracking_code_amd import _lib, encode_png_host, map_descriptor, map_overlay_host
    pic = _map(64)
    want = map_overlay_host(pic)
    whole = encode_png_host(want)
    d, keep = map_descriptor(pic)
    n = C.c_uint64(0)
    buf = np.full(len(whole) + 16, 0xAA, np.uint8)
    rgb = np.zeros((MAP_HEIGHT, 64, 3), np.uint8)

    def call(cap, with_rgb):
        ptr, stride = (rgb.ctypes.data_as(_lib.u8p), rgb.strides[0]) if with_rgb else (None, 0)
        return ctx._lib.icelk_map_draw_png(ctx._h, C.byref(d), None, 0, ptr, stride, C.c_void_p(buf.ctypes.data), cap, C.byref(n))
    for with_rgb in (True, False):
        for cap in (len(whole) - 1, 0):
            n.value = 0
            assert call(cap, with_rgb) == _lib.ECAP, (cap, with_rgb)
            assert n.value == len(whole) and (buf == 0xAA).all(), (cap, with_rgb)
        rgb[:] = 0
        assert call(len(whole), with_rgb) == _lib.OK and n.value == len(whole)
        assert buf[:len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAA).all()
        assert not with_rgb or np.array_equal(rgb, want)
        buf[:] = 0xAA
    del keep


@gpu
def test_refusals_come_before_the_first_allocation():
    """a fresh handle has no working set: a null length and a short R G B stride are refused by the writer's check, for
    both kinds of picture, with nothing written; the first correct call then allocates and gives the reference's bytes"""
    from iceberg_tracking_code_amd import _lib, map_descriptor
    gray, tracks, stamp, _ = pc.case(*FRAME, 40, 5)
    tracks = np.ascontiguousarray(tracks)
    pic = _map(64)
    d, keep = map_descriptor(pic)
    n = C.c_uint64(77)
    buf = np.full(1 << 16, 0xAA, np.uint8)
    rgb = np.full((MAP_HEIGHT, 64, 3), 0xAA, np.uint8)
    out, rgb_ptr = C.c_void_p(buf.ctypes.data), rgb.ctypes.data_as(_lib.u8p)
    with _small_context() as c:
        c.upload_gray(0, gray)
        L, h = c._lib, c._h

        def png(ptr, stride, length):
            return L.icelk_map_draw_png(h, C.byref(d), None, 0, ptr, stride, out, buf.size, length)

        def plot(ptr, stride, length):
            return L.icelk_plot_tracks(h, 0, tracks.ctypes.data_as(_lib.f32p), tracks.shape[0], tracks.shape[1], 40, stamp.encode(), 85, ptr,
                                       stride, out, buf.size, length)
        for draw, width in ((png, 64), (plot, 40)):
            assert draw(None, 0, None) == _lib.EARG
            assert L.icelk_last_error(h) == b"null length"
            assert draw(rgb_ptr, 3 * width - 1, C.byref(n)) == _lib.EARG
            assert L.icelk_last_error(h) == b"rgb stride smaller than 3 x the picture's width"
            assert n.value == 77 and (buf == 0xAA).all() and (rgb == 0xAA).all()
        for step in (("png", 64), ("plot", 40)):
            data, got = _draw(c, step)
            want_data, want_rgb = _want(step)
            assert data == want_data and np.array_equal(got, want_rgb), step
    del keep


def test_file_call_offers_the_size_the_call_names():
    """context._file_call with a stub in the library's place: no library is loaded, no Context made"""
    from iceberg_tracking_code_amd import _lib
    from iceberg_tracking_code_amd.context import FIRST_GUESSES, _file_call
    assert FIRST_GUESSES == dict(crop=1 << 16, resave=1 << 16, plot=1 << 18, map_jpeg=1 << 18, map_png=1 << 18)
    size = (1 << 20) + 3
    payload = (np.arange(size) % 251).astype(np.uint8)
    offered = []

    def stub(out, cap, n):
        offered.append(cap)
        n._obj.value = size
        if cap < size:
            return _lib.ECAP
        C.memmove(out, payload.ctypes.data, size)
        return _lib.OK
    guesses = dict(FIRST_GUESSES)
    assert _file_call(guesses, "plot", stub, "stub") == payload.tobytes()
    assert offered == [1 << 18, size]
    assert guesses == dict(FIRST_GUESSES, plot=max(1 << 16, size + size // 4))
    # the next one is offered what was remembered, plus what the caller adds (a comment's length)
    del offered[:]
    assert _file_call(guesses, "plot", stub, "stub", extra=5) == payload.tobytes()
    assert offered == [size + size // 4 + 5]
    # a small file: never less than 1 << 16 is remembered
    size = 100
    assert _file_call(guesses, "crop", stub, "stub") == payload[:100].tobytes() and guesses["crop"] == 1 << 16
    # any other code, and a second ICELK_ECAP, raise as _encode_call does; the guess stays
    before = dict(guesses)
    for rc, kind in ((_lib.ESTATE, _lib.IcelkError), (_lib.EHIP, _lib.IcelkError), (_lib.EARG, ValueError), (_lib.ENOMEM, MemoryError),
                     (_lib.ECAP, _lib.IcelkError)):
        calls = []

        def failing(out, cap, n, rc=rc):
            calls.append(cap)
            n._obj.value = cap + 1
            return rc
        with pytest.raises(kind) as e:
            _file_call(guesses, "map_png", failing, "stub")
        assert e.value.code == rc and "stub" in str(e.value)
        assert len(calls) == (2 if rc == _lib.ECAP else 1)
    assert guesses == before

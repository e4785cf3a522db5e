"""GPU: the PNG writer on the device (csrc/k_png.hip behind icelk_png_encode_rgb) against the host statement
of the same file (tests/test_png_host.py pins that one to zlib, Pillow and a numpy restatement) -- every byte, on the
pictures of tests/png_cases.py --, the working set's growth and reuse, and the call's refusals."""
import ctypes as C

import numpy as np
import pytest

import png_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_file_equals_host_statement(ctx, name):
    from iceberg_tracking_code_amd import encode_png_host
    rgb = pc.case(name)
    want = encode_png_host(rgb)
    got = ctx.png_encode(rgb)
    assert len(got) == len(want)
    assert got == want, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)


def test_working_set_grows_and_is_reused(ctx):
    from iceberg_tracking_code_amd import encode_png_host
    large, small = pc.case("pitch 32770"), pc.case("1x1")
    flat = pc.case(pc.LARGEST)
    once = ctx.png_encode(flat)
    assert ctx.png_encode(small) == encode_png_host(small)
    assert ctx.png_encode(flat) == once == encode_png_host(flat)                         # the largest case twice, a small one between
    noise = np.random.default_rng(11).integers(0, 256, (64, 512, 3), dtype=np.uint8)   # as many filtered bytes as the largest flat case
    first = ctx.png_encode(noise)
    assert ctx.png_encode(small) == encode_png_host(small)
    assert ctx.png_encode(noise) == first == encode_png_host(noise)
    assert ctx.png_encode(large) == encode_png_host(large)
    assert ctx.png_encode(pc.case(pc.LARGEST)) == encode_png_host(pc.case(pc.LARGEST))   # zeros where noise was
    view = noise[:, 3:200]                                                               # rows farther apart than 3 w
    assert ctx.png_encode(view) == encode_png_host(view.copy())


def test_refusals_and_the_capacity_protocol(ctx):
    from iceberg_tracking_code_amd import _lib, encode_png_host
    lib, h = ctx._lib, ctx._h
    n = C.c_uint64(0)
    px = np.full(48, 9, np.uint8)
    p, out = px.ctypes.data_as(_lib.u8p), np.zeros(256, np.uint8)
    o = C.c_void_p(out.ctypes.data)
    for w, hh in ((0, 1), (1, 0), (16385, 1), (16384, 5462)):
        assert lib.icelk_png_encode_rgb(h, p, w, hh, 3 * w, o, 256, C.byref(n)) == _lib.EARG
    assert lib.icelk_png_encode_rgb(h, p, 4, 4, 11, o, 256, C.byref(n)) == _lib.EARG
    assert lib.icelk_png_encode_rgb(h, None, 4, 4, 12, o, 256, C.byref(n)) == _lib.EARG
    assert lib.icelk_png_encode_rgb(h, p, 4, 4, 12, o, 256, None) == _lib.EARG
    want = encode_png_host(px.reshape(4, 4, 3))
    assert lib.icelk_png_encode_rgb(h, p, 4, 4, 12, o, 16, C.byref(n)) == _lib.ECAP and n.value == len(want) and not out.any()
    assert lib.icelk_png_encode_rgb(h, p, 4, 4, 12, o, 256, C.byref(n)) == _lib.OK and out[:n.value].tobytes() == want

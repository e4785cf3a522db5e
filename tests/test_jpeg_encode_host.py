"""The JPEG writer, the part that needs no GPU: the host statement of the entropy coder (csrc/jpeg_enc.h walked serially,
csrc/jpeg_enc_host.h) and the header against the files Pillow writes, against the reference's crop-and-save call for call,
and -- on hand-made coefficients that reach the coder's edges -- against tests/jpeg_writer.py.  Every comparison is
equality of bytes."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_cases as ec
import jpeg_resave_cases as rc

# 1x1, a height with h mod 16 = 1 and one with h mod 16 = 3 (in 2 .. 8: chroma is not padded to 16 rows there)
QUALITY_SIZES = ((1, 1), (17, 33), (99, 131))


def _first_difference(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d" % (len(a), len(b), k)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: "%dx%d" % s)
def test_e1_resave_bytes_equal_pillows_file_quality_75(size):
    from iceberg_tracking_code_amd import resave_bytes
    w, h = size
    for kind in rc.CONTENTS:
        rgb = rc.content(kind, w, h)
        want = rc.pillow_save(rgb)                           # no quality named, as the reference saves
        got = resave_bytes(rgb)
        assert got == want, (size, kind, _first_difference(got, want))
        assert resave_bytes(rgb, 75) == want and resave_bytes(rgb, "reference") == want


@pytest.mark.parametrize("quality", (1, 20, 50, 95, 100))
@pytest.mark.parametrize("size", QUALITY_SIZES, ids=lambda s: "%dx%d" % s)
def test_e1_resave_bytes_other_qualities(size, quality):
    from iceberg_tracking_code_amd import resave_bytes
    w, h = size
    for kind in rc.CONTENTS:
        rgb = rc.content(kind, w, h, seed=quality)
        want = rc.pillow_save(rgb, quality)
        got = resave_bytes(rgb, quality)
        assert got == want, (size, kind, quality, _first_difference(got, want))


def _source_photo(tmp_path, comment, **kw):
    """a photo as a file that carries dpi, Exif and (optionally) a comment and whatever else `kw` says"""
    exif = Image.Exif()
    exif[0x010F] = "a camera maker"
    path = str(tmp_path / "20190801-120000.jpg")
    if comment is not None:
        kw["comment"] = comment
    Image.fromarray(rc.content("smooth", *rc.PHOTO_SIZE, seed=3)).save(path, "JPEG", quality=90, subsampling=2, dpi=(300, 300),
                                                                         exif=exif, **kw)
    return path


@pytest.mark.parametrize("comment", (None, b"time-lapse camera 7, firmware 1.2"), ids=("no-comment", "comment"))
def test_e2_header_and_metadata(tmp_path, comment):
    from iceberg_tracking_code_amd import read_jpeg, resave_bytes, source_comment
    from iceberg_tracking_code_amd.jpeg import encode_header
    src = _source_photo(tmp_path, comment)
    with open(src, "rb") as f:
        data = f.read()
    im = Image.open(src)
    assert im.info.get("dpi") is not None and im.getexif()[0x010F] == "a camera maker"
    assert im.info.get("comment") == comment and source_comment(data) == comment
    left, top, right, bottom = rc.CROP
    w, h = im.size
    crop = im.crop((left, top, w - right, h - bottom))
    f = io.BytesIO()
    crop.save(f, "JPEG")
    want = f.getvalue()
    got = resave_bytes(np.array(crop), comment=comment)
    assert got == want, _first_difference(got, want)
    # the header alone: everything of Pillow's file up to the first byte of the scan
    head = encode_header(read_jpeg(want).info, comment)
    assert want.startswith(head) and len(head) == len(want) - len(ec.segments(want)[1]) - 2
    markers = [m for m, _ in ec.segments(want)[0]]
    assert markers == [0xE0] + ([0xFE] if comment is not None else []) + [0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert ec.bodies(want, 0xE0)[0] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert [b[0] for b in ec.bodies(want, 0xC4)] == [0x00, 0x10, 0x01, 0x11]
    assert ec.bodies(want, 0xDA)[0] == bytes.fromhex("03010002110311003f00")


def test_e2_last_comment_and_icc_profile(tmp_path):
    """Pillow reports the LAST COM segment, and `crop().save()` does not carry an ICC profile over (it writes one only when
    `save` is given `icc_profile=`): the crop of a photo with a profile is the plain file the header writer makes"""
    from iceberg_tracking_code_amd import resave_bytes, source_comment
    two = ec.pillow_file()
    two = two[:2] + b"\xff\xfe\x00\x07first" + two[2:20] + b"\xff\xfe\x00\x08second" + two[20:]
    assert Image.open(io.BytesIO(two)).info["comment"] == b"second" == source_comment(two)
    src = _source_photo(tmp_path, b"with a profile", icc_profile=b"not a real profile, but carried as bytes" * 4)
    im = Image.open(src)
    assert im.info.get("icc_profile")
    crop = im.crop((1, 2, 100, 90))
    f = io.BytesIO()
    crop.save(f, "JPEG")
    assert 0xE2 not in [m for m, _ in ec.segments(f.getvalue())[0]]
    assert resave_bytes(np.array(crop), comment=b"with a profile") == f.getvalue()


def test_e3_reference_crop_and_save_file(tmp_path):
    """crop_image_standalone (camtools.py:64-104) call for call on the 131 x 99 photo with the box 3, 5, 6, 7: the file"""
    from iceberg_tracking_code_amd import resave_bytes, source_comment
    src, dst = str(tmp_path / "20190801-120000.jpg"), str(tmp_path / "cropped.jpg")
    with open(src, "wb") as f:
        f.write(rc.photo_file())
    rc.reference_crop_resave(src, dst, rc.CROP)
    with open(dst, "rb") as f:
        want = f.read()
    left, top, right, bottom = rc.CROP
    w, h = rc.PHOTO_SIZE
    photo = np.array(Image.open(src))
    with open(src, "rb") as f:
        comment = source_comment(f.read())
    got = resave_bytes(photo[top:h - bottom, left:w - right], "reference", comment=comment)   # a strided view
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("mode,subsampling", (("RGB", 0), ("RGB", 1), ("RGB", 2), ("L", None)), ids=("444", "422", "420", "gray"))
def test_e4_lossless_round_trip(mode, subsampling):
    from iceberg_tracking_code_amd import encode_jpeg, read_jpeg
    for size, quality in (((99, 131), 85), ((16, 16), 100), ((33, 7), 30)):
        kw = {} if subsampling is None else {"subsampling": subsampling}
        f = ec.pillow_file(mode, size, quality=quality, **kw)
        got = encode_jpeg(read_jpeg(f))
        assert got == f, (size, quality, _first_difference(got, f))


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_e5_hand_made_coefficients(name):
    from iceberg_tracking_code_amd import encode_jpeg, read_jpeg
    j = ec.CASES[name]()
    got, want = encode_jpeg(j), ec.writer_file(j)
    (gs, gscan), (ws, wscan) = ec.segments(got), ec.segments(want)
    assert gscan == wscan, _first_difference(gscan, wscan)
    for marker in (0xDB, 0xC0, 0xDA):
        assert ec.bodies(got, marker) == ec.bodies(want, marker), hex(marker)
    # the header differs from the test writer's in the JFIF density and the order of the DHT segments only
    assert sorted(ec.bodies(got, 0xC4)) == sorted(ec.bodies(want, 0xC4))
    assert [m for m, _ in gs if m != 0xC4] == [m for m, _ in ws if m != 0xC4]
    back = read_jpeg(got)
    assert np.array_equal(back.coef, j.coef)
    if name == "padded_ff":
        assert got[-4:] == b"\xff\x00\xff\xd9" and got[-5] != 0xFF
    if name == "mostly_ff":
        assert 2 * gscan.count(b"\xff\x00") > len(gscan) - gscan.count(b"\xff\x00")


def test_e5_errors():
    from iceberg_tracking_code_amd import _lib, encode_jpeg
    lib = _lib.load()
    for make, code, exc in ((ec.ac_without_code, _lib.EARG, ValueError), (ec.dc_without_code, _lib.EARG, ValueError),
                            (ec.with_restarts, _lib.EUNSUP, ValueError)):
        with pytest.raises(exc) as e:
            encode_jpeg(make())
        assert e.value.code == code
    for ok in (1023, -1023):
        j = ec.descriptor(16, 16)
        j.blocks(1)[0, 0, 3, 3] = ok
        assert ec.segments(encode_jpeg(j))[1] == ec.segments(ec.writer_file(j))[1]
    j = ec.dc_staircase()
    whole = encode_jpeg(j)
    n = C.c_uint64(0)
    call = lambda buf, cap: lib.icelk_jpeg_encode_coefficients_host(C.byref(j.info), j.coef_ptr, None, 0, buf, cap, C.byref(n))
    assert call(None, 0) == _lib.ECAP and n.value == len(whole)
    buf = np.full(len(whole), 0xAA, np.uint8)
    n.value = 0
    assert call(C.c_void_p(buf.ctypes.data), len(whole) - 1) == _lib.ECAP and n.value == len(whole)
    assert call(C.c_void_p(buf.ctypes.data), len(whole)) == _lib.OK and buf.tobytes() == whole
    bad = ec.ac_without_code()
    buf[:] = 0xAA
    assert lib.icelk_jpeg_encode_coefficients_host(C.byref(bad.info), bad.coef_ptr, None, 0, C.c_void_p(buf.ctypes.data), buf.size,
                                                   C.byref(n)) == _lib.EARG
    assert (buf == 0xAA).all()                               # nothing is written

"""The crop stage without a GPU: the budget decisions of csrc/jpeg_enc.h (which the device-sized kernels of
csrc/k_jpeg_enc.hip take on their control words) against Python arithmetic at their edges, the budgeted host walk
(csrc/jpeg_enc_host.h) against the plain host writer, and what `crop_image_sequence` does before it touches a device:
an empty list, bad arguments, and the `"pil"` route on a truncated photo against Pillow's own truncated-load
crop-and-save (camtools.py:83-104).  Every comparison is equality."""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

import jpeg_resave_cases as rc

CODED, OVER, INVALID = 1, 2, 3
CHUNK, GROUP = 64, 256


def _budget(blocks, bpb, bits, invalid, ff):
    from iceberg_tracking_code_amd import _lib
    out = (C.c_uint32 * 8)()
    assert _lib.load().icelk_jpeg_enc_budget(blocks, bpb, bits, invalid, ff, out) == _lib.OK
    return list(out)


def _model(blocks, bpb, bits, invalid, ff):
    """the same eight words in Python's unbounded integers"""
    cap = blocks * bpb
    chunks = -(-cap // CHUNK)
    packed = -(-bits // 8)
    pack_runs = int(not invalid and packed <= cap)
    stuff_runs = int(bool(pack_runs) and packed + ff <= cap)
    verdict = INVALID if invalid else (CODED if stuff_runs else OVER)
    return [cap, chunks, -(-chunks // GROUP), packed, pack_runs, packed if pack_runs else 0, stuff_runs, verdict]


def test_budget_decisions_at_their_edges():
    cases = []
    blocks, bpb = 78, 13                                   # cap 1014
    cap = blocks * bpb
    for ff in (0, 1, 46):
        p = cap - ff
        cases += [(blocks, bpb, 8 * p, 0, ff),             # the stuffed stream is exactly the capacity
                  (blocks, bpb, 8 * p - 7, 0, ff),         # ... with its last byte begun by one bit
                  (blocks, bpb, 8 * p + 1, 0, ff),         # one byte more
                  (blocks, bpb, 8 * p, 0, ff + 1)]         # one stuffed byte more
    cases += [(blocks, bpb, 8 * 980, 0, 46),               # packed fits, stuffed does not (stripes at quality 95 on 200 x 9)
              (blocks, 14, 8 * 980, 0, 46),                # ... one byte per block more: both fit
              (blocks, bpb, 8 * cap, 0, 0), (blocks, bpb, 8 * cap + 1, 0, 0),
              (blocks, bpb, 8 * 100, 1, 0), (blocks, bpb, 8 * 100, 7, 3), (blocks, 416, 0, 1, 0),   # JE_INVALID set
              (blocks, bpb, 0, 0, 0), (blocks, bpb, 1, 0, 0), (blocks, bpb, 0xFFFFFFFF, 0, 0), (blocks, bpb, 0xFFFFFFF9, 0, 0xFFFFFFFF),
              (blocks, bpb, 8, 0, 0xFFFFFFFF)]
    for bits in (0, 1, 8, 9, 1660, 8 * 416, 8 * 416 + 1):  # 1 block, from one byte to its most
        cases += [(1, 1, bits, 0, 0), (1, 208, bits, 0, 1), (1, 416, bits, 0, 208), (1, 416, bits, 0, 209)]
    for b in (63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 32768, 32769):   # chunk counts at 64-byte and 16-KiB boundaries
        cases += [(b, 1, 8 * b, 0, 0), (b, 1, 8 * b - 8, 0, 1), (b, 1, 8 * b - 8, 0, 2)]
    big = 2587000 * 416 - 2 ** 29                          # the largest capacity, the most bits 32 bits count: 2^29 packed bytes
    cases += [(2587000, 416, 0xFFFFFFFF, 0, 0), (2587000, 416, 0xFFFFFFFF, 0, big), (2587000, 416, 0xFFFFFFFF, 0, big + 1)]
    for case in cases:
        assert _budget(*case) == _model(*case), case
    groups = {b: _budget(b, 1, 0, 0, 0)[1:3] for b in (64, 65, 16384, 16385)}
    assert groups == {64: [1, 1], 65: [2, 1], 16384: [256, 1], 16385: [257, 2]}
    from iceberg_tracking_code_amd import _lib
    out = (C.c_uint32 * 8)()
    lib = _lib.load()
    assert lib.icelk_jpeg_enc_budget(78, 0, 0, 0, 0, out) == _lib.EARG and lib.icelk_jpeg_enc_budget(78, 417, 0, 0, 0, out) == _lib.EARG
    assert lib.icelk_jpeg_enc_budget(2587400, 1, 0, 0, 0, out) == _lib.ECAP     # blocks * 1660 >= 2^32


def _walk(j, bpb, force=None, mask=0, capacity=1 << 20):
    from iceberg_tracking_code_amd import _lib
    n, report = C.c_uint64(123), (C.c_uint32 * 8)()
    buf = np.full(capacity, 0xAA, np.uint8)
    f = (C.c_uint32 * 3)(*force) if force is not None else None
    rc_ = _lib.load().icelk_jpeg_encode_budgeted_host(C.byref(j.info), j.coef_ptr, bpb, f, mask, b"a comment", 9, C.c_void_p(buf.ctypes.data),
                                                      capacity, C.byref(n), report)
    keys = ("cap", "bits", "invalid", "ff", "verdict", "stuffed", "packed_stores", "out_stores")
    return rc_, n.value, buf, dict(zip(keys, report))


@pytest.mark.parametrize("kind,quality,size", [("stripes", 95, (200, 9)), ("noise", 100, (176, 16)), ("noise", 1, (41, 7)), ("zeros", 100, (3, 3)),
                                               ("smooth", 75, (99, 131)), ("full", 100, (250, 333))])
def test_budgeted_walk_equals_the_host_writer_or_writes_nothing(kind, quality, size):
    from iceberg_tracking_code_amd import _lib, encode_jpeg, resave_coefficients
    from iceberg_tracking_code_amd.jpeg import encode_header
    w, h = size
    j = resave_coefficients(rc.content(kind, w, h, seed=7), quality)
    want = encode_jpeg(j, comment=b"a comment")
    scan = want[len(encode_header(j.info, b"a comment")):-2]
    S, ff = len(scan), scan.count(b"\xff\x00")
    blocks = 6 * j.info.mcus_x * j.info.mcus_y
    fit = -(-S // blocks)
    for bpb in sorted({fit, min(fit + 1, 416), 48, 416}):
        if blocks * bpb < S:
            continue
        code, n, buf, r = _walk(j, bpb)
        assert code == _lib.OK and buf[:n].tobytes() == want and (buf[n:] == 0xAA).all(), (bpb, r)
        assert r == dict(cap=blocks * bpb, bits=r["bits"], invalid=0, ff=ff, verdict=CODED, stuffed=S, packed_stores=S - ff, out_stores=S), (bpb, r)
        assert -(-r["bits"] // 8) == S - ff
    for bpb in range(max(1, fit - 3), fit):
        if blocks * bpb >= S:
            continue
        code, n, buf, r = _walk(j, bpb)
        assert code == _lib.OK and n == 0 and (buf == 0xAA).all(), (bpb, r)       # over budget: nothing is written
        assert r["verdict"] == OVER and r["stuffed"] == 0 and r["out_stores"] == 0, (bpb, r)
        assert (r["packed_stores"] != 0) == (blocks * bpb >= S - ff), (bpb, r)    # the exit behind the FF count, or the one in front of pack
    # a buffer too small: the length, nothing written
    code, n, buf, r = _walk(j, fit, capacity=len(want) - 1)
    assert code == _lib.ECAP and n == len(want) and (buf == 0xAA).all()
    # forced control words: the verdict follows the words, and what is coded is inside the capacity
    for force, mask in (((0, 1, 0), 2), ((8 * blocks * fit + 1, 0, 0), 1), ((0, 0, blocks * fit), 4), ((0xFFFFFFFF, 1, 0xFFFFFFFF), 7)):
        code, n, buf, r = _walk(j, fit, force, mask)
        assert code == _lib.OK and n == 0 and (buf == 0xAA).all() and r["verdict"] in (OVER, INVALID), (force, mask, r)
        assert r["out_stores"] == 0


def test_fixture_of_the_exit_behind_the_ff_count():
    """stripes at quality 95 on 200 x 9: 78 blocks, 980 packed and 1026 stuffed bytes, so 13 bytes per block (1014) hold the
    packed scan and not the stuffed one"""
    from iceberg_tracking_code_amd import resave_coefficients
    j = resave_coefficients(rc.content("stripes", 200, 9, seed=7), 95)
    assert 6 * j.info.mcus_x * j.info.mcus_y == 78
    _, n13, _, r13 = _walk(j, 13)
    _, n14, _, r14 = _walk(j, 14)
    assert (-(-r13["bits"] // 8), r13["ff"]) == (980, 46) and r13["verdict"] == OVER and r13["packed_stores"] == 980 and n13 == 0
    assert r14["verdict"] == CODED and r14["stuffed"] == 1026 and n14 > 1026


def test_driver_before_the_device(tmp_path):
    from iceberg_tracking_code_amd import crop_image_sequence
    assert crop_image_sequence([], str(tmp_path / "never")) == []
    assert not os.path.exists(str(tmp_path / "never"))
    names = [str(tmp_path / "20190801-120000.jpg")]         # not there: nothing may get as far as reading it
    for kw in (dict(quality=0), dict(quality=101), dict(quality="best"), dict(quality=None), dict(quality=75.5), dict(in_flight=0),
               dict(in_flight=-1), dict(read_threads=0), dict(write_threads=0)):
        with pytest.raises(ValueError):
            crop_image_sequence(names, str(tmp_path / "never"), crop=rc.CROP, **kw)
    assert not os.path.exists(str(tmp_path / "never"))


@pytest.mark.parametrize("progressive", [False, True])
def test_pil_route_on_a_truncated_photo(tmp_path, progressive):
    from iceberg_tracking_code_amd.crop import pil_crop_file
    src, dst = str(tmp_path / "20190801-120000.jpg"), str(tmp_path / "cropped.jpg")
    f = io.BytesIO()
    Image.fromarray(rc.content("smooth", 131, 99, seed=3)).save(f, "JPEG", quality=90, progressive=progressive, comment=b"camera 7")
    data = f.getvalue()
    with open(src, "wb") as g:
        g.write(data[:len(data) * 2 // 3])
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    with pytest.raises(OSError):
        rc.reference_crop_resave(src, dst, rc.CROP)          # Pillow refuses it as truncated
    ImageFile.LOAD_TRUNCATED_IMAGES = True                   # camtools.py:95-102
    try:
        rc.reference_crop_resave(src, dst, rc.CROP)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = False
    with open(dst, "rb") as g:
        want = g.read()
    got = pil_crop_file(src, rc.CROP, 75)
    assert got == want
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False          # set for that load only
    # a whole photo takes the first load, and the same function
    with open(src, "wb") as g:
        g.write(data)
    rc.reference_crop_resave(src, dst, rc.CROP)
    with open(dst, "rb") as g:
        assert pil_crop_file(src, rc.CROP, 75) == g.read()

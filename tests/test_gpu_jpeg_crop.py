"""GPU: the crop stage on its own (csrc/abi_jpeg_crop.hip on csrc/abi_jpeg_job.hip, the device-sized kernels of csrc/k_jpeg_enc.hip,
iceberg_tracking_code_amd/crop.py) against the file the reference's crop step writes (camtools.py:64-104, Pillow's
`Image.open(p).crop(box).save(out)`), against the synchronous calls on the same bytes, and -- the two-pass route --
against the one-pass folder driver.  Every comparison is equality of bytes or arrays.

Source photos are Pillow files with a comment and `CROP` margins around the crop that a case names.  Where a case names
the content of the crop (C3), the source is written at quality 100 without chroma subsampling, so that the crop the job
decodes is that content to within a few grey levels; the stream sizes the budget is set by are recomputed from the host's
bytes of the decoded crop, never taken from a table."""
import ctypes as C
import datetime as dt
import io
import os
import threading

import numpy as np
import pytest
from PIL import Image

import jpeg_resave_cases as rc

pytestmark = pytest.mark.gpu

CROP = rc.CROP
COMMENT = b"camera 7"


def _first_difference(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d" % (len(a), len(b), k)


def _photo(kind, w, h, seed=7, quality=90, subsampling=2, crop=CROP):
    """(the bytes of a photo whose crop is w x h, the file of the reference's crop step for it, the decoded crop)"""
    left, top, right, bottom = crop
    full = rc.content("smooth", w + left + right, h + top + bottom, seed)
    if kind != "smooth":
        full[top:top + h, left:left + w] = rc.content(kind, w, h, seed)
    f = io.BytesIO()
    Image.fromarray(full).save(f, "JPEG", quality=quality, subsampling=subsampling, comment=COMMENT)
    img = Image.open(io.BytesIO(f.getvalue()))
    width, height = img.size
    img_crop = img.crop((left, top, width - right, height - bottom))      # crop_image_standalone, call for call
    g = io.BytesIO()
    img_crop.save(g, "JPEG")
    return f.getvalue(), g.getvalue(), np.array(img_crop)


def _job(ctx, data, quality="reference", crop=CROP, comment=COMMENT):
    return ctx.jpeg_crop_finish(ctx.jpeg_crop_start(data, crop, quality), comment)


@pytest.fixture(scope="module")
def small():
    """a handle of its own, smaller than every photo here: max_w x max_h of icelk_create bound neither photo nor crop"""
    from iceberg_tracking_code_amd import Context
    c = Context(64, 64, n_slots=2, max_pts=64)
    yield c
    c.close()


@pytest.fixture()
def cctx(small):
    small.jpeg_crop_config()
    small.jpeg_huff_config()
    yield small
    small.jpeg_crop_config()
    small.jpeg_huff_config()


# ---- C1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", [2, 1, 0], ids=["420", "422", "444"])
@pytest.mark.parametrize("size", [(3, 3), (200, 9), (176, 16), (640, 480)], ids=lambda s: "%dx%d" % s)
def test_c1_one_file_against_the_references_file(ctx, cctx, tmp_path, size, subsampling):
    from iceberg_tracking_code_amd import source_comment
    w, h = size
    data, _, _ = _photo("smooth", w, h, subsampling=subsampling)
    src, dst = str(tmp_path / "20190801-120000.jpg"), str(tmp_path / "cropped.jpg")
    with open(src, "wb") as f:
        f.write(data)
    rc.reference_crop_resave(src, dst, CROP)
    with open(dst, "rb") as f:
        want = f.read()
    comment = source_comment(data)
    assert comment == COMMENT
    got, stats = _job(cctx, data, comment=comment)
    assert got == want, (size, subsampling, _first_difference(got, want))
    assert stats["route"] == "device" and stats["fallback"] == 0 and stats["stream_len"] <= stats["budget"] == 48 * stats["blocks"], stats
    assert stats["blocks"] == {(3, 3): 6, (200, 9): 78, (176, 16): 66, (640, 480): 7200}[size]
    ctx.upload_jpeg_file(0, data, 4, CROP, resave="reference")
    assert ctx.jpeg_resave_file(comment) == got
    assert _job(cctx, data, comment=None)[0] == got[:20] + got[20 + 4 + len(comment):]      # no comment: no COM segment


# ---- C2 ---------------------------------------------------------------------------------------------------------------
def test_c2_second_scan_past_one_pass(cctx):
    """528 x 5296: 65 538 blocks; at 416 bytes per block the capacity is 1665 workgroups of 16 KiB, more than the 1024
    entries the prefix sum takes per pass"""
    cctx.jpeg_crop_config(416)
    data, want, _ = _photo("smooth", 528, 5296)
    got, stats = _job(cctx, data, 75)
    chunks = -(-stats["budget"] // 64)
    assert stats["blocks"] == 65538 and stats["budget"] == 65538 * 416 and -(-chunks // 256) == 1665 > 1024
    assert got == want, _first_difference(got, want)
    assert stats["route"] == "device", stats


# ---- C3 ---------------------------------------------------------------------------------------------------------------
def _sizes(rgb, quality):
    """(blocks, packed bytes, stuffed bytes) of the re-saved crop's scan, from the host's file"""
    from iceberg_tracking_code_amd import resave_bytes, resave_coefficients
    from iceberg_tracking_code_amd.jpeg import encode_header
    info = resave_coefficients(rgb, quality).info
    scan = resave_bytes(rgb, quality)[len(encode_header(info)):-2]
    return 6 * info.mcus_x * info.mcus_y, len(scan) - scan.count(b"\xff\x00"), len(scan)


C3_CASES = [("noise", 100, (176, 16), "over-budget"), ("noise", 100, (640, 480), "over-budget"), ("noise", 75, (640, 480), "device"),
            ("stripes", 95, (640, 480), "device"), ("noise", 1, (176, 16), "device"), ("zeros", 100, (176, 16), "device")]


@pytest.mark.parametrize("kind,quality,size,route", C3_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_c3_budget_at_48_bytes_per_block_and_its_exact_edge(cctx, kind, quality, size, route):
    w, h = size
    data, _, rgb = _photo(kind, w, h, quality=100, subsampling=0)
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, "JPEG", quality=quality, comment=COMMENT)
    want = f.getvalue()
    blocks, P, S = _sizes(rgb, quality)
    print("%s quality %d %dx%d: %d blocks, packed %d, stuffed %d, %.1f bytes per block" % (kind, quality, w, h, blocks, P, S, S / blocks))
    assert (S > 48 * blocks) == (route == "over-budget")         # the table of the issue, recomputed for the decoded crop
    got, stats = _job(cctx, data, quality)
    assert got == want, (kind, quality, size, _first_difference(got, want))
    assert stats["route"] == route and stats["stream_len"] == S and stats["blocks"] == blocks and stats["budget"] == 48 * blocks, stats
    fit = -(-S // blocks)
    cctx.jpeg_crop_config(fit)
    got, stats = _job(cctx, data, quality)
    assert got == want and stats["route"] == "device" and stats["budget"] == fit * blocks >= S, stats
    if fit - 1 >= 1 and (fit - 1) * blocks < S:
        cctx.jpeg_crop_config(fit - 1)
        got, stats = _job(cctx, data, quality)
        assert got == want and stats["route"] == "over-budget" and stats["stream_len"] == S, stats


def test_c3_the_exit_behind_the_ff_count(cctx):
    """stripes at quality 95 on 200 x 9: the packed scan fits 13 bytes per block and the stuffed one does not"""
    data, _, rgb = _photo("stripes", 200, 9, quality=100, subsampling=0)
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, "JPEG", quality=95, comment=COMMENT)
    want = f.getvalue()
    blocks, P, S = _sizes(rgb, 95)
    print("blocks %d, packed %d, stuffed %d" % (blocks, P, S))
    assert blocks == 78 and P <= 13 * blocks < S <= 14 * blocks, (blocks, P, S)     # 1014 and 1092 bracket them
    cctx.jpeg_crop_config(13)
    got, stats = _job(cctx, data, 95)
    assert got == want and stats["route"] == "over-budget" and stats["budget"] == 1014, stats
    cctx.jpeg_crop_config(14)
    got, stats = _job(cctx, data, 95)
    assert got == want and stats["route"] == "device" and stats["stream_len"] == S and stats["budget"] == 1092, stats


# ---- C4 ---------------------------------------------------------------------------------------------------------------
def test_c4_decoder_fallback_inside_a_crop_job(cctx):
    data, want, _ = _photo("smooth", 640, 480)
    cctx.jpeg_huff_config(32, 1, 1)                              # a chain of one hop is at the bound: no file meets it
    t = cctx.jpeg_crop_start(data, CROP)
    cctx.jpeg_huff_config()
    t2 = cctx.jpeg_crop_start(data, CROP)                        # under the default bound again
    got, stats = cctx.jpeg_crop_finish(t, COMMENT)
    assert got == want, _first_difference(got, want)
    assert stats["route"] == "host-huffman" and stats["fallback"] != 0, stats
    got, stats = cctx.jpeg_crop_finish(t2, COMMENT)
    assert got == want and stats["route"] == "device" and stats["fallback"] == 0, stats


# ---- C5 ---------------------------------------------------------------------------------------------------------------
def test_c5_several_in_flight(cctx):
    sizes = ((99, 131), (640, 480), (3, 3), (640, 480), (200, 9), (99, 131))
    photos = [_photo("smooth", w, h, seed=11 + k) for k, (w, h) in enumerate(sizes)]
    runs = []
    for _ in range(2):
        tickets = [cctx.jpeg_crop_start(data, CROP) for data, _, _ in photos]
        assert len(set(tickets)) == 6
        got = {}
        for k in reversed(range(6)):
            got[k], stats = cctx.jpeg_crop_finish(tickets[k], COMMENT)
            assert stats["route"] == "device", (k, stats)
            assert got[k] == photos[k][1], (k, _first_difference(got[k], photos[k][1]))
        runs.append(got)
    assert runs[0] == runs[1]
    cctx.sync()


# ---- C6 ---------------------------------------------------------------------------------------------------------------
def test_c6_errors(cctx):
    from iceberg_tracking_code_amd import Context, IcelkError, _lib
    data, want, _ = _photo("smooth", 99, 131)
    lib, h = cctx._lib, cctx._h
    n, st = C.c_uint64(0), _lib.JpegCropStats()
    buf = np.full(len(want) + 16, 0xAA, np.uint8)
    finish = lambda ticket, cap: lib.icelk_jpeg_crop_finish(h, ticket, COMMENT, len(COMMENT), C.c_void_p(buf.ctypes.data), cap, C.byref(n), C.byref(st))
    t = cctx.jpeg_crop_start(data, CROP)
    assert finish(t, len(want) - 1) == _lib.ECAP and n.value == len(want) and (buf == 0xAA).all()
    assert finish(t, 0) == _lib.ECAP and n.value == len(want) and (buf == 0xAA).all()
    assert cctx.jpeg_crop_poll(t) == 1                           # the ticket stays valid
    assert finish(t, buf.size) == _lib.OK and n.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
    assert st.route == 0 and st.stream_len > 0
    assert finish(t, buf.size) == _lib.ESTATE                    # finished
    assert finish(t + 1000, buf.size) == _lib.ESTATE and finish(0, buf.size) == _lib.ESTATE and finish(-1, buf.size) == _lib.ESTATE
    with pytest.raises(IcelkError) as e:
        cctx.jpeg_crop_finish(t)
    assert e.value.code == _lib.ESTATE
    with pytest.raises(IcelkError):
        cctx.jpeg_crop_poll(t)
    t = cctx.jpeg_crop_start(data, CROP)
    cctx.jpeg_crop_cancel(t)
    assert finish(t, buf.size) == _lib.ESTATE
    with pytest.raises(IcelkError):
        cctx.jpeg_crop_cancel(t)
    # a crop narrower than 3: refused at start, and no ticket is taken -- the next one is the next number
    before = cctx.jpeg_crop_start(data, CROP)
    for bad in ((53, 5, 53, 7), (0, 0, 200, 0), (-1, 0, 0, 0)):  # 2 pixels wide; no image; a negative margin
        with pytest.raises(ValueError):
            cctx.jpeg_crop_start(data, bad)
    for quality in (0, 101):
        with pytest.raises(ValueError):
            cctx.jpeg_crop_start(data, CROP, quality)
    with pytest.raises(ValueError):
        cctx.jpeg_crop_start(b"not a JPEG file", CROP)
    with pytest.raises(ValueError):
        cctx.jpeg_crop_config(0)
    with pytest.raises(ValueError):
        cctx.jpeg_crop_config(417)
    after = cctx.jpeg_crop_start(data, CROP)
    assert after == before + 1
    assert cctx.jpeg_crop_finish(after, COMMENT)[0] == want and cctx.jpeg_crop_finish(before, COMMENT)[0] == want
    # a handle destroyed with tickets in flight does not hang
    big = _photo("smooth", 640, 480)[0]
    c = Context(64, 64, n_slots=2, max_pts=64)
    for _ in range(3):
        c.jpeg_crop_start(big, CROP)
    closer = threading.Thread(target=c.close, daemon=True)
    closer.start()
    closer.join(20.0)
    assert not closer.is_alive(), "icelk_destroy hangs with crop jobs in flight"


# ---- C7: the driver and the two-pass route ---------------------------------------------------------------------------------
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
    """the folder of test_gpu_jpeg_encode.py: 7 photos of 320 x 240 -- one saved progressive (it goes through PIL), two with
    a comment, the progressive one among them -- and the files the reference's crop step writes for them"""
    d = tmp_path_factory.mktemp("cropfolder")
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


def test_c7_driver_and_two_pass_route(folder):
    from iceberg_tracking_code_amd import crop_image_sequence
    d = folder["dir"]
    target = str(d / "target")
    done = crop_image_sequence(folder["names"], target, crop=FOLDER_CROP, in_flight=3)
    assert sorted(os.listdir(target)) == sorted(folder["cropped"])
    assert [os.path.basename(p) for p, _, _ in done] == [os.path.basename(p) for p in folder["names"]]
    for k, (path, nbytes, route) in enumerate(done):
        with open(path, "rb") as f:
            mine = f.read()
        want = folder["cropped"][os.path.basename(path)]
        assert mine == want, (path, _first_difference(mine, want))
        assert nbytes == len(want) and route == ("pil" if k == 3 else "device"), (k, route)
    cropped = [p for p, _, _ in done]
    got = _track(cropped, str(d / "out_two_pass"), decoder="device", huffman="device", pipeline=True)
    want = _track(folder["names"], str(d / "out_one_pass"), crop=FOLDER_CROP, resave="reference", decoder="device", huffman="device")
    assert len(got) == len(want) >= 3
    for (pg, tg, qg), (pw, tw, qw) in zip(got, want):
        assert os.path.basename(pg) == os.path.basename(pw) and len(tw) > 10
        assert np.array_equal(tg, tw) and np.array_equal(qg, qw)

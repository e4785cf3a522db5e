"""GPU: the slot-bound re-save job (csrc/abi_jpeg_async.hip on csrc/abi_jpeg_job.hip: icelk_upload_jpeg_file_async_resave, icelk_jpeg_async_finish,
icelk_jpeg_async_finish_file) -- one enqueued job per photo that leaves the slot the frame the reference tracks on and,
when asked, the crop file it would have written.  The slot is compared with the synchronous `upload_jpeg_file(resave=)`
and with `upload_bgr` of Pillow's reopened crop, the file with the bytes of Pillow's `Image.open(f).crop(box).save(out)`.
Every comparison is equality."""
import ctypes as C
import io
import threading
import time

import numpy as np
import pytest
from PIL import Image

import jpeg_resave_cases as rc
import jpeg_streams as js

pytestmark = pytest.mark.gpu

CROP = rc.CROP
COMMENT = b"camera 7"
DEADLINE = 20.0


def _first_difference(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d" % (len(a), len(b), k)


def _reference(data, crop=CROP, quality=None):
    """(the file of the reference's crop step for `data`, the pixels of that file reopened)"""
    left, top, right, bottom = crop
    img = Image.open(io.BytesIO(data))
    width, height = img.size
    img_crop = img.crop((left, top, width - right, height - bottom))
    g = io.BytesIO()
    kw = {} if quality is None else dict(quality=quality)
    img_crop.save(g, "JPEG", **kw)                                   # crop_image_standalone (camtools.py:64-104), call for call
    return g.getvalue(), np.array(Image.open(io.BytesIO(g.getvalue())))


def _photo(kind, w, h, seed=7, quality=90, subsampling=2, crop=CROP, comment=COMMENT):
    """the bytes of a photo whose crop is w x h"""
    left, top, right, bottom = crop
    full = rc.content("smooth", w + left + right, h + top + bottom, seed)
    if kind != "smooth":
        full[top:top + h, left:left + w] = rc.content(kind, w, h, seed)
    f = io.BytesIO()
    kw = dict(comment=comment) if comment else {}
    Image.fromarray(full).save(f, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return f.getvalue()


def _poll_until_there(ctx, slot):
    t0 = time.monotonic()
    while True:
        state = ctx.jpeg_async_poll(slot)
        if state != 0:
            return state
        assert time.monotonic() - t0 < DEADLINE, "no verdict within %g s" % DEADLINE


@pytest.fixture()
def hctx(ctx):
    ctx.jpeg_huff_config()
    ctx.jpeg_crop_config()
    yield ctx
    ctx.jpeg_huff_config()
    ctx.jpeg_crop_config()


# ---- J1: the slot ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("size", [(3, 3), (176, 16), (314, 235)], ids=lambda s: "%dx%d" % s)
def test_j1_slot(hctx, size, variant):
    w, h = size
    data = _photo("smooth", w, h)
    _, reopened = _reference(data)
    hctx.upload_bgr(1, reopened, variant)
    want = hctx.download_level(1, 0)
    hctx.upload_jpeg_file(2, data, variant, CROP, resave="reference")
    sync = hctx.download_level(2, 0)
    for crop_file in (False, True):
        hctx.upload_jpeg_file_async(0, data, variant, CROP, resave="reference", crop_file=crop_file)
        assert _poll_until_there(hctx, 0) == 1
        st = hctx.jpeg_async_finish(0)
        assert st["fallback"] == 0 and hctx.jpeg_async_poll(0) == 1
        got = hctx.download_level(0, 0)
        assert got.shape == want.shape == (h, w)
        assert np.array_equal(got, sync), (crop_file, int(np.count_nonzero(got != sync)))
        assert np.array_equal(got, want), (crop_file, int(np.count_nonzero(got != want)))
    hctx.upload_jpeg_file_async(0, data, variant, CROP)              # the option matters
    hctx.jpeg_async_finish(0)
    if size != (3, 3):
        assert not np.array_equal(hctx.download_level(0, 0), want)


# ---- J2: the file ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", [2, 0], ids=["420", "444"])
@pytest.mark.parametrize("size", [(3, 3), (176, 16), (314, 235)], ids=lambda s: "%dx%d" % s)
def test_j2_file(hctx, size, subsampling):
    from iceberg_tracking_code_amd import source_comment
    w, h = size
    data = _photo("smooth", w, h, subsampling=subsampling)
    want, reopened = _reference(data)
    comment = source_comment(data)
    assert comment == COMMENT
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=True)
    got, stats = hctx.jpeg_async_finish_file(0, comment)
    assert got == want, (size, _first_difference(got, want))
    assert stats["route"] == "device" and stats["fallback"] == 0 and stats["stream_len"] <= stats["budget"] == 48 * stats["blocks"], stats
    hctx.upload_bgr(1, reopened, 4)
    assert np.array_equal(hctx.download_level(0, 0), hctx.download_level(1, 0))
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=True)
    bare, _ = hctx.jpeg_async_finish_file(0, None)
    assert bare == got[:20] + got[20 + 4 + len(comment):]           # no comment: no COM segment
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave=50, crop_file=True)
    assert hctx.jpeg_async_finish_file(0, comment)[0] == _reference(data, quality=50)[0]


def test_j2_ecap_and_repeat(hctx):
    from iceberg_tracking_code_amd import IcelkError, _lib
    data = _photo("smooth", 99, 131)
    want, reopened = _reference(data)
    lib, h = hctx._lib, hctx._h
    n, st = C.c_uint64(0), _lib.JpegCropStats()
    buf = np.full(len(want) + 16, 0xAA, np.uint8)
    finish = lambda slot, cap: lib.icelk_jpeg_async_finish_file(h, slot, COMMENT, len(COMMENT), C.c_void_p(buf.ctypes.data), cap, C.byref(n), C.byref(st))
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=True)
    assert finish(0, len(want) - 1) == _lib.ECAP and n.value == len(want) and (buf == 0xAA).all()
    assert finish(0, 0) == _lib.ECAP and n.value == len(want)
    assert hctx.jpeg_async_poll(0) == 1                             # the job stays with its slot, the frame is there
    with pytest.raises(IcelkError, match="-5"):                       # ICELK_ESTATE
        hctx.upload_jpeg_file_async(0, data, 4, CROP)
    assert finish(0, buf.size) == _lib.OK and buf[:n.value].tobytes() == want and (buf[len(want):] == 0xAA).all()
    assert st.route == 0 and st.stream_len > 0
    assert finish(0, buf.size) == _lib.ESTATE                        # released
    hctx.upload_bgr(1, reopened, 4)
    assert np.array_equal(hctx.download_level(0, 0), hctx.download_level(1, 0))
    # after ICELK_ECAP the plain finish drops the file; a job without a file has none to give
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=True)
    assert finish(0, 0) == _lib.ECAP
    assert hctx.jpeg_async_finish(0)["fallback"] == 0
    assert np.array_equal(hctx.download_level(0, 0), hctx.download_level(1, 0))
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference")
    assert finish(0, buf.size) == _lib.ESTATE
    hctx.jpeg_async_finish(0)
    with pytest.raises(ValueError):
        hctx.upload_jpeg_file_async(0, data, 4, CROP, crop_file=True)
    for bad in ((53, 5, 53, 7), (0, 0, 200, 0)):                     # 2 pixels wide; no image
        with pytest.raises(ValueError):
            hctx.upload_jpeg_file_async(0, data, 4, bad, resave="reference")
    with pytest.raises(ValueError):
        hctx.upload_jpeg_file_async(0, data, 4, CROP, resave=101)
    hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference")    # none of them took the slot
    hctx.jpeg_async_finish(0)


# ---- J3: the decoder's fallback inside the job -----------------------------------------------------------------------------
def test_j3_decoder_fallback(hctx):
    photo = _photo("smooth", 314, 235)
    flat = js.stream("flat black 420 531x397").data
    for label, data in (("photo", photo), ("flat", flat)):
        want, reopened = _reference(data)
        hctx.upload_bgr(1, reopened, 4)
        px = hctx.download_level(1, 0)
        hctx.jpeg_huff_config(32, 1, 1)                              # a chain of one hop is at the bound: no file meets it
        hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=True)
        hctx.jpeg_huff_config()
        assert _poll_until_there(hctx, 0) == 2
        got, stats = hctx.jpeg_async_finish_file(0, COMMENT if label == "photo" else None)
        assert got == want, (label, _first_difference(got, want))
        assert stats["route"] == "host-huffman" and stats["fallback"] != 0, stats
        assert hctx.jpeg_async_poll(0) == 2
        assert np.array_equal(hctx.download_level(0, 0), px), label
        # the plain finish on the same fallback: the pixels, no file
        hctx.jpeg_huff_config(32, 1, 1)
        hctx.upload_jpeg_file_async(0, data, 4, CROP, resave="reference", crop_file=(label == "flat"))
        hctx.jpeg_huff_config()
        assert hctx.jpeg_async_finish(0)["fallback"] != 0
        assert np.array_equal(hctx.download_level(0, 0), px), label


# ---- J4: the budget ------------------------------------------------------------------------------------------------------
def _sizes(rgb, quality):
    """(blocks, stuffed bytes) of the re-saved crop's scan, from the host's file"""
    from iceberg_tracking_code_amd import resave_bytes, resave_coefficients
    from iceberg_tracking_code_amd.jpeg import encode_header
    info = resave_coefficients(rgb, quality).info
    scan = resave_bytes(rgb, quality)[len(encode_header(info)):-2]
    return 6 * info.mcus_x * info.mcus_y, len(scan)


def test_j4_budget_exact_edge_and_one_below(hctx):
    data = _photo("noise", 176, 16, quality=100, subsampling=0)
    left, top, right, bottom = CROP
    img = Image.open(io.BytesIO(data))
    rgb = np.array(img.crop((left, top, img.size[0] - right, img.size[1] - bottom)))
    want = _reference(data, quality=100)[0]
    blocks, S = _sizes(rgb, 100)
    fit = -(-S // blocks)
    print("blocks %d, stuffed %d, %d bytes per block fit" % (blocks, S, fit))
    assert fit > 48 and (fit - 1) * blocks < S <= fit * blocks
    hctx.upload_jpeg_file(1, data, 4, CROP, resave=100)
    px = hctx.download_level(1, 0)
    for per_block, route in ((48, "over-budget"), (fit, "device"), (fit - 1, "over-budget")):
        hctx.jpeg_crop_config(per_block)
        hctx.upload_jpeg_file_async(0, data, 4, CROP, resave=100, crop_file=True)
        assert _poll_until_there(hctx, 0) == 1                       # the frame is usable: the budget concerns only the file
        got, stats = hctx.jpeg_async_finish_file(0, COMMENT)
        assert got == want, (per_block, _first_difference(got, want))
        assert stats["route"] == route and stats["stream_len"] == S and stats["budget"] == per_block * blocks, (per_block, stats)
        assert np.array_equal(hctx.download_level(0, 0), px)


# ---- J5: several in flight, beside the tracker ---------------------------------------------------------------------------
def test_j5_four_jobs_in_six_slots_beside_tracker_steps(synth):
    from iceberg_tracking_code_amd import Context
    sizes = ((99, 131), (314, 235), (3, 3), (200, 9))
    photos = [_photo("smooth", w, h, seed=11 + k) for k, (w, h) in enumerate(sizes)]
    refs = [_reference(d) for d in photos]
    grays, _ = synth.sequence(320, 240, 2, seed=5, max_step_px=2.0)
    with Context(1024, 768, n_slots=6, max_pts=1 << 12) as ctx:
        want_px = []
        for d, (_, reopened) in zip(photos, refs):
            ctx.upload_bgr(4, reopened, 4)
            want_px.append(ctx.download_level(4, 0))
        ctx.upload_gray(4, grays[0])
        ctx.upload_gray(5, grays[1])
        pts = ctx.good_features(4, 200, 0.01, 8)
        assert len(pts) > 20
        tracked = ctx.track_fb(4, 5, pts)
        runs = []
        for rnd in range(2):
            with_file = [(k + rnd) % 2 == 0 for k in range(4)]
            for k in range(4):
                ctx.upload_jpeg_file_async(k, photos[k], 4, CROP, resave="reference", crop_file=with_file[k])
            files = {}
            for k in range(4):
                again = ctx.track_fb(4, 5, pts)                       # a tracker step between the finishes
                assert all(np.array_equal(again[key], tracked[key]) for key in tracked)
                if with_file[k]:
                    files[k], stats = ctx.jpeg_async_finish_file(k, COMMENT)
                    assert stats["route"] == "device", (k, stats)
                    assert files[k] == refs[k][0], (rnd, k, _first_difference(files[k], refs[k][0]))
                else:
                    assert ctx.jpeg_async_finish(k)["fallback"] == 0
                got = ctx.download_level(k, 0)
                assert got.shape == want_px[k].shape and np.array_equal(got, want_px[k]), (rnd, k)
            runs.append(files)
        assert set(runs[0]) == {0, 2} and set(runs[1]) == {1, 3}
        ctx.sync()


# ---- J6: errors and teardown ---------------------------------------------------------------------------------------------
def test_j6_busy_slot_and_teardown():
    from iceberg_tracking_code_amd import Context, IcelkError
    big = _photo("smooth", 640, 480)
    c = Context(1024, 768, n_slots=3, max_pts=64)
    c.upload_jpeg_file_async(0, big, 4, CROP, resave="reference", crop_file=True)
    for kw in (dict(), dict(resave="reference"), dict(resave="reference", crop_file=True)):
        with pytest.raises(IcelkError, match="-5"):                   # ICELK_ESTATE
            c.upload_jpeg_file_async(0, big, 4, CROP, **kw)
    c.upload_jpeg_file_async(1, big, 4, CROP, resave="reference")
    c.upload_jpeg_file_async(2, big, 4, CROP, resave="reference", crop_file=True)
    c.sync()                                                          # the decode streams count; the jobs stay their slots'
    assert c.jpeg_async_poll(0) == 1
    closer = threading.Thread(target=c.close, daemon=True)
    closer.start()
    closer.join(20.0)
    assert not closer.is_alive(), "icelk_destroy hangs with re-save jobs in flight"

"""GPU: the hand-written streams of jpeg_streams.py through the device decoder (k_jpeg_huff.hip, k_jpeg.hip):
coefficients against the Python reader, the synchronisation statistics against the CPU statement of the same algorithm
field for field, pixels against Pillow for the streams whose blocks an 8-bit encoder can produce, uploads into a slot,
the DC pass of long restart intervals block by block, state left over between files, flat frames under the default
work bound, and coefficients outside an encoder's range.  Every comparison is exact; no expected count of rounds or
fallbacks is written down here, the CPU statement says them."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_streams as js
import jpeg_writer as jw

pytestmark = pytest.mark.gpu

SUBSEQ = (32, 512, 1024)
GENEROUS = dict(max_hops=256, max_rounds=255)
DEFAULT = dict(max_hops=256, max_rounds=8)
DECODED = [e for e in js.ENTRIES if e != "out-of-range"]


@pytest.fixture()
def hctx(ctx):
    """the session's context with the decoder's defaults, whatever a test sets"""
    ctx.jpeg_huff_config()
    yield ctx
    ctx.jpeg_huff_config()


def _streams(entry):
    return [s for s in js.catalogue() if s.entry == entry]


def _check_coefficients(ctx, s, what=""):
    want = js.reference(s.label)[2]
    got = ctx.jpeg_device_coefficients(s.data)
    assert got.shape == want.shape, (s.label, what, got.shape, want.shape)
    assert np.array_equal(got, want), (s.label, what, int(np.count_nonzero(got != want)), int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("entry", DECODED)
def test_coefficients_and_statistics(hctx, entry):
    from iceberg_tracking_code_amd import read_jpeg_lanes
    streams = _streams(entry)
    assert streams
    for s in streams:
        for S in SUBSEQ:
            for name, bounds in (("generous", GENEROUS), ("default", DEFAULT)):
                hctx.jpeg_huff_config(S, **bounds)
                _check_coefficients(hctx, s, (S, name))
                got = hctx.jpeg_huff_stats()
                _, want = read_jpeg_lanes(s.data, S, **bounds)
                print("%s S=%d %s: %s" % (s.label, S, name, got))
                assert got == want, (s.label, S, name, got, want)
                assert got["segments"] == s.segments, (s.label, got)
                if bounds is GENEROUS:
                    assert got["fallback"] == 0, (s.label, S, got)


@pytest.mark.parametrize("entry", DECODED)
def test_pixels_equal_pillow(hctx, entry):
    from iceberg_tracking_code_amd import decode_jpeg
    for s in _streams(entry):
        if s.tier != "pixels":
            continue
        want = js.pillow(s.label)
        for huffman in ("host", "device"):
            got = decode_jpeg(s.data, ctx=hctx, huffman=huffman)
            assert got.shape == want.shape and got.dtype == np.uint8, (s.label, huffman)
            assert np.array_equal(got, want), (s.label, huffman, int(np.count_nonzero(got != want)))


UPLOADS = ("big-interval b 444 528x512", "slots crossed 420 48x32", "slots four-defined 420 48x32", "ri-1 420 256x256",
           "flat black 420 531x397")


@pytest.mark.parametrize("crop", [None, (5, 3, 7, 2)])
def test_upload_jpeg_file_equals_upload_bgr(hctx, crop):
    for label in UPLOADS:
        s = js.stream(label)
        for variant in (3, 4):
            hctx.upload_bgr(0, js.pillow(label), variant, crop)
            want = hctx.download_level(0, 0)
            hctx.upload_jpeg_file(1, s.data, variant, crop)
            got = hctx.download_level(1, 0)
            assert got.shape == want.shape, (label, got.shape, want.shape)
            assert np.array_equal(got, want), (label, variant, int(np.count_nonzero(got != want)))


@pytest.mark.parametrize("S", (512, 1024))
def test_dc_pass_of_long_intervals_block_by_block(hctx, S):
    """the DC kernels exist on the device only: a wrong chunk sum or carry shows as the first block, in scan order, whose
    DC differs, with its chunk"""
    hctx.jpeg_huff_config(S, **GENEROUS)
    for s in _streams("big-interval"):
        info, planes, _ = js.reference(s.label)
        got = hctx.jpeg_device_coefficients(s.data)
        assert hctx.jpeg_huff_stats()["fallback"] == 0, s.label        # the device's own DC pass made these values
        off, mine = 0, []
        for p in planes:
            mine.append(got[off:off + p.size].reshape(p.shape[0], p.shape[1], 64))
            off += p.size
        assert off == got.size
        ref = [p.reshape(p.shape[0], p.shape[1], 64) for p in planes]
        ri = info["restart_interval"]
        ri = ri if 0 < ri < info["mcus_x"] * info["mcus_y"] else info["mcus_x"] * info["mcus_y"]
        for (m, c, a, _), (_, _, b, _) in zip(jw.scan_order(mine, info["sampling"]), jw.scan_order(ref, info["sampling"])):
            assert a[0] == b[0], "%s S=%d: component %d, MCU %d (interval %d, chunk %d of it, pass %d of the scan loop): DC %d, " \
                "expected %d" % (s.label, S, c, m, m // ri, (m % ri) // js.DC_CHUNK, (m % ri) // js.DC_CHUNK // 256, a[0], b[0])
        for c, (a, b) in enumerate(zip(mine, ref)):
            assert np.array_equal(a, b), (s.label, c)


def test_state_left_between_files(hctx):
    """the lane, group and DC buffers grow and are never cleared: a large file, a file of many tiny segments, the large
    one again at another lane length, then a photo"""
    big, tiny = js.stream("big-interval a gray 1032x512"), js.stream("ri-1 420 256x256")
    photo = jc.encode(jc.photo(120, 88, 21), quality=85, subsampling=2)
    from iceberg_tracking_code_amd import read_jpeg
    for s, S in ((big, 32), (tiny, 1024), (big, 512)):
        hctx.jpeg_huff_config(S, **GENEROUS)
        _check_coefficients(hctx, s, S)
        assert hctx.jpeg_huff_stats()["fallback"] == 0, (s.label, S)
    hctx.jpeg_huff_config()
    got = hctx.jpeg_device_coefficients(photo)
    assert np.array_equal(got, read_jpeg(photo).coef)
    assert np.array_equal(hctx.jpeg_decode_rgb_file(photo), jc.pil_decode(photo))
    # and the other way round: the small files first leave short buffers behind
    hctx.jpeg_huff_config(1024, **GENEROUS)
    _check_coefficients(hctx, tiny, "again")
    _check_coefficients(hctx, js.stream("big-interval c 420 1056x1024 ri4100"), "after ri-1")


@pytest.mark.parametrize("S", (32, 512))
def test_flat_frames_under_the_default_bounds(hctx, S):
    from iceberg_tracking_code_amd import decode_jpeg, read_jpeg_lanes
    hctx.jpeg_huff_config(S, **DEFAULT)
    fallbacks = {}
    for s in _streams("flat"):
        got = decode_jpeg(s.data, ctx=hctx, huffman="device")
        st = hctx.jpeg_huff_stats()
        assert np.array_equal(got, js.pillow(s.label)), (s.label, S, st)
        _, want = read_jpeg_lanes(s.data, S, **DEFAULT)
        assert st["fallback"] == want["fallback"], (s.label, S, st, want)
        fallbacks[s.label] = st["fallback"]
    print("S=%d: %s" % (S, fallbacks))
    if S == 32:
        assert fallbacks["flat black 420 736x736"] == 1


def test_coefficients_outside_an_encoders_range(hctx):
    """nothing is said about these pixels (Pillow's own SIMD path departs from libjpeg's C code here); the decoder
    answers, answers the same twice, and goes on working"""
    from iceberg_tracking_code_amd import decode_jpeg
    good = js.stream("slots crossed 420 48x32")
    for s in _streams("out-of-range"):
        info = js.reference(s.label)[0]
        for huffman in ("host", "device"):
            a = decode_jpeg(s.data, ctx=hctx, huffman=huffman)
            b = decode_jpeg(s.data, ctx=hctx, huffman=huffman)
            assert a.shape == b.shape == (info["height"], info["width"], 3) and a.dtype == b.dtype == np.uint8, (s.label, huffman)
            assert np.array_equal(a, b), (s.label, huffman)
            assert np.array_equal(decode_jpeg(good.data, ctx=hctx, huffman=huffman), js.pillow(good.label)), (s.label, huffman)

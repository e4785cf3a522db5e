"""GPU: Huffman decoding of the JPEG scan on the device (k_jpeg_huff.hip behind icelk_jpeg_device_coefficients /
icelk_jpeg_decode_rgb_file / icelk_upload_jpeg_file): coefficients equal to the host decoder's, pixels equal to Pillow's,
restart intervals, the work bound's fallback, malformed files, and the folder driver with huffman="device"."""
import ctypes as C
import datetime as dt
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc

pytestmark = pytest.mark.gpu

BIG = (531, 397)    # 67 x 50 blocks: thousands of subsequences at 32 and 128 bits, several workgroups of lanes at all three
GENEROUS = dict(max_hops=256, max_rounds=255)


@pytest.fixture()
def hctx(ctx):
    """the session's context with the decoder's defaults, whatever a test sets"""
    ctx.jpeg_huff_config()
    yield ctx
    ctx.jpeg_huff_config()


@pytest.fixture(scope="module")
def big_files():
    out = {"photo s%d" % sub: jc.encode(jc.photo(*BIG, 21), quality=85, subsampling=sub) for sub in (0, 1, 2)}
    out["edges q100"] = jc.encode(jc.edges(*BIG), quality=100, subsampling=2)
    return out


def _equal_coefficients(ctx, label, data):
    from iceberg_tracking_code_amd import read_jpeg
    want = read_jpeg(data).coef
    got = ctx.jpeg_device_coefficients(data)
    assert got.shape == want.shape and np.array_equal(got, want), (label, int(np.count_nonzero(got != want)))


def test_coefficients_equal_host_decoder_on_the_matrix(hctx):
    cases = jc.matrix(min_width=3)
    assert len(cases) > 250
    for label, data in cases:
        _equal_coefficients(hctx, label, data)
        assert hctx.jpeg_huff_stats()["fallback"] == 0, label


@pytest.mark.parametrize("S", [32, 128, 1024])
def test_coefficients_across_workgroups_and_statistics(hctx, big_files, S):
    hctx.jpeg_huff_config(S, **GENEROUS)
    for label, data in big_files.items():
        _equal_coefficients(hctx, label, data)
        st = hctx.jpeg_huff_stats()
        assert st["fallback"] == 0 and st["segments"] == 1, (label, st)
        assert st["subsequences"] > 256 * (3 if S == 1024 else 20), (label, st)   # several workgroups of lanes
        if S == 128:
            assert st["subsequences"] - st["lanes_in_step"] > st["subsequences"] / 2, (label, st)
            assert st["max_hops"] >= 2 and st["total_hops"] >= st["max_hops"], (label, st)
        assert st["spanning_blocks"] >= 1, (label, st)
    if S == 32:
        blocks = hctx.jpeg_device_coefficients(big_files["edges q100"]).size // 64
        assert hctx.jpeg_huff_stats()["spanning_blocks"] > 0.9 * blocks


def test_statistics_equal_the_host_statement(hctx, big_files):
    """the device's counters against the same algorithm run lane by lane on the CPU"""
    from iceberg_tracking_code_amd import read_jpeg_lanes
    hctx.jpeg_huff_config(128, **GENEROUS)
    for label in ("photo s2", "edges q100"):
        hctx.jpeg_device_coefficients(big_files[label])
        got = hctx.jpeg_huff_stats()
        _, want = read_jpeg_lanes(big_files[label], 128, **GENEROUS)
        assert got == want, (label, got, want)


def test_pixels_equal_pillow(hctx, big_files):
    from iceberg_tracking_code_amd import decode_jpeg
    files = dict(big_files)
    files["gray"] = jc.encode(jc.photo(*BIG, 22, channels=1), quality=80)
    for label, data in files.items():
        want = jc.pil_decode(data)
        got = decode_jpeg(data, ctx=hctx, huffman="device")
        assert got.shape == want.shape and got.dtype == np.uint8, label
        assert np.array_equal(got, want), (label, int(np.count_nonzero(got != want)))


@pytest.mark.parametrize("crop", [None, (5, 3, 7, 2), (16, 16, 16, 16)])
def test_upload_jpeg_file_equals_upload_bgr(hctx, big_files, crop):
    for label in ("photo s0", "photo s1", "photo s2"):
        data = big_files[label]
        for variant in (3, 4):
            hctx.upload_bgr(0, jc.pil_decode(data), variant, crop)
            want = hctx.download_level(0, 0)
            hctx.upload_jpeg_file(1, data, variant, crop)
            got = hctx.download_level(1, 0)
            assert got.shape == want.shape, (label, got.shape, want.shape)
            assert np.array_equal(got, want), (label, variant, int(np.count_nonzero(got != want)))


def _segments(data):
    from iceberg_tracking_code_amd import _lib as L
    lib = L.load()
    info, scan = L.JpegInfo(), L.JpegScan()
    assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, None) == 0
    begin, end = (C.c_uint32 * scan.segments)(), (C.c_uint32 * scan.segments)()
    assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), begin, end, scan.segments, None) == 0
    return [(begin[s], end[s]) for s in range(scan.segments)]


def test_restart_intervals_are_segments(hctx):
    rows = jc.encode(jc.photo(*BIG, 3), quality=90, subsampling=2, restart_marker_rows=1)
    blocks = jc.encode(jc.photo(*BIG, 3), quality=90, subsampling=1, restart_marker_blocks=3)
    for S in (32, 1024):
        hctx.jpeg_huff_config(S, **GENEROUS)
        for label, data, nseg in (("rst-rows", rows, 25), ("rst-blocks", blocks, -(-34 * 50 // 3))):
            _equal_coefficients(hctx, label, data)
            st = hctx.jpeg_huff_stats()
            assert st["segments"] == nseg and st["fallback"] == 0 and st["subsequences"] >= nseg, (label, S, st)
            assert np.array_equal(hctx.jpeg_decode_rgb_file(data), jc.pil_decode(data)), (label, S)
    # every segment shorter than one subsequence, the last one too: one lane each
    hctx.jpeg_huff_config(1024, **GENEROUS)
    tiny = jc.encode(jc.photo(50, 47, 3), quality=50, subsampling=2, restart_marker_blocks=1)
    segs = _segments(tiny)
    assert len(segs) == 12 and 0 < segs[-1][1] - segs[-1][0] < 1024 // 8
    _equal_coefficients(hctx, "tiny segments", tiny)
    assert hctx.jpeg_huff_stats()["subsequences"] == 12
    # ... and a long segment in front of a short last one
    hctx.jpeg_huff_config(128, **GENEROUS)
    tail = jc.encode(jc.photo(64, 40, 3), quality=90, subsampling=0, restart_marker_blocks=39)
    segs = _segments(tail)
    assert len(segs) == 2 and segs[0][1] - segs[0][0] > 10 * 16 and segs[1][1] - segs[1][0] < 128 // 8 * 8
    _equal_coefficients(hctx, "short last segment", tail)


def test_work_bound_falls_back_to_the_host_decoder(hctx, big_files):
    data = big_files["edges q100"]
    want = jc.pil_decode(data)
    hctx.jpeg_huff_config(128, max_hops=2, max_rounds=2)
    assert np.array_equal(hctx.jpeg_decode_rgb_file(data), want)
    assert hctx.jpeg_huff_stats()["fallback"] == 1
    hctx.upload_bgr(0, want, 4, (5, 3, 7, 2))
    hctx.upload_jpeg_file(1, data, 4, (5, 3, 7, 2))
    assert hctx.jpeg_huff_stats()["fallback"] == 1
    assert np.array_equal(hctx.download_level(1, 0), hctx.download_level(0, 0))
    hctx.jpeg_huff_config(128, **GENEROUS)
    assert np.array_equal(hctx.jpeg_decode_rgb_file(data), want)
    assert hctx.jpeg_huff_stats()["fallback"] == 0
    with pytest.raises(ValueError):
        hctx.jpeg_huff_config(48)
    with pytest.raises(ValueError):
        hctx.jpeg_huff_config(128, max_hops=0)


def test_malformed_files_raise_and_leave_the_handle_usable(hctx, big_files):
    """one truncated file and one with a flipped byte that the host decoder rejects (tests/test_jpeg_lanes_host.py runs the
    whole list on the CPU)"""
    from iceberg_tracking_code_amd import UnsupportedJpeg, read_jpeg
    good = big_files["photo s2"]
    sos = good.index(b"\xff\xda")
    begin, end = sos + 2 + int.from_bytes(good[sos + 2:sos + 4], "big"), good.rindex(b"\xff\xd9")
    cut = good[:begin + (end - begin) // 2]
    flipped = None
    rng = np.random.default_rng(9)
    for _ in range(200):
        bad = bytearray(good)
        bad[int(rng.integers(begin, end))] ^= int(rng.integers(1, 256))
        try:
            read_jpeg(bytes(bad))
        except UnsupportedJpeg:
            raise
        except ValueError:
            flipped = bytes(bad)
            break
    assert flipped is not None
    for label, data in (("truncated", cut), ("flipped", flipped)):
        with pytest.raises(ValueError):
            hctx.jpeg_device_coefficients(data)
        with pytest.raises(ValueError):
            hctx.upload_jpeg_file(0, data, 4)
        _equal_coefficients(hctx, "good file after " + label, good)
        assert hctx.jpeg_huff_stats()["fallback"] == 0
    with pytest.raises(ValueError):
        hctx.upload_jpeg_file(0, jc.encode(jc.photo(64, 48, 25, channels=1)), 4)      # one component
    with pytest.raises(ValueError):
        hctx.upload_jpeg_file(0, good, 4, (300, 0, 300, 0))                            # nothing left
    buf = jc.encode(jc.photo(64, 48, 25), progressive=True)
    with pytest.raises(UnsupportedJpeg):
        hctx.jpeg_device_coefficients(buf)


def test_sequence_with_device_huffman_equals_pil_decoder(synth, tmp_path):
    """the folder of test_gpu_jpeg.py, one photo saved progressive (it goes through PIL), with huffman="device" """
    from iceberg_tracking_code_amd import track_image_sequence
    w, h, n, T, dts = 720, 540, 9, 2, 60
    grays, _ = synth.sequence(w, h, n, seed=31, max_step_px=2.0)
    src = tmp_path / "photos"
    src.mkdir()
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    names = []
    for k, g in enumerate(grays):
        rgb = np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)
        p = src / ((t0 + dt.timedelta(seconds=k * dts)).strftime("%Y%m%d-%H%M%S") + ".jpg")
        Image.fromarray(rgb).save(p, quality=95, progressive=(k == 3))
        names.append(str(p))
    crop = (24, 60, 16, 8)
    poly = [(40, 80), (700, 70), (690, 520), (300, 470), (50, 530)]
    fp = dict(maxCorners=400, qualityLevel=0.007, minDistance=10, blockSize=10)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
    res = {}
    for decoder, huffman in (("pil", "host"), ("device", "device")):
        dst = tmp_path / (decoder + "-" + huffman)
        dst.mkdir()
        res[decoder] = (track_image_sequence(names, str(dst), T, dts, crop=crop, mask_polygon=(poly, crop[0], crop[1]),
                                             feature_params=fp, lk_params=lk, decode_threads=3, decoder=decoder,
                                             huffman=huffman), dst)
    (a, da), (b, db) = res["pil"], res["device"]
    assert len(a) == len(b) == 4
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) and len(os.listdir(da)) == 4
    for (pa, ta, qa), (pb, tb, qb) in zip(a, b):
        assert os.path.basename(pa) == os.path.basename(pb) and len(ta) > 100
        assert np.array_equal(ta, tb) and np.array_equal(qa, qb)
        za, zb = np.load(pa, allow_pickle=False), np.load(pb, allow_pickle=False)
        assert np.array_equal(za["tracks"], zb["tracks"]) and np.array_equal(za["trackquality"], zb["trackquality"])
    with pytest.raises(ValueError):
        track_image_sequence(names, str(tmp_path), T, dts, decoder="pil", huffman="device")

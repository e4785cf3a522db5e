"""The parallel Huffman decoder of csrc/jpeg_lanes.h, run lane by lane on the CPU (icelk_jpeg_read_coefficients_lanes),
against the serial host decoder (icelk_jpeg_read_coefficients): equal coefficients on the matrix for three subsequence
lengths, the synchronisation statistics, the work bound and its fallback, stuffed bytes on subsequence boundaries, and
malformed streams.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSEQ = (32, 128, 1024)
GENEROUS = dict(max_hops=256, max_rounds=255)


def _lib():
    from iceberg_tracking_code_amd import _lib as L
    return L, L.load()


def _host(data):
    """(rc, coefficients or None) of the serial decoder"""
    L, lib = _lib()
    info = L.JpegInfo()
    rc = lib.icelk_jpeg_describe(data, len(data), C.byref(info))
    if rc:
        return rc, None
    coef = np.full(int(info.coef_count), 0x5a5a, np.int16)
    rc = lib.icelk_jpeg_read_coefficients(data, len(data), C.c_void_p(coef.ctypes.data), coef.size)
    return rc, (coef if rc == 0 else None)


def _lanes(data, S, max_hops=256, max_rounds=255):
    """(rc, coefficients or None, stats) of the lanes' decoder"""
    L, lib = _lib()
    info = L.JpegInfo()
    rc = lib.icelk_jpeg_describe(data, len(data), C.byref(info))
    if rc:
        return rc, None, None
    coef = np.full(int(info.coef_count), 0x5a5a, np.int16)
    st = L.JpegHuffStats()
    rc = lib.icelk_jpeg_read_coefficients_lanes(data, len(data), C.c_void_p(coef.ctypes.data), coef.size, S, max_hops, max_rounds,
                                                C.byref(st))
    return rc, (coef if rc == 0 else None), st


def _same_verdict(label, data, S):
    rc_h, want = _host(data)
    rc_l, got, st = _lanes(data, S)
    assert rc_l == rc_h, (label, S, rc_l, rc_h)
    if rc_h == 0:
        assert np.array_equal(got, want), (label, S, int(np.count_nonzero(got != want)))
    return rc_h, st


@pytest.fixture(scope="module")
def matrix():
    return jc.matrix()


@pytest.fixture(scope="module")
def photo_q85():
    return jc.encode(jc.photo(120, 88, 21), quality=85, subsampling=2)


@pytest.fixture(scope="module")
def edges_q100():
    return jc.encode(jc.edges(120, 88), quality=100, subsampling=2)


@pytest.mark.parametrize("S", SUBSEQ)
def test_lanes_equal_host_decoder_on_the_matrix(matrix, S):
    assert len(matrix) > 250
    labels = " ".join(label for label, _ in matrix)
    assert "rst-blocks" in labels and "rst-rows" in labels and "gray" in labels and "opt1" in labels and "1x1" in labels
    L, _ = _lib()
    decoded = 0
    for label, data in matrix:
        rc_h, want = _host(data)
        rc_l, got, st = _lanes(data, S, **GENEROUS)
        if rc_h == L.EUNSUP:                       # one and two pixels' width: no decoder of this project takes them
            assert rc_l == L.EUNSUP and label.startswith("1x1"), (label, rc_l)
            continue
        assert rc_h == rc_l == 0, (label, rc_h, rc_l)
        assert np.array_equal(got, want), (label, S, int(np.count_nonzero(got != want)))
        assert st.fallback == L.JPEG_FALLBACK_NONE, (label, S, st.fallback)
        decoded += 1
    assert decoded > 250


def test_restart_files_have_one_segment_per_interval(matrix):
    L, lib = _lib()
    seen = 0
    for label, data in matrix:
        if "rst" not in label:
            continue
        info, scan = L.JpegInfo(), L.JpegScan()
        assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, None) == 0
        nmcu, ri = info.mcus_x * info.mcus_y, info.restart_interval
        assert ri > 0 and scan.segments == -(-nmcu // ri) > 1, label
        begin, end = (C.c_uint32 * scan.segments)(), (C.c_uint32 * scan.segments)()
        tables = (C.c_uint8 * L.JPEG_TABLE_BYTES)()
        assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), begin, end, scan.segments, tables) == 0
        for s in range(scan.segments - 1):
            assert data[end[s]:end[s] + 2] == bytes([0xFF, 0xD0 + s % 8]) and begin[s + 1] == end[s] + 2, (label, s)
        assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), begin, end, 1, None) == L.ECAP
        _, _, st = _lanes(data, 128)
        assert st.segments == scan.segments
        seen += 1
    assert seen == 6


def test_many_restart_intervals_need_no_fallback():
    """567 and 25 segments; among them some whose padding ones fill a byte to FF, so that they end in a stuffed zero"""
    L, _ = _lib()
    rows = jc.encode(jc.photo(531, 397, 3), quality=90, subsampling=2, restart_marker_rows=1)
    blocks = jc.encode(jc.photo(531, 397, 3), quality=90, subsampling=1, restart_marker_blocks=3)
    assert re.search(rb"\xff\x00\xff[\xd0-\xd7]", blocks)
    for label, data, nseg in (("rst-rows", rows, 25), ("rst-blocks", blocks, 567)):
        for S in (32, 1024):
            _, want = _host(data)
            rc, got, st = _lanes(data, S, **GENEROUS)
            assert rc == 0 and st.segments == nseg and st.fallback == L.JPEG_FALLBACK_NONE, (label, S, st.fallback)
            assert np.array_equal(got, want), (label, S)


def test_statistics_say_that_lanes_start_out_of_step(photo_q85, edges_q100):
    for label, data in (("photo q85", photo_q85), ("edges q100", edges_q100)):
        rc, _, st = _lanes(data, 128, **GENEROUS)
        assert rc == 0 and st.fallback == 0 and st.segments == 1, label
        assert st.subsequences == -(-_scan_bytes(data) * 8 // 128), label
        assert st.subsequences - st.lanes_in_step > st.subsequences / 2, (label, st.lanes_in_step, st.subsequences)
        assert st.max_hops >= 2 and st.total_hops >= st.max_hops, (label, st.max_hops, st.total_hops)
        assert st.spanning_blocks >= 1, label
    # at 32 bits a lane nearly every block of the quality-100 file is longer than a subsequence
    rc, coef, st = _lanes(edges_q100, 32, **GENEROUS)
    blocks = coef.size // 64
    assert rc == 0 and st.fallback == 0 and st.spanning_blocks > 0.9 * blocks, (st.spanning_blocks, blocks)


def _scan_span(data):
    """(first byte, byte behind the last) of the entropy-coded data of a file without restart markers"""
    sos = data.index(b"\xff\xda")
    begin = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    end = begin
    while not (data[end] == 0xFF and data[end + 1] != 0):
        end += 1
    return begin, end


def _scan_bytes(data):
    begin, end = _scan_span(data)
    return end - begin


def test_work_bound_hands_the_file_to_the_host_decoder(edges_q100):
    L, _ = _lib()
    _, want = _host(edges_q100)
    rc, got, st = _lanes(edges_q100, 128, max_hops=2, max_rounds=2)     # 4 hops in all: far from enough for this file
    assert rc == 0 and st.fallback == L.JPEG_FALLBACK_BOUND
    assert np.array_equal(got, want)
    rc, got, st = _lanes(edges_q100, 128, max_hops=256, max_rounds=1)   # whole groups, but one round of carrying on
    assert rc == 0 and np.array_equal(got, want)
    rc, got, st = _lanes(edges_q100, 128, **GENEROUS)
    assert rc == 0 and st.fallback == L.JPEG_FALLBACK_NONE and st.rounds >= 1
    assert np.array_equal(got, want)


def test_bad_configuration_is_rejected(photo_q85):
    L, _ = _lib()
    for S, hops, rounds in ((0, 4, 4), (48, 4, 4), (16, 4, 4), (128, 0, 4), (128, 4, 0), (128, 4, 256)):
        rc, _, _ = _lanes(photo_q85, S, hops, rounds)
        assert rc == L.EARG, (S, hops, rounds)


def test_subsequence_boundary_on_a_stuffed_byte(edges_q100):
    begin, end = _scan_span(edges_q100)
    scan = edges_q100[begin:end]
    assert scan.count(b"\xff\x00") > 20
    L, _ = _lib()
    _, want = _host(edges_q100)
    hit = 0
    for S in (32, 64, 96, 128):
        on_stuffed = [q for q in range(S // 8, len(scan), S // 8) if scan[q] == 0 and scan[q - 1] == 0xFF]
        hit += len(on_stuffed)
        if S == 32:
            assert on_stuffed, "no subsequence of 32 bits begins on a stuffed zero"
        rc, got, st = _lanes(edges_q100, S, **GENEROUS)
        assert rc == 0 and st.fallback == L.JPEG_FALLBACK_NONE and np.array_equal(got, want), S
    assert hit >= 2


# ---- malformed input -------------------------------------------------------------------------------------------------
def _malformed_sources():
    plain = jc.encode(jc.photo(64, 48, 31), quality=85, subsampling=2)
    rst = jc.encode(jc.photo(64, 48, 32), quality=85, subsampling=2, restart_marker_blocks=2)
    return plain, rst


def _rst_scan_span(data):
    sos = data.index(b"\xff\xda")
    begin = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    return begin, data.rindex(b"\xff\xd9")


@pytest.mark.parametrize("S", (32, 128))
def test_truncated_streams(S):
    L, _ = _lib()
    for data in _malformed_sources():
        begin, end = _rst_scan_span(data)
        for part in (0.25, 0.5, 0.99):
            cut = data[:begin + int((end - begin) * part)]
            rc, _ = _same_verdict("cut %.2f" % part, cut, S)
            assert rc == L.EARG, part


@pytest.mark.parametrize("S", (32, 128))
def test_one_flipped_byte(S):
    L, _ = _lib()
    verdicts = {0: 0, L.EARG: 0}
    for k, data in enumerate(_malformed_sources()):
        begin, end = _rst_scan_span(data)
        rng = np.random.default_rng(77 + k)
        for _ in range(50):
            at = int(rng.integers(begin, end))
            bad = bytearray(data)
            bad[at] ^= int(rng.integers(1, 256))
            rc, _ = _same_verdict("flip at %d" % at, bytes(bad), S)
            assert rc in verdicts, rc
            verdicts[rc] += 1
    assert verdicts[0] > 0 and verdicts[L.EARG] > 0, verdicts     # both ends of the rule were exercised


def test_wrong_restart_order_and_trailing_garbage():
    L, lib = _lib()
    plain, rst = _malformed_sources()
    first = rst.index(b"\xff\xd1")
    swapped = rst[:first] + b"\xff\xd2" + rst[first + 2:]
    for S in (32, 128):
        rc, _ = _same_verdict("RST1 -> RST2", swapped, S)
        assert rc == L.EARG
    info, scan = L.JpegInfo(), L.JpegScan()
    assert lib.icelk_jpeg_index(swapped, len(swapped), C.byref(info), C.byref(scan), None, None, 0, None) == L.EARG
    # a restart marker too few: the last two intervals run together
    last = rst.rindex(bytes([0xFF, 0xD0 + (scan_segments(rst) - 2) % 8]))
    rc, _ = _same_verdict("marker removed", rst[:last] + rst[last + 2:], 128)
    assert rc == L.EARG
    for data in (plain, rst):
        rng = np.random.default_rng(5)
        rc, _ = _same_verdict("garbage behind EOI", data + bytes(rng.integers(0, 256, 300, dtype=np.uint8)), 128)
        assert rc == 0


def scan_segments(data):
    L, lib = _lib()
    info, scan = L.JpegInfo(), L.JpegScan()
    assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, None) == 0
    return scan.segments


def test_unsupported_and_null_arguments(photo_q85):
    import io
    from PIL import Image
    L, lib = _lib()
    buf = io.BytesIO()
    Image.fromarray(jc.photo(40, 30, 3)).save(buf, "JPEG", progressive=True)
    rc, _, _ = _lanes(buf.getvalue(), 128)
    assert rc == L.EUNSUP
    coef = np.zeros(8, np.int16)
    assert lib.icelk_jpeg_read_coefficients_lanes(photo_q85, len(photo_q85), C.c_void_p(coef.ctypes.data), 8, 128, 4, 4, None) == L.ECAP
    assert lib.icelk_jpeg_read_coefficients_lanes(None, 0, C.c_void_p(coef.ctypes.data), 8, 128, 4, 4, None) == L.EARG
    assert lib.icelk_jpeg_index(photo_q85, len(photo_q85), None, None, None, None, 0, None) == L.EARG


def test_read_jpeg_lanes_wrapper(photo_q85):
    from iceberg_tracking_code_amd import read_jpeg, read_jpeg_lanes
    j, st = read_jpeg_lanes(photo_q85, subseq_bits=256)
    assert np.array_equal(j.coef, read_jpeg(photo_q85).coef)
    assert st["segments"] == 1 and st["fallback"] == 0 and st["subsequences"] > 10
    with pytest.raises(ValueError):
        read_jpeg_lanes(photo_q85[:len(photo_q85) // 2])


def test_abi_names_the_new_entry_points():
    from iceberg_tracking_code_amd import _lib as L
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "icelk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(icelk_[a-z0-9_]+)\s*\(", text))
    new = ["icelk_jpeg_index", "icelk_jpeg_read_coefficients_lanes", "icelk_jpeg_huff_config", "icelk_jpeg_huff_stats",
           "icelk_upload_jpeg_file", "icelk_jpeg_decode_rgb_file", "icelk_jpeg_device_coefficients"]
    for name in new:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(L.JpegHuffStats) == 40 and C.sizeof(L.JpegScan) == 40
    assert L.JPEG_TABLE_BYTES == int(re.search(r"#define ICELK_JPEG_TABLE_BYTES (\d+)", text).group(1))

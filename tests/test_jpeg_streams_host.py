"""The hand-written streams of jpeg_streams.py on the CPU: the writer against the Python reader and Pillow, the host
decoder (icelk_jpeg_read_coefficients) and the CPU statement of the lane decoder (icelk_jpeg_read_coefficients_lanes)
against the reader, icelk_jpeg_index against the markers, and the properties every entry was built for, measured from
its bytes.  Every comparison is exact.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import jpeg_restatement as jr
import jpeg_streams as js
import jpeg_writer as jw

SUBSEQ = (32, 128, 512, 1024)
GENEROUS = dict(max_hops=256, max_rounds=255)
DEFAULT = dict(max_hops=256, max_rounds=8)
DECODED = [e for e in js.ENTRIES if e != "out-of-range"]


def _streams(entry):
    out = [s for s in js.catalogue() if s.entry == entry]
    assert out, entry
    return out


def _lib():
    from iceberg_tracking_code_amd import _lib as L
    return L, L.load()


# ---- the writer --------------------------------------------------------------------------------------------------------
def test_zigzag_and_code_assignment_follow_t81():
    assert jw.ZIGZAG[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and jw.ZIGZAG[-3:] == [55, 62, 63]
    assert sorted(jw.ZIGZAG) == list(range(64))
    # T.81 Figure C.1 .. C.3 on the lengths of table K.3's first symbols: 2, 3, 3, 3, 3, 3, 4
    assert jw.codes({0: 2, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 4}) == \
        {0: (0, 2), 1: (2, 3), 2: (3, 3), 3: (4, 3), 4: (5, 3), 5: (6, 3), 6: (14, 4)}
    assert jw.codes(js.AC_FF)[0x0A] == (0b1111110, 7)
    with pytest.raises(ValueError):
        jw.codes({0: 1, 1: 1, 2: 1})
    with pytest.raises(ValueError):
        jw.codes({s: 16 for s in range(2)} | {100 + n: n for n in range(1, 16)} | {99: 16})   # would need the all-ones code


@pytest.mark.parametrize("entry", js.ENTRIES)
def test_files_read_back_as_written(entry):
    """the Python reader finds exactly the coefficients that went into the writer"""
    for s in _streams(entry):
        info, planes, _ = js.reference(s.label)
        if s.coef is None:
            assert entry == "flat"          # Pillow's files: nothing went into the writer
            continue
        assert len(planes) == len(s.coef), s.label
        for c, (got, want) in enumerate(zip(planes, s.coef)):
            assert got.shape[:2] == want.shape[:2] and np.array_equal(got.reshape(want.shape), want), (s.label, c)
        assert max(int(np.abs(p.astype(np.int32)).max()) for p in planes) <= 32767
        assert info["restart_interval"] == s.restart_interval, s.label


@pytest.mark.parametrize("entry", DECODED)
def test_pixels_tier_decodes_as_pillow(entry):
    """what licenses the pixel assertions on the device: for these files the integer restatement and Pillow agree in
    every sample, so their blocks are inside the range in which "as Pillow" is defined"""
    for s in _streams(entry):
        if s.tier != "pixels":
            assert s.tier == "coefficients" and entry in ("ff-runs", "full-blocks", "categories"), s.label
            continue
        want = js.pillow(s.label)
        got = jr.decode(s.data)
        assert got.shape == want.shape and np.array_equal(got, want), (s.label, int(np.count_nonzero(got != want)))


# ---- the product's host code -------------------------------------------------------------------------------------------
def _host(data):
    L, lib = _lib()
    info = L.JpegInfo()
    rc = lib.icelk_jpeg_describe(data, len(data), C.byref(info))
    if rc:
        return rc, None, None
    coef = np.full(int(info.coef_count), 0x5a5a, np.int16)
    rc = lib.icelk_jpeg_read_coefficients(data, len(data), C.c_void_p(coef.ctypes.data), coef.size)
    return rc, coef, info


def _lanes(data, S, max_hops, max_rounds):
    L, lib = _lib()
    info = L.JpegInfo()
    assert lib.icelk_jpeg_describe(data, len(data), C.byref(info)) == 0
    coef = np.full(int(info.coef_count), 0x5a5a, np.int16)
    st = L.JpegHuffStats()
    rc = lib.icelk_jpeg_read_coefficients_lanes(data, len(data), C.c_void_p(coef.ctypes.data), coef.size, S, max_hops, max_rounds,
                                                C.byref(st))
    return rc, coef, st


@pytest.mark.parametrize("entry", DECODED)
def test_host_decoder_equals_the_reader(entry):
    for s in _streams(entry):
        info, planes, want = js.reference(s.label)
        rc, got, pinfo = _host(s.data)
        assert rc == 0, (s.label, rc)
        assert (pinfo.width, pinfo.height, pinfo.ncomp) == (info["width"], info["height"], info["ncomp"]), s.label
        assert [pinfo.coef_offset[c] for c in range(len(planes))] == list(np.cumsum([0] + [p.size for p in planes])[:-1]), s.label
        assert got.shape == want.shape and np.array_equal(got, want), (s.label, int(np.count_nonzero(got != want)))
        for c in range(len(planes)):
            assert np.array_equal(np.array(pinfo.quant[c]).reshape(8, 8), info["quant"][c]), (s.label, c)


@pytest.mark.parametrize("S", SUBSEQ)
@pytest.mark.parametrize("entry", DECODED)
def test_lane_statement_equals_the_reader(entry, S):
    L, _ = _lib()
    for s in _streams(entry):
        want = js.reference(s.label)[2]
        rc, got, st = _lanes(s.data, S, **GENEROUS)
        assert rc == 0 and st.fallback == L.JPEG_FALLBACK_NONE, (s.label, S, rc, st.fallback)
        assert np.array_equal(got, want), (s.label, S, int(np.count_nonzero(got != want)))
        assert st.segments == s.segments, (s.label, st.segments)
        rc, got, st = _lanes(s.data, S, **DEFAULT)
        assert rc == 0 and st.fallback in (L.JPEG_FALLBACK_NONE, L.JPEG_FALLBACK_BOUND), (s.label, S, rc, st.fallback)
        assert np.array_equal(got, want), (s.label, S, "default bounds", int(np.count_nonzero(got != want)))


def test_flat_frames_do_not_synchronise():
    """a black frame never gets a lane in step at 32 bits; under the default bounds the host decoder takes it over"""
    L, _ = _lib()
    s = js.stream("flat black 420 736x736")
    rc, _, st = _lanes(s.data, 32, **DEFAULT)
    assert rc == 0 and (st.fallback, st.lanes_in_step, st.rounds) == (L.JPEG_FALLBACK_BOUND, 0, 9)
    rc, _, st = _lanes(s.data, 32, **GENEROUS)
    assert rc == 0 and st.fallback == L.JPEG_FALLBACK_NONE and st.lanes_in_step == 1 and st.rounds == 9


# ---- icelk_jpeg_index ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", DECODED)
def test_index_reports_the_segments_between_the_markers(entry):
    L, lib = _lib()
    for s in _streams(entry):
        data, m = s.data, js.measure(s.data)
        info, scan = L.JpegInfo(), L.JpegScan()
        assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, None) == 0, s.label
        assert scan.segments == s.segments == len(m["segments"]), (s.label, scan.segments, len(m["segments"]))
        assert scan.blocks_per_mcu == m["blocks_per_mcu"] and scan.total_blocks == m["blocks_per_mcu"] * m["mcus"], s.label
        assert [(scan.dc_table[b], scan.ac_table[b]) for b in range(scan.blocks_per_mcu)] == \
            [m["selectors"][scan.component[b]] for b in range(scan.blocks_per_mcu)], s.label
        begin, end = (C.c_uint32 * scan.segments)(), (C.c_uint32 * scan.segments)()
        assert lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), begin, end, scan.segments, None) == 0
        assert [(begin[k], end[k]) for k in range(scan.segments)] == m["segments"], s.label
        for k, (at, fills, n) in enumerate(m["rst"]):
            # the segment ends where the fill bytes begin, the next one begins behind the marker, the markers count up
            assert end[k] == at - fills and begin[k + 1] == at + 2 and n == k % 8, (s.label, k)
            assert data[end[k]:begin[k + 1]] == b"\xff" * fills + bytes([0xFF, 0xD0 + k % 8]), (s.label, k)


# ---- the properties the entries were built for -----------------------------------------------------------------------------
def _cps(mcus_per_interval):
    return -(-mcus_per_interval // js.DC_CHUNK)


def _bits_add_up(label):
    """the blocks' bits, padded per segment, are the file's entropy-coded bytes"""
    s, m, bits = js.stream(label), js.measure(js.stream(label).data), js.block_bits(label)
    per_seg = m["blocks_per_mcu"] * (s.restart_interval if s.segments > 1 else m["mcus"])
    nbytes = sum(-(-sum(bits[k:k + per_seg]) // 8) for k in range(0, len(bits), per_seg))
    assert nbytes + m["ff_pairs"] == m["scan_bytes"], (label, nbytes, m["ff_pairs"], m["scan_bytes"])
    return bits


def test_every_stream_adds_up():
    for s in js.catalogue():
        _bits_add_up(s.label)


def test_properties_long_codes():
    (s,) = _streams("long-codes")
    m = js.measure(s.data)
    assert set(m["dht_bits"]) == {(0, 0), (1, 0)}
    planes = js.reference(s.label)[1]
    counts = jw.symbol_counts([p.reshape(p.shape[0], p.shape[1], 64) for p in planes], s.sampling)
    for kind, per_component in zip((0, 1), counts):
        assert all(n >= 1 for n in m["dht_bits"][(kind, 0)]), kind          # a code of every length 1 .. 16
        used = js._total(per_component)
        long = sum(n for sym, n in used.items() if m["dht"][(kind, 0)][sym] >= 10)
        assert long > 0.5 * sum(used.values()), (kind, long, sum(used.values()))
        assert max(used, key=used.get) in [sym for sym, ln in m["dht"][(kind, 0)].items() if ln >= 10]
        assert {m["dht"][(kind, 0)][sym] for sym in used} >= set(range(10, 17)), kind   # every long length occurs in the scan
    print("long-codes: bits per block %.0f, FF share %.2f" % (np.mean(js.block_bits(s.label)), m["ff_share"]))


def test_properties_ff_runs():
    (s,) = _streams("ff-runs")
    m = js.measure(s.data)
    print("ff-runs: FF share %.3f, longest run of pairs %d" % (m["ff_share"], m["ff_run"]))
    assert m["ff_share"] > 0.5 and m["ff_run"] >= 2
    assert b"\xff\x00\xff\x00" in s.data[m["segments"][0][0]:m["segments"][0][1]]


def test_properties_two_bit_blocks():
    shared, separate = _streams("two-bit-blocks")
    for s in (shared, separate):
        bits = js.block_bits(s.label)
        assert set(bits) == {2} and sum(bits) >= 1024 and 1024 // 2 >= 512, s.label     # a full lane of 1024 bits: 512 blocks
        assert sum(bits) - js.reference(s.label)[0]["mcus_x"] * 6 * 2 < 1024, s.label    # and a row of MCUs less would not do
        m = js.measure(s.data)
        assert m["blocks_per_mcu"] == 6 and m["scan_bytes"] * 8 == sum(bits), s.label
    assert set(js.measure(shared.data)["selectors"]) == {(0, 0)} and len(js.measure(shared.data)["dht"]) == 2
    assert js.measure(separate.data)["selectors"] == [(0, 0), (1, 1), (1, 1)] and len(js.measure(separate.data)["dht"]) == 4


def test_properties_full_blocks():
    (s,) = _streams("full-blocks")
    bits = js.block_bits(s.label)
    print("full-blocks: bits per block %d .. %d" % (min(bits), max(bits)))
    assert min(bits) > 1024                                # longer than the longest subsequence: spans lanes at every S
    planes = js.reference(s.label)[1]
    ac = planes[0].reshape(-1, 64)[:, 1:].astype(np.int32)
    assert np.all((np.abs(ac) >= 512) & (np.abs(ac) <= 1023))   # all 63 at category 10
    assert sum(bits) > 16 * 256 * 32                       # more than 16 groups of lanes at 32 bits


def test_properties_runs():
    (s,) = _streams("runs")
    m = js.measure(s.data)
    assert m["restart_interval"] == 5 and len(m["segments"]) == 7 == -(-m["mcus"] // 5)
    planes = js.reference(s.label)[1]
    zz = np.concatenate([p.reshape(-1, 64)[:, jw.ZIGZAG] for p in planes])
    only63 = [b for b in zz if np.flatnonzero(b[1:]).tolist() == [62]]
    assert len(only63) >= 5
    assert sum(1 for b in zz if b[63] != 0) > len(only63)          # position 63 filled behind other coefficients too
    assert any(b[62] != 0 and b[63] == 0 for b in zz) and any(not b[1:].any() for b in zz)
    ac = js._total(jw.symbol_counts([p.reshape(p.shape[0], p.shape[1], 64) for p in planes], s.sampling, 5)[1])
    assert ac[0xF0] >= 3 * len(only63)                              # ZRL x3 in front of coefficient 63
    assert any(sym >> 4 == 14 for sym in ac) and any(sym >> 4 == 15 and sym & 15 for sym in ac)    # run 14; exactly 15 zeros
    gaps = [np.diff(np.flatnonzero(np.r_[1, b[1:]])) - 1 for b in zz]
    assert any(15 in g for g in gaps) and any(16 in g for g in gaps)
    print("runs: segments of %s bytes" % [e - b for b, e in m["segments"]])


def test_properties_categories():
    (s,) = _streams("categories")
    planes = js.reference(s.label)[1]
    dc, ac = jw.symbol_counts([planes[0].reshape(planes[0].shape[0], -1, 64)], s.sampling)
    assert set(dc[0]) == {11, 12, 13, 14, 15}
    assert {sym & 15 for sym in ac[0] if sym & 15} == {11, 12, 13, 14, 15}
    diffs = np.diff(np.r_[0, planes[0].reshape(-1, 64)[:, 0].astype(np.int32)])
    assert np.all(np.sign(diffs) == np.where(np.arange(diffs.size) % 2 == 0, 1, -1))


def test_properties_slots():
    crossed, four = _streams("slots")
    m = js.measure(crossed.data)
    assert set(m["dht"]) == {(0, 3), (0, 1), (1, 2), (1, 0)} and m["selectors"] == [(3, 0), (1, 2), (3, 0)]
    assert m["quant_slots"] == [0, 3, 3]
    m = js.measure(four.data)
    assert set(m["dht"]) == {(k, t) for k in (0, 1) for t in range(4)} and m["selectors"] == [(2, 1), (0, 3), (0, 1)]
    assert m["quant_slots"] == [1, 3, 3]
    # the tables of one kind differ in their codes: a decoder that takes the wrong slot reads other symbols
    for kind in (0, 1):
        orders = [list(m["dht"][(kind, t)]) for t in range(4)]
        assert all(orders[a] != orders[b] for a in range(4) for b in range(a))


def test_properties_ri_1():
    (s,) = _streams("ri-1")
    m = js.measure(s.data)
    assert m["restart_interval"] == 1 and m["mcus"] == 256 and len(m["segments"]) == 256
    assert {e - b for b, e in m["segments"]} == {2} and set(js.block_bits(s.label)) == {2}
    assert [n for _, _, n in m["rst"]] == [k % 8 for k in range(255)] and 256 // 8 == 32


def test_properties_ri_edges():
    by = {s.label.split()[-1]: s for s in _streams("ri-edges")}
    assert set(by) == {"no-padding", "ff-padding", "fill-rst", "ri-above", "ri-uneven"}
    s = by["no-padding"]
    m, bits = js.measure(s.data), js.block_bits(s.label)
    per = m["blocks_per_mcu"] * 2
    assert len(m["segments"]) == 4 and all(sum(bits[k:k + per]) == 8 * (e - b) for k, (b, e) in zip(range(0, 48, per), m["segments"]))
    s = by["ff-padding"]
    m, bits = js.measure(s.data), js.block_bits(s.label)
    ends_ff = [k for k, (b, e) in enumerate(m["segments"]) if s.data[e - 2:e] == b"\xff\x00" and bits[k] % 8]
    print("ri-edges ff-padding: segments whose padding completes an FF:", ends_ff)
    assert len(ends_ff) >= 3 and len(ends_ff) < len(m["segments"]) and re.search(rb"\xff\x00\xff[\xd0-\xd7]", s.data)
    for k in ends_ff:      # the byte's leading bits are data, the rest padding
        assert 0 < bits[k] % 8 and m["segments"][k][1] - m["segments"][k][0] == -(-bits[k] // 8) + 1
    m = js.measure(by["fill-rst"].data)
    assert [fills for _, fills, _ in m["rst"]] == [1, 3]
    m = js.measure(by["ri-above"].data)
    assert m["restart_interval"] == 100 > m["mcus"] == 6 and len(m["segments"]) == 1 and not m["rst"]
    m = js.measure(by["ri-uneven"].data)
    assert m["restart_interval"] == 4 and m["mcus"] % 4 == 2 and len(m["segments"]) == 2


def test_properties_big_interval():
    a, b, c = _streams("big-interval")
    facts = []
    for s, mcus, ri, cps, passes, segs in ((a, 8256, 0, 516, 3, 1), (b, 4224, 0, 264, 2, 1), (c, 4224, 4100, 257, 2, 2)):
        m = js.measure(s.data)
        assert m["mcus"] == mcus and m["restart_interval"] == ri and len(m["segments"]) == segs == s.segments, s.label
        assert _cps(ri or mcus) == cps and -(-cps // 256) == passes, s.label
        assert len(s.data) <= 40 * 1024, (s.label, len(s.data))
        planes = js.reference(s.label)[1]
        coef = [p.reshape(p.shape[0], p.shape[1], 64) for p in planes]
        assert not any(p[..., 1:].any() for p in coef), s.label
        sums = js.dc_chunk_sums(coef, s.sampling, ri)
        assert len(sums) == len(coef) and all(len(row) == (cps if segs == 1 else cps + _cps(mcus - ri)) for row in sums), s.label
        assert all(v != 0 for row in sums for v in row), s.label
        pred = {}
        for _, comp, blk, first in jw.scan_order(coef, s.sampling, ri):      # DC differs from block to block
            assert first or pred.get(comp) != int(blk[0]), s.label
            pred[comp] = int(blk[0])
        facts.append("%s: %d bytes, %d MCUs, cps %d, %d passes" % (s.label, len(s.data), mcus, cps, passes))
    print("\n".join(facts))


def test_properties_headers():
    merged, split = _streams("headers")
    m = js.measure(merged.data)
    marks = [k for k, _, _ in m["markers"]]
    assert marks.count(0xC4) == 1 and marks.count(0xDB) == 1 and marks.count(0xFE) == 2 and marks.count(0xE1) == 1
    assert {k: f for k, _, f in m["markers"] if f} == {0xC4: 2, 0xC0: 1}
    assert 0xDD in marks and m["restart_interval"] == 0
    at = next(pos for k, pos, _ in m["markers"] if k == 0xE1)
    body = merged.data[at + 4:at + 2 + int.from_bytes(merged.data[at + 2:at + 4], "big")]
    thumb = body[body.index(b"\xff\xd8"):]
    assert thumb.endswith(b"\xff\xd9") and b"\xff\xda" in thumb and b"\xff\xc0" in thumb
    info = jr.coefficients(thumb)[0]
    assert (info["width"], info["height"], info["ncomp"]) == (16, 8, 1)      # a complete file of another shape
    m = js.measure(split.data)
    marks = [k for k, _, _ in m["markers"]]
    assert marks.count(0xC4) == 4 and marks.count(0xDB) == 2 and 0xDD not in marks
    assert {k: f for k, _, f in m["markers"] if f} == {0xDB: 1, 0xDA: 3}


def test_properties_flat():
    flat = _streams("flat")
    assert len(flat) == 12
    seen = set()
    for s in flat:
        px = js.pillow(s.label)
        shade, sub, size = s.label.split()[1:]
        assert "%dx%d" % (px.shape[1], px.shape[0]) == size and (px.shape[1], px.shape[0]) in js.FLAT_SIZES
        assert px.min() == px.max() == {"black": 0, "white": 255, "mid-gray": 128}[shade], s.label
        assert js.measure(s.data)["blocks_per_mcu"] == {"420": 6, "444": 3}[sub]
        seen.add((shade, sub, size))
    assert len(seen) == 12


def _idct_two_passes(x):
    x = jr._idct_1d(x, 11)
    return np.swapaxes(jr._idct_1d(np.swapaxes(x, -1, -2), 18), -1, -2)


def _wrapped_samples(label):
    """samples in which the inverse DCT in 32-bit wrap-around arithmetic (numpy's int32) departs from the one in 64 bits"""
    info, planes, _ = js.reference(label)
    n = 0
    for p, q in zip(planes, info["quant"]):
        x = p.astype(np.int64) * q.astype(np.int64)
        n += int(np.count_nonzero(_idct_two_passes(x) != _idct_two_passes(x.astype(np.int32))))
    return n


def test_pixels_tier_stays_inside_32_bits():
    for s in js.catalogue():
        if s.tier == "pixels":
            assert _wrapped_samples(s.label) == 0, s.label


def test_properties_out_of_range():
    """No 8-bit block has this energy: the DCT is orthonormal, so the squares of a block's dequantised coefficients sum
    to those of its 64 samples, at most 64 * 128^2 (a little more behind a quantiser)."""
    big, clip = _streams("out-of-range")
    for s, q, top in ((big, 1, 1023), (clip, 16, 255)):
        info, planes, _ = js.reference(s.label)
        assert all(np.all(t == q) for t in info["quant"]) and max(int(np.abs(p).max()) for p in planes) == top
        for p in planes:
            energy = ((p.astype(np.float64) * q) ** 2).reshape(-1, 64).sum(1)
            assert energy.min() > 4 * 64 * 128 ** 2, s.label
    assert np.all(np.abs(js.reference(clip.label)[1][0]) == 255)
    # 255 * 16 in every coefficient: the sums of the kernel's 32-bit inverse DCT wrap
    print("out-of-range: samples a 32-bit inverse DCT wraps in: %d and %d" % (_wrapped_samples(big.label), _wrapped_samples(clip.label)))
    assert _wrapped_samples(clip.label) > 0

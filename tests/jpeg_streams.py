"""The catalogue of hand-written JPEG streams (jpeg_writer.py) that test_jpeg_streams_host.py and
test_gpu_jpeg_streams.py decode: what Pillow's encoder with its two table sets never emits.  `catalogue()` makes every
file once per process; a Stream unpacks as (label, bytes, tier).

    tier "pixels"        the blocks come from `blocks_from_pixels`, so they are what an 8-bit encoder can produce: the
                         decoded pixels must equal Pillow's.  Content designed as coefficients goes through
                         `pixels_from_blocks` first and must come back unchanged (`_through_pixels`).
    tier "coefficients"  anything the syntax allows inside int16: only the coefficients are compared.
    tier "out-of-range"  coefficients far outside what a forward DCT of 8-bit samples gives: nothing is said about the
                         pixels, the decoder only has to stay well-behaved.

Every size is the smallest at which the property the entry is built for holds; test_jpeg_streams_host.py measures the
properties from the bytes (`measure`), so an edit here cannot drop them unnoticed.
"""
import functools

import numpy as np

import jpeg_cases as jc
import jpeg_restatement as jr
import jpeg_writer as jw

DC_CHUNK = 16        # MCUs per chunk of the device's DC pass (kJpegDcChunk); its scan loop takes 256 chunks per pass


class Stream:
    """entry: the catalogue's name for the property; coef / sampling: what went into the writer (None for Pillow's own
    files); restart_interval and segments: as the file states and implies them"""

    def __init__(self, entry, label, data, tier, coef=None, sampling=None, restart_interval=0, segments=1):
        self.entry, self.label, self.data, self.tier = entry, label, data, tier
        self.coef, self.sampling, self.restart_interval, self.segments = coef, sampling, restart_interval, segments

    def __iter__(self):
        return iter((self.label, self.data, self.tier))

    def __repr__(self):
        return "Stream(%s)" % self.label


# ---- tables ----------------------------------------------------------------------------------------------------------
DC_FLAT = jw.flat_table(jw.DC_SYMBOLS, 4)
AC_FLAT = jw.flat_table(jw.AC_SYMBOLS, 8)
DC_FLAT_ALL = jw.flat_table(jw.DC_SYMBOLS_ALL, 5)
AC_FLAT_ALL = jw.flat_table(jw.AC_SYMBOLS_ALL, 8)
DC_ONE_BIT = {c: c + 1 for c in range(12)}                      # category 0 is the code "0"
AC_ONE_BIT = {0x00: 1, 0x01: 2, 0x11: 3, 0xF0: 4, 0x02: 5}       # end-of-block is the code "0"
DC_ONE_BIT_B = {0: 1, 5: 2, 3: 3, 1: 4}
AC_ONE_BIT_B = {0x00: 1, 0x21: 2, 0x01: 3}
AC_FF = {0x01: 1, 0x02: 2, 0x03: 3, 0x04: 4, 0x05: 5, 0x06: 6, 0x0A: 7, 0x00: 8, 0xF0: 8}     # 0x0A is "1111110"

Q_LUMA = np.array([4 + 3 * (r + c) for r in range(8) for c in range(8)])
Q_CHROMA = np.array([6 + 5 * (r + c) for r in range(8) for c in range(8)])
Q8, Q16, Q1 = np.full(64, 8), np.full(64, 16), np.full(64, 1)

S444, S420, GRAY = [(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)], [(1, 1)]


def _shuffled(symbols, length, seed):
    """a flat table whose codes differ from those of every other seed: the wrong slot decodes to something else"""
    order = list(symbols)
    np.random.default_rng(seed).shuffle(order)
    return jw.flat_table(order, length)


def _write(coef, w, h, sampling, q=None, comp_q=None, dc=None, ac=None, comp_dc=None, comp_ac=None, **kw):
    n = len(coef)
    q = q if q is not None else ({0: Q_LUMA, 1: Q_CHROMA} if n == 3 else {0: Q_LUMA})
    comp_q = comp_q if comp_q is not None else [0, 1, 1][:n]
    return jw.write(coef, w, h, sampling, q, comp_q, dc or {0: DC_FLAT}, ac or {0: AC_FLAT}, comp_dc or [0] * n,
                    comp_ac or [0] * n, **kw)


def _photo_blocks(w, h, sampling, seed, qs=None):
    """a photo of jpeg_cases as an 8-bit encoder sees it"""
    if len(sampling) == 1:
        return jw.blocks_from_pixels(jc.photo(w, h, seed, channels=1), sampling, qs or [Q_LUMA])
    return jw.blocks_from_pixels(jw.ycbcr_from_rgb(jc.photo(w, h, seed)), sampling, qs or [Q_LUMA, Q_CHROMA, Q_CHROMA])


def _through_pixels(coef, sampling, qs):
    """designed coefficients -> 8-bit samples -> the encoder's coefficients, which must be the designed ones"""
    back = jw.blocks_from_pixels(jw.pixels_from_blocks(coef, sampling, qs), sampling, qs)
    for a, b in zip(coef, back):
        assert np.array_equal(a, b), "the designed blocks do not survive 8-bit samples"
    return back


def _zero_blocks(w, h, sampling):
    img = np.full((h, w) if len(sampling) == 1 else (h, w, 3), 128, np.uint8)
    coef = jw.blocks_from_pixels(img, sampling, [Q8] * len(sampling))
    assert not any(p.any() for p in coef)
    return coef


def _segments(coef, sampling, ri):
    n = (coef[0].shape[0] // sampling[0][1]) * (coef[0].shape[1] // sampling[0][0])
    return -(-n // ri) if 0 < ri < n else 1


# ---- the entries -----------------------------------------------------------------------------------------------------
def _long_code_lengths(counts, all_symbols):
    """one code of every length 1 .. 16; the seven symbols the content uses most get the lengths 10 .. 16, the other
    symbols in use 9 downwards, symbols not in use the short rest"""
    used = sorted(counts, key=lambda s: (-counts[s], s))
    assert 7 <= len(used) <= 16, len(used)
    spare = [s for s in all_symbols if s not in counts]
    lengths = {s: n for s, n in zip(used[:7], range(10, 17))}
    lengths.update({s: n for s, n in zip(used[7:] + spare, range(9, 0, -1))})
    assert sorted(lengths.values()) == list(range(1, 17))
    return lengths


def _total(per_component):
    out = {}
    for d in per_component:
        for s, n in d.items():
            out[s] = out.get(s, 0) + n
    return out


def _long_codes():
    rng = np.random.default_rng(101)
    w, h = 48, 40
    coef = [np.zeros((h // 8, w // 8, 64), np.int16) for _ in range(3)]
    for p in coef:
        dc = 0
        for blk in p.reshape(-1, 64):
            dc = int(np.clip(dc + rng.integers(-40, 41), -50, 50))
            blk[0] = dc
            k = 0
            for _ in range(int(rng.integers(2, 7))):
                k += 1 + int(rng.choice([0, 1, 2, 5]))
                if k > 63:
                    break
                mag = int(rng.choice([1, 1, 1, 2, 3, 3, 5]))
                blk[jw.ZIGZAG[k]] = mag if rng.integers(0, 2) else -mag
    coef = _through_pixels(coef, S444, [Q8] * 3)
    dcs, acs = jw.symbol_counts(coef, S444)
    dc_t, ac_t = _long_code_lengths(_total(dcs), jw.DC_SYMBOLS_ALL), _long_code_lengths(_total(acs), jw.AC_SYMBOLS)
    data = _write(coef, w, h, S444, q={0: Q8}, comp_q=[0, 0, 0], dc={0: dc_t}, ac={0: ac_t})
    return [Stream("long-codes", "long-codes 444 48x40", data, "pixels", coef, S444)]


def _ff_runs():
    coef = [np.full((8, 8, 64), 1023, np.int16)]
    coef[0][..., 0] = 0
    data = _write(coef, 64, 64, GRAY, q={0: Q1}, dc={0: DC_FLAT_ALL}, ac={0: AC_FF})
    return [Stream("ff-runs", "ff-runs gray 64x64", data, "coefficients", coef, GRAY)]


def _two_bit_blocks():
    w, h = 176, 128          # 88 MCUs of 6 blocks of 2 bits: 1056 bits, the first lane of 1024 bits holds 512 blocks
    coef = _zero_blocks(w, h, S420)
    shared = _write(coef, w, h, S420, q={0: Q8}, comp_q=[0, 0, 0], dc={0: DC_ONE_BIT}, ac={0: AC_ONE_BIT})
    separate = _write(coef, w, h, S420, q={0: Q8, 1: Q16}, dc={0: DC_ONE_BIT, 1: DC_ONE_BIT_B}, ac={0: AC_ONE_BIT, 1: AC_ONE_BIT_B},
                      comp_dc=[0, 1, 1], comp_ac=[0, 1, 1])
    return [Stream("two-bit-blocks", "two-bit-blocks shared", shared, "pixels", coef, S420),
            Stream("two-bit-blocks", "two-bit-blocks separate", separate, "pixels", coef, S420)]


def _full_blocks():
    rng = np.random.default_rng(102)
    w, h = 96, 80            # 120 blocks of more than 1024 bits: 17 groups of lanes at 32 bits
    coef = [(rng.integers(512, 1024, (h // 8, w // 8, 64)) * rng.choice([-1, 1], (h // 8, w // 8, 64))).astype(np.int16)]
    coef[0][..., 0] = np.cumsum(rng.integers(-30, 31, coef[0].shape[:2]).ravel()).reshape(coef[0].shape[:2])
    data = _write(coef, w, h, GRAY, q={0: Q1}, dc={0: DC_FLAT_ALL}, ac={0: AC_FLAT_ALL})
    return [Stream("full-blocks", "full-blocks gray 96x80", data, "coefficients", coef, GRAY)]


RUN_PATTERNS = {
    "only-63": [63],              # ZRL x3, then run 14; no end-of-block
    "15-and-16": [1, 17, 34],     # runs of 0, exactly 15 and exactly 16 zeros, then end-of-block
    "to-63": [16, 33, 63],        # run 15 first, ZRL + run 0, ZRL + run 13 up to position 63; no end-of-block
    "zero": [],
    "62": [62],                   # one short of a full block: ends with end-of-block
}


def _runs():
    rng = np.random.default_rng(103)
    w, h, ri = 56, 40, 5
    names = list(RUN_PATTERNS)
    coef = [np.zeros((h // 8, w // 8, 64), np.int16) for _ in range(3)]
    for c, p in enumerate(coef):
        for n, blk in enumerate(p.reshape(-1, 64)):
            blk[0] = int(rng.integers(-20, 21))
            for k in RUN_PATTERNS[names[(n + c) % len(names)]]:
                blk[jw.ZIGZAG[k]] = int(rng.choice([-2, -1, 1, 2]))
    coef = _through_pixels(coef, S444, [Q16] * 3)
    data = _write(coef, w, h, S444, q={0: Q16}, comp_q=[0, 0, 0], restart_interval=ri)
    return [Stream("runs", "runs 444 56x40 ri5", data, "pixels", coef, S444, ri, _segments(coef, S444, ri))]


def _categories():
    rng = np.random.default_rng(104)
    w, h = 80, 16
    coef = [np.zeros((h // 8, w // 8, 64), np.int16)]
    pred = 0
    for n, blk in enumerate(coef[0].reshape(-1, 64)):
        cat = 11 + n % 5
        mag = (1 << (cat - 1)) + int(rng.integers(0, 1 << (cat - 3)))
        pred += mag if n % 2 == 0 else -mag
        assert -32768 <= pred <= 32767
        blk[0] = pred
        for k in rng.choice(np.arange(1, 64), 6, replace=False):
            c = 11 + int(rng.integers(0, 5))
            v = int(rng.integers(1 << (c - 1), 1 << c))
            blk[jw.ZIGZAG[int(k)]] = v if rng.integers(0, 2) else -v
    data = _write(coef, w, h, GRAY, q={0: Q1}, dc={0: DC_FLAT_ALL}, ac={0: AC_FLAT_ALL})
    return [Stream("categories", "categories gray 80x16", data, "coefficients", coef, GRAY)]


def _slots():
    w, h = 48, 32
    coef = _photo_blocks(w, h, S420, 41)
    dcs = {s: _shuffled(jw.DC_SYMBOLS, 4, 200 + s) for s in range(4)}
    acs = {s: _shuffled(jw.AC_SYMBOLS, 8, 210 + s) for s in range(4)}
    q = {0: Q_LUMA, 3: Q_CHROMA}
    crossed = _write(coef, w, h, S420, q=q, comp_q=[0, 3, 3], dc={3: dcs[3], 1: dcs[1]}, ac={2: acs[2], 0: acs[0]},
                     comp_dc=[3, 1, 3], comp_ac=[0, 2, 0])
    q4 = {0: Q16, 1: Q_LUMA, 2: Q8, 3: Q_CHROMA}
    four = _write(coef, w, h, S420, q=q4, comp_q=[1, 3, 3], dc=dcs, ac=acs, comp_dc=[2, 0, 0], comp_ac=[1, 3, 1])
    return [Stream("slots", "slots crossed 420 48x32", crossed, "pixels", coef, S420),
            Stream("slots", "slots four-defined 420 48x32", four, "pixels", coef, S420)]


def _ri_1():
    w, h = 256, 256
    coef = _zero_blocks(w, h, S420)
    data = _write(coef, w, h, S420, q={0: Q8}, comp_q=[0, 0, 0], dc={0: DC_ONE_BIT}, ac={0: AC_ONE_BIT}, restart_interval=1)
    return [Stream("ri-1", "ri-1 420 256x256", data, "pixels", coef, S420, 1, 256)]


def _ri_edges():
    out = []
    # 12 bits per MCU, two MCUs per interval: three bytes and no padding
    coef = _zero_blocks(64, 32, S420)
    data = _write(coef, 64, 32, S420, q={0: Q8}, comp_q=[0, 0, 0], dc={0: DC_ONE_BIT}, ac={0: AC_ONE_BIT}, restart_interval=2)
    out.append(Stream("ri-edges", "ri-edges no-padding", data, "pixels", coef, S420, 2, 4))
    # one block per interval: DC (4 + category bits), ZRL x3 and (14, 4) (32 bits), the value 15 = "1111".  With category
    # 4 the value's ones begin a byte that the padding completes to FF
    coef = [np.zeros((1, 8, 64), np.int16)]
    coef[0][0, :, 0] = [9, 3, -12, 1, 15, 40, -8, 10]
    coef[0][0, :, 63] = 15
    coef = _through_pixels(coef, GRAY, [Q8])
    data = _write(coef, 64, 8, GRAY, q={0: Q8}, restart_interval=1)
    out.append(Stream("ri-edges", "ri-edges ff-padding", data, "pixels", coef, GRAY, 1, 8))
    coef = _photo_blocks(48, 32, S420, 42)
    data = _write(coef, 48, 32, S420, restart_interval=2, fill_rst={0: 1, 1: 3})
    out.append(Stream("ri-edges", "ri-edges fill-rst", data, "pixels", coef, S420, 2, 3))
    data = _write(coef, 48, 32, S420, restart_interval=100)
    out.append(Stream("ri-edges", "ri-edges ri-above", data, "pixels", coef, S420, 100, 1))
    data = _write(coef, 48, 32, S420, restart_interval=4)
    out.append(Stream("ri-edges", "ri-edges ri-uneven", data, "pixels", coef, S420, 4, 2))
    return out


def dc_chunk_sums(coef, sampling, ri):
    """per component, the sums of the DC differences over the chunks of DC_CHUNK MCUs of every restart interval, as the
    device's DC pass forms them: (components, chunks)"""
    ncomp = len(coef)
    nmcu = (coef[0].shape[0] // sampling[0][1]) * (coef[0].shape[1] // sampling[0][0])
    ri = ri if 0 < ri < nmcu else nmcu
    sums, pred = {}, [0] * ncomp
    for m, c, blk, first in jw.scan_order(coef, sampling, ri):
        if first:
            pred = [0] * ncomp
        key = (c, m // ri, (m % ri) // DC_CHUNK)
        sums[key] = sums.get(key, 0) + int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
    return [[v for (cc, _, _), v in sorted(sums.items()) if cc == c] for c in range(ncomp)]


def _constant_blocks(w, h, sampling, ri, seed):
    """every block of every component a constant of its own: DC only, and no chunk of the DC pass sums to zero"""
    rng = np.random.default_rng(seed)
    ncomp = len(sampling)
    hmax, vmax = sampling[0]
    want = [np.zeros((h // 8 * v // vmax, w // 8 * hh // hmax, 64), np.int16) for hh, v in sampling]
    nmcu = (h // (8 * vmax)) * (w // (8 * hmax))
    length = ri if 0 < ri < nmcu else nmcu
    # a sample value per block, drawn in scan order: never the value of the component's block in front, and at the
    # end of a chunk never the value the chunk in front ended on (a chunk's sum is the difference of the two)
    last, chunk_end = [128] * ncomp, [128] * ncomp
    draws = iter(rng.integers(0, 256, 4 * sum(p.shape[0] * p.shape[1] for p in want)).tolist())
    blocks = list(jw.scan_order(want, sampling, length))
    for n, (m, c, blk, first) in enumerate(blocks):
        if first:
            last, chunk_end = [128] * ncomp, [128] * ncomp
        q = m % length
        closes = (q % DC_CHUNK == DC_CHUNK - 1 or q == length - 1 or m == nmcu - 1) and \
            (n + 1 == len(blocks) or blocks[n + 1][1] != c or blocks[n + 1][0] != m)
        v = next(draws)
        while v == last[c] or (closes and v == chunk_end[c]):
            v = next(draws)
        blk[0] = v - 128
        last[c] = v
        if closes:
            chunk_end[c] = v
    coef = _through_pixels(want, sampling, [Q8] * ncomp)
    assert not any(p[..., 1:].any() for p in coef)
    assert all(all(s != 0 for s in row) for row in dc_chunk_sums(coef, sampling, ri))
    return coef


def _big_interval():
    out = []
    ac = {0: {0x00: 1, 0x01: 2, 0xF0: 3}}
    for tag, w, h, sampling, ri in (("a gray 1032x512", 1032, 512, GRAY, 0), ("b 444 528x512", 528, 512, S444, 0),
                                    ("c 420 1056x1024 ri4100", 1056, 1024, S420, 4100)):
        coef = _constant_blocks(w, h, sampling, ri, 300)
        data = _write(coef, w, h, sampling, q={0: Q8}, comp_q=[0] * len(sampling), ac=ac, restart_interval=ri)
        out.append(Stream("big-interval", "big-interval " + tag, data, "pixels", coef, sampling, ri, 2 if ri else 1))
    return out


def _headers():
    w, h = 40, 24
    thumb_coef = _photo_blocks(16, 8, GRAY, 44, [Q16])
    thumb = _write(thumb_coef, 16, 8, GRAY, q={0: Q16}, dc={0: _shuffled(jw.DC_SYMBOLS, 4, 220)}, ac={0: _shuffled(jw.AC_SYMBOLS, 8, 221)})
    coef = _photo_blocks(w, h, S420, 43)
    tables = dict(dc={0: DC_FLAT, 1: _shuffled(jw.DC_SYMBOLS, 4, 222)}, ac={0: AC_FLAT, 1: _shuffled(jw.AC_SYMBOLS, 8, 223)},
                  comp_dc=[0, 1, 1], comp_ac=[0, 1, 1])
    merged = _write(coef, w, h, S420, thumbnail=thumb, comments=[b"time lapse", b"\xff\xd8\xff\xda is no marker here"],
                    fill={0xC4: 2, 0xC0: 1}, merge_tables=True, dri0=True, **tables)
    split = _write(coef, w, h, S420, comments=[b"one table per segment"], fill={0xDB: 1, 0xDA: 3}, merge_tables=False, **tables)
    return [Stream("headers", "headers merged thumbnail dri0", merged, "pixels", coef, S420),
            Stream("headers", "headers split", split, "pixels", coef, S420)]


FLAT_SIZES = ((531, 397), (736, 736))


def _flat():
    out = []
    for w, h in FLAT_SIZES:
        for sub, name in ((2, "420"), (0, "444")):
            for v, shade in ((0, "black"), (255, "white"), (128, "mid-gray")):
                data = jc.encode(np.full((h, w, 3), v, np.uint8), quality=75, subsampling=sub)
                out.append(Stream("flat", "flat %s %s %dx%d" % (shade, name, w, h), data, "pixels"))
    return out


def _out_of_range():
    rng = np.random.default_rng(105)
    a = [rng.integers(-1023, 1024, (n, n, 64)).astype(np.int16) for n in (6, 3, 3)]
    d1 = _write(a, 48, 48, S420, q={0: Q1}, comp_q=[0, 0, 0], dc={0: DC_FLAT_ALL}, ac={0: AC_FLAT_ALL})
    b = [(255 * rng.choice([-1, 1], (4, 4, 64))).astype(np.int16) for _ in range(3)]
    d2 = _write(b, 32, 32, S444, q={0: Q16}, comp_q=[0, 0, 0], dc={0: DC_FLAT_ALL}, ac={0: AC_FLAT_ALL})
    return [Stream("out-of-range", "out-of-range 1023 q1 420 48x48", d1, "out-of-range", a, S420),
            Stream("out-of-range", "out-of-range 255 q16 444 32x32", d2, "out-of-range", b, S444)]


ENTRIES = ("long-codes", "ff-runs", "two-bit-blocks", "full-blocks", "runs", "categories", "slots", "ri-1", "ri-edges",
           "big-interval", "headers", "flat", "out-of-range")


@functools.lru_cache(maxsize=None)
def catalogue():
    out = []
    for make in (_long_codes, _ff_runs, _two_bit_blocks, _full_blocks, _runs, _categories, _slots, _ri_1, _ri_edges,
                 _big_interval, _headers, _flat, _out_of_range):
        out += make()
    assert tuple(dict.fromkeys(s.entry for s in out)) == ENTRIES and len({s.label for s in out}) == len(out)
    return tuple(out)


def stream(label):
    return next(s for s in catalogue() if s.label == label)


@functools.lru_cache(maxsize=None)
def reference(label):
    """(info, per-component (blocks_y, blocks_x, 8, 8) coefficients, the same as one flat array in the package's layout)
    of the Python reader; read once per process and not to be written to"""
    info, planes = jr.coefficients(stream(label).data)
    flat = np.concatenate([p.reshape(-1) for p in planes])
    for a in planes + [flat]:
        a.setflags(write=False)
    return info, planes, flat


@functools.lru_cache(maxsize=None)
def pillow(label):
    a = jc.pil_decode(stream(label).data)
    a.setflags(write=False)
    return a


# ---- what a file's bytes say -----------------------------------------------------------------------------------------
def measure(data):
    """Walks the markers of a file on its own terms.  Returns a dict:
    markers     [(marker, offset of its FF, number of fill bytes in front)] up to SOS
    dht_bits    {(class, slot): the 16 counts};  dht: {(class, slot): {symbol: code length}}
    quant_slots, selectors [(DC slot, AC slot)] per component
    restart_interval, ncomp, blocks_per_mcu, mcus
    segments    [(begin, end)] of the entropy-coded data: end is the first byte that is no data (a fill byte, a marker)
    rst         [(offset of the marker's FF, fill bytes in front, n of RSTn)]
    scan_bytes  entropy-coded bytes, stuffed zeros included;  ff_pairs: FF 00 pairs among them
    ff_share    share of the entropy-coded bytes that belong to FF 00 pairs;  ff_run: most consecutive pairs
    """
    assert data[:2] == b"\xff\xd8"
    pos, m = 2, {"markers": [], "dht_bits": {}, "dht": {}, "restart_interval": 0}
    while True:
        fills = 0
        while data[pos + 1] == 0xFF:
            pos, fills = pos + 1, fills + 1
        assert data[pos] == 0xFF
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        m["markers"].append((marker, pos, fills))
        pos += 2 + n
        if marker == 0xC4:
            k = 0
            while k < len(body):
                bits = list(body[k + 1:k + 17])
                m["dht_bits"][(body[k] >> 4, body[k] & 15)] = bits
                vals = iter(body[k + 17:k + 17 + sum(bits)])
                m["dht"][(body[k] >> 4, body[k] & 15)] = {next(vals): n + 1 for n in range(16) for _ in range(bits[n])}
                k += 17 + sum(bits)
        elif marker == 0xDD:
            m["restart_interval"] = int.from_bytes(body, "big")
        elif marker == 0xC0:
            h, w, nc = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            hv = [(body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15) for c in range(nc)] if nc > 1 else [(1, 1)]
            m["ncomp"], m["blocks_per_mcu"] = nc, sum(a * b for a, b in hv)
            m["quant_slots"] = [body[8 + 3 * c] for c in range(nc)]
            m["mcus"] = -(-w // (8 * hv[0][0])) * -(-h // (8 * hv[0][1]))
        elif marker == 0xDA:
            m["selectors"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            break
    segments, rst, begin, pairs, run, best = [], [], pos, 0, 0, 0
    while True:
        if data[pos] != 0xFF:
            pos, run = pos + 1, 0
            continue
        if data[pos + 1] == 0:
            pos, pairs, run = pos + 2, pairs + 1, run + 1
            best = max(best, run)
            continue
        segments.append((begin, pos))
        run, fills = 0, 0
        while data[pos + 1] == 0xFF:
            pos, fills = pos + 1, fills + 1
        if not 0xD0 <= data[pos + 1] <= 0xD7:
            assert data[pos + 1] == 0xD9
            break
        rst.append((pos, fills, data[pos + 1] - 0xD0))
        pos += 2
        begin = pos
    nbytes = sum(e - b for b, e in segments)
    m.update(segments=segments, rst=rst, ff_share=2 * pairs / max(nbytes, 1), ff_run=best, scan_bytes=nbytes, ff_pairs=pairs)
    return m


def block_bits(label):
    """bits of every block of a file in scan order: the symbols of the coefficients the Python reader found, at the code
    lengths the file's own DHT segments state.  Their sum, padded per segment, must be the entropy-coded bytes."""
    s = stream(label)
    m = measure(s.data)
    info, planes, _ = reference(label)
    coef = [p.reshape(p.shape[0], p.shape[1], 64) for p in planes]
    ri = info["restart_interval"]
    out, pred = [], [0] * len(coef)
    for _, c, blk, first in jw.scan_order(coef, info["sampling"], ri):
        if first:
            pred = [0] * len(coef)
        td, ta = m["selectors"][c]
        out.append(sum(m["dht"][(0, td) if is_dc else (1, ta)][sym] + n for is_dc, sym, _, n in jw.block_symbols(blk, pred[c])))
        pred[c] = int(blk[0])
    return out

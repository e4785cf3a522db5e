"""A baseline JPEG writer for tests, written from ITU-T T.81 (markers B.1, frame and scan headers B.2.2 / B.2.3, tables
B.2.4, Huffman code assignment Annex C, the entropy coding of F.1.2), in plain Python and numpy.  It takes quantised
coefficients, not pixels, so a test decides every symbol of the scan; it shares nothing with Pillow's encoder, with
jpeg_restatement.py or with the package.

    write(coef, width, height, sampling, qtables, comp_q, dc_tables, ac_tables, comp_dc, comp_ac, ...) -> bytes
    blocks_from_pixels(img, sampling, qtables) -> coefficients an 8-bit encoder produces (float64 forward DCT, rounded)
    pixels_from_blocks(coef, sampling, qtables) -> 8-bit samples whose blocks_from_pixels may be asked to give `coef` back

A Huffman table is given as {symbol: code length}; the codes follow from the lengths (shorter first, symbols of one
length in the dictionary's order), as BITS / HUFFVAL say them.
"""
import numpy as np


def _zigzag():
    """natural (row-major) index of the k-th coefficient in zigzag order (T.81 Figure A.6)"""
    order = sorted(((r + c, (r if (r + c) % 2 else c), r * 8 + c) for r in range(8) for c in range(8)))
    return [n for _, _, n in order]


ZIGZAG = _zigzag()


# ---- Huffman tables --------------------------------------------------------------------------------------------------
def bits_huffval(lengths):
    """{symbol: length} -> (BITS: 16 counts, HUFFVAL: the symbols by increasing code length)"""
    bits, vals = [0] * 16, []
    for n in range(1, 17):
        for sym, ln in lengths.items():
            if ln == n:
                bits[n - 1] += 1
                vals.append(sym)
    if len(vals) != len(lengths):
        raise ValueError("code lengths are 1 to 16")
    return bits, vals


def codes(lengths):
    """{symbol: length} -> {symbol: (code, length)} (T.81 C.2); the all-ones code of 16 bits stays free"""
    bits, vals = bits_huffval(lengths)
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            if code >= (1 << n) - (n == 16):
                raise ValueError("more codes than the lengths leave room for")
            out[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return out


def flat_table(symbols, length):
    """every symbol on a code of the same length, in the order given"""
    return {s: length for s in symbols}


DC_SYMBOLS = list(range(12))                                                            # categories of 8-bit data
AC_SYMBOLS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]         # the 162 of 8-bit data
DC_SYMBOLS_ALL = list(range(16))
AC_SYMBOLS_ALL = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 16)]


# ---- the symbols of a block ------------------------------------------------------------------------------------------
def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, s):
    v = int(v)
    return v if v >= 0 else v + (1 << s) - 1


def block_symbols(blk, pred):
    """one block (64, natural order) -> [(is_dc, symbol, extra bits, number of extra bits)], T.81 F.1.2"""
    diff = int(blk[0]) - pred
    s = _category(diff)
    out = [(True, s, _value_bits(diff, s), s)]
    run = 0
    last = max((k for k in range(1, 64) if blk[ZIGZAG[k]]), default=0)
    for k in range(1, last + 1):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((False, 0xF0, 0, 0))
            run -= 16
        s = _category(v)
        out.append((False, run << 4 | s, _value_bits(v, s), s))
        run = 0
    if last < 63:
        out.append((False, 0x00, 0, 0))
    return out


def scan_order(coef, sampling, restart_interval=0):
    """the blocks in the order of the interleaved scan: yields (mcu, component, block, first of a restart interval)"""
    ncomp = len(coef)
    samp = [(1, 1)] if ncomp == 1 else sampling
    my, mx = coef[0].shape[0] // samp[0][1], coef[0].shape[1] // samp[0][0]
    for m in range(my * mx):
        j, i = divmod(m, mx)
        first = restart_interval > 0 and m % restart_interval == 0
        for c in range(ncomp):
            hs, vs = samp[c]
            for v in range(vs):
                for u in range(hs):
                    yield m, c, coef[c][j * vs + v, i * hs + u], first
                    first = False


def symbol_counts(coef, sampling, restart_interval=0):
    """how often the scan of these coefficients uses every DC and AC symbol, per component: ([{sym: n}], [{sym: n}])"""
    dc, ac = [dict() for _ in coef], [dict() for _ in coef]
    pred = [0] * len(coef)
    for _, c, blk, first in scan_order(coef, sampling, restart_interval):
        if first:
            pred = [0] * len(coef)
        for is_dc, sym, _, _ in block_symbols(blk, pred[c]):
            d = dc[c] if is_dc else ac[c]
            d[sym] = d.get(sym, 0) + 1
        pred[c] = int(blk[0])
    return dc, ac


# ---- the file --------------------------------------------------------------------------------------------------------
class _BitSink:
    """bits -> bytes, a zero stuffed behind every FF"""

    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        self.acc = self.acc << nbits | value
        self.n += nbits
        self.bits += nbits
        while self.n >= 8:
            self.n -= 8
            b = self.acc >> self.n & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self):
        """fills the last byte with 1-bits; returns the number of padding bits"""
        k = -self.n % 8
        if k:
            self.put((1 << k) - 1, k)
            self.bits -= k
        return k


def _segment(marker, body, fill=0):
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write(coef, width, height, sampling, qtables, comp_q, dc_tables, ac_tables, comp_dc, comp_ac, restart_interval=0,
          thumbnail=None, comments=(), fill=None, fill_rst=None, merge_tables=True, dri0=False, layout=None):
    """A baseline (SOF0) file with one interleaved scan.

    coef            per component, (blocks_y, blocks_x, 64) quantised coefficients in natural order, whole MCUs
    sampling        per component, (h, v)
    qtables         {slot: 64 values in natural order};  comp_q: per component, its slot
    dc_tables,
    ac_tables       {slot: {symbol: code length}};  comp_dc / comp_ac: per component, its slot
    thumbnail       a complete JPEG file, embedded in an APP1 segment behind an Exif header
    comments        COM segments' texts
    fill            {marker: number of fill bytes FF in front of every segment with this marker}
    fill_rst        {n: number of fill bytes in front of the n-th restart marker of the file (0, 1, ...)}
    merge_tables    all tables of a kind in one DQT / DHT segment, or a segment each
    dri0            a DRI segment that says "no restart intervals" (only with restart_interval 0)
    layout          a list that receives (data bits, padding bits) of every entropy-coded segment
    """
    fill, fill_rst = fill or {}, fill_rst or {}
    ncomp = len(coef)
    coef = [np.asarray(p) for p in coef]
    hmax, vmax = (1, 1) if ncomp == 1 else (max(h for h, _ in sampling), max(v for _, v in sampling))
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    for c, p in enumerate(coef):
        hs, vs = (1, 1) if ncomp == 1 else sampling[c]
        if p.shape != (my * vs, mx * hs, 64):
            raise ValueError("component %d: %r, expected %r" % (c, p.shape, (my * vs, mx * hs, 64)))

    def seg(marker, body):
        return _segment(marker, body, fill.get(marker, 0))

    out = bytearray(b"\xff\xd8")
    out += seg(0xE0, b"JFIF\x00\x01\x01\x01\x00\x48\x00\x48\x00\x00")
    if thumbnail is not None:
        tiff = b"II*\x00\x08\x00\x00\x00" + b"\x00\x00" + b"\x00\x00\x00\x00"      # an image file directory without entries
        out += seg(0xE1, b"Exif\x00\x00" + tiff + bytes(thumbnail))
    for text in comments:
        out += seg(0xFE, text)
    dqt = [bytes([slot]) + bytes(int(q[ZIGZAG[k]]) for k in range(64)) for slot, q in
           ((s, np.asarray(t).reshape(64)) for s, t in sorted(qtables.items()))]
    for body in ([b"".join(dqt)] if merge_tables else dqt):
        out += seg(0xDB, body)
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp]) +
               b"".join(bytes([c + 1, sampling[c][0] << 4 | sampling[c][1], comp_q[c]]) for c in range(ncomp)))
    dht = []
    for tc, tables in ((0, dc_tables), (1, ac_tables)):
        for slot, lengths in sorted(tables.items()):
            bits, vals = bits_huffval(lengths)
            codes(lengths)                                                          # raises when the lengths do not fit
            dht.append(bytes([tc << 4 | slot]) + bytes(bits) + bytes(vals))
    for body in ([b"".join(dht)] if merge_tables else dht):
        out += seg(0xC4, body)
    if restart_interval or dri0:
        out += seg(0xDD, restart_interval.to_bytes(2, "big"))
    out += seg(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, comp_dc[c] << 4 | comp_ac[c]]) for c in range(ncomp)) +
               bytes([0, 63, 0]))

    dc_codes = [codes(dc_tables[comp_dc[c]]) for c in range(ncomp)]
    ac_codes = [codes(ac_tables[comp_ac[c]]) for c in range(ncomp)]
    sink, pred, nrst, started = _BitSink(), [0] * ncomp, 0, False
    for _, c, blk, first in scan_order(coef, sampling, restart_interval):
        if first and started:
            k = sink.pad()
            if layout is not None:
                layout.append((sink.bits, k))
            out += sink.out
            out += b"\xff" * fill_rst.get(nrst, 0) + bytes([0xFF, 0xD0 + nrst % 8])
            sink, pred, nrst = _BitSink(), [0] * ncomp, nrst + 1
        started = True
        for is_dc, sym, extra, nextra in block_symbols(blk, pred[c]):
            code, n = (dc_codes if is_dc else ac_codes)[c][sym]
            sink.put(code << nextra | extra, n + nextra)
        pred[c] = int(blk[0])
    k = sink.pad()
    if layout is not None:
        layout.append((sink.bits, k))
    out += sink.out
    out += b"\xff\xd9"
    return bytes(out)


# ---- pixels <-> coefficients -----------------------------------------------------------------------------------------
def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    m = np.cos((2 * n + 1) * k * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m                                                                        # orthonormal: m @ m.T = 1


_D = _dct_matrix()


def ycbcr_from_rgb(rgb):
    """JFIF's full-range conversion in float64, rounded to 8 bits"""
    a = np.asarray(rgb, np.float64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = 128 - 0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 128 + 0.5 * r - 0.418688 * g - 0.081312 * b
    return np.clip(np.rint(np.stack([y, cb, cr], -1)), 0, 255).astype(np.uint8)


def blocks_from_pixels(img, sampling, qtables):
    """8-bit samples -> quantised coefficients as an encoder makes them, so in the range a forward DCT of 8-bit data
    gives.  img: H x W (one component) or H x W x 3 (Y Cb Cr at full size; `ycbcr_from_rgb` makes it of a photo);
    sampling: per component (h, v), chroma (1, 1) under luma (1, 1), (2, 1) or (2, 2); qtables: per component, 64
    values in natural order.  Planes are padded to whole MCUs by repeating the edge, chroma is averaged over 2x1 / 2x2
    boxes, the DCT is float64, the quotient is rounded to nearest."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError("8-bit samples expected")
    planes = [img] if img.ndim == 2 else [img[..., c] for c in range(3)]
    samp = [(1, 1)] if len(planes) == 1 else sampling
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    h, w = planes[0].shape
    ph, pw = -(-h // (8 * vmax)) * 8 * vmax, -(-w // (8 * hmax)) * 8 * hmax
    out = []
    for c, p in enumerate(planes):
        p = np.pad(p.astype(np.float64), ((0, ph - h), (0, pw - w)), mode="edge")
        fy, fx = vmax // samp[c][1], hmax // samp[c][0]
        if fy > 1 or fx > 1:
            p = np.rint(p.reshape(ph // fy, fy, pw // fx, fx).mean(axis=(1, 3)))
        by, bx = p.shape[0] // 8, p.shape[1] // 8
        blk = p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128.0
        f = _D @ blk @ _D.T
        q = np.asarray(qtables[c], np.float64).reshape(8, 8)
        out.append(np.rint(f / q).astype(np.int16).reshape(by, bx, 64))
    return out


def pixels_from_blocks(coef, sampling, qtables):
    """The way back, for content that is designed as coefficients and still has to come from pixels: a float64 inverse
    DCT of the dequantised blocks, rounded and clipped to 8 bits, chroma repeated to full size.  Whoever uses it checks
    that `blocks_from_pixels` of the result gives `coef` again."""
    samp = [(1, 1)] if len(coef) == 1 else sampling
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    planes = []
    for c, p in enumerate(coef):
        by, bx = p.shape[:2]
        f = p.reshape(by, bx, 8, 8).astype(np.float64) * np.asarray(qtables[c], np.float64).reshape(8, 8)
        s = np.clip(np.rint(_D.T @ f @ _D + 128.0), 0, 255).astype(np.uint8)
        s = s.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
        planes.append(np.repeat(np.repeat(s, vmax // samp[c][1], 0), hmax // samp[c][0], 1))
    return planes[0] if len(planes) == 1 else np.stack(planes, -1)

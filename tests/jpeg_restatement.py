"""Baseline JPEG decoding restated independently of the package: a pure-Python Huffman reader (one bit at a time, the
code tree of ITU-T T.81 Annex C / F as a dictionary) and the published integer arithmetic of libjpeg's default decoder
in numpy -- the 13-bit "islow" inverse DCT, "fancy" (triangle) chroma upsampling on the true plane sizes, the 16-bit
fixed-point YCbCr -> RGB.  Nothing here imports the package; tests compare it with Pillow (test_jpeg_host.py) and the
package with it.

    coefficients(data) -> info dict + per-component arrays (blocks_y, blocks_x, 8, 8) int16, natural order, not dequantised
    decode(data)       -> H x W x 3 (or H x W) uint8, what np.array(Image.open(...)) gives
"""
import numpy as np


class Unsupported(Exception):
    pass


def _zigzag():
    """natural (row-major) index of the k-th coefficient in zigzag order (T.81 Figure A.6), walked along the diagonals"""
    order = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]     # (row, col) on the diagonal row + col = s
        if s % 2 == 0:
            cells.reverse()                                          # even diagonals run upwards
        order += [r * 8 + c for r, c in cells]
    return order


ZIGZAG = _zigzag()


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            if self.p >= len(self.d):
                raise ValueError("scan data ends early")
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                if self.p >= len(self.d):
                    raise ValueError("scan data ends early")
                if self.d[self.p] != 0:
                    raise ValueError("marker inside the scan")
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code, length = 0, 0
        while True:
            code = (code << 1) | self.bit()
            length += 1
            s = table.get((length, code))
            if s is not None:
                return s
            if length >= 16:
                raise ValueError("no such Huffman code")

    def restart(self, expect):
        self.n = 0
        while self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xFF:    # fill bytes in front of the marker (T.81 B.1.1.2)
            self.p += 1
        if self.d[self.p] != 0xFF or self.d[self.p + 1] != 0xD0 + expect:
            raise ValueError("restart marker missing")
        self.p += 2


def _huffman_table(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(data):
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file")
    pos, qt, dc_tab, ac_tab, frame, ri = 2, {}, {}, {}, None, 0
    while True:
        while data[pos] == 0xFF and data[pos + 1] == 0xFF:
            pos += 1
        if data[pos] != 0xFF:
            raise ValueError("marker expected")
        m = data[pos + 1]
        n = (data[pos + 2] << 8) | data[pos + 3]
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xC0:
            if body[0] != 8:
                raise Unsupported("precision")
            h, w, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)]
            frame = (w, h, comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                counts = list(body[k + 1:k + 17])
                nsym = sum(counts)
                (ac_tab if tc else dc_tab)[th] = _huffman_table(counts, body[k + 17:k + 17 + nsym])
                k += 17 + nsym
        elif m == 0xDB:
            k = 0
            while k < len(body):
                if body[k] >> 4:
                    raise Unsupported("16-bit quantisation table")
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = list(body[k + 1:k + 65])
                qt[body[k] & 15] = t.reshape(8, 8)
                k += 65
        elif m == 0xDD:
            ri = (body[0] << 8) | body[1]
        elif m == 0xDA:
            break
    w, h, comps = frame
    if len(comps) not in (1, 3) or body[0] != len(comps):
        raise Unsupported("components")
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]       # a single-component scan is never interleaved
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    sel = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(len(comps))]
    planes = [np.zeros((my * c[2], mx * c[1], 64), np.int16) for c in comps]
    rd, pred, left, nrst = _Bits(data, pos), [0] * len(comps), ri, 0
    for j in range(my):
        for i in range(mx):
            if ri and left == 0:
                rd.restart(nrst & 7)
                nrst, left, pred = nrst + 1, ri, [0] * len(comps)
            left -= 1
            for c, (_, hs, vs, _) in enumerate(comps):
                for v in range(vs):
                    for u in range(hs):
                        blk = planes[c][j * vs + v, i * hs + u]
                        s = rd.symbol(dc_tab[sel[c][0]])
                        pred[c] += _extend(rd.bits(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = rd.symbol(ac_tab[sel[c][1]])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[ZIGZAG[k]] = _extend(rd.bits(s), s)
                            k += 1
    info = dict(width=w, height=h, ncomp=len(comps), hmax=hmax, vmax=vmax, mcus_x=mx, mcus_y=my, restart_interval=ri,
                sampling=[(c[1], c[2]) for c in comps], quant=[qt[c[3]] for c in comps])
    return info, [p.reshape(p.shape[0], p.shape[1], 8, 8) for p in planes]


# ---- arithmetic ------------------------------------------------------------------------------------------------------
def _idct_1d(x, shift):
    """8-point inverse DCT along axis -2 of int64 data (the factorisation of Loeffler, Ligtenberg and Moschytz with 13-bit
    constants), result descaled by `shift` with rounding"""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., k, :] for k in range(8))
    z = (x2 + x6) * 4433
    e2 = z - x6 * 15137
    e3 = z + x2 * 6270
    e0 = (x0 + x4) << 13
    e1 = (x0 - x4) << 13
    a0, a3, a1, a2 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    z1, z2, z3, z4 = x7 + x1, x5 + x3, x7 + x3, x5 + x1
    z5 = (z3 + z4) * 9633
    z3 = z5 - z3 * 16069
    z4 = z5 - z4 * 3196
    z1 = -z1 * 7373
    z2 = -z2 * 20995
    o0 = x7 * 2446 + z1 + z3
    o1 = x5 * 16819 + z2 + z4
    o2 = x3 * 25172 + z2 + z3
    o3 = x1 * 12299 + z1 + z4
    out = np.stack([a0 + o3, a1 + o2, a2 + o1, a3 + o0, a3 - o0, a2 - o1, a1 - o2, a0 - o3], -2)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, q):
    """(..., 8, 8) coefficients, (8, 8) table -> (..., 8, 8) samples 0..255"""
    x = coef.astype(np.int64) * q.astype(np.int64)
    x = _idct_1d(x, 11)                                             # columns: axis -2 is the row index
    x = np.swapaxes(_idct_1d(np.swapaxes(x, -1, -2), 18), -1, -2)   # rows
    return np.clip(x + 128, 0, 255).astype(np.uint8)


def _plane(blocks):
    by, bx = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _edge(a, axis, shift):
    """a shifted by one sample along `axis` with the edge sample repeated: shift -1 gives a[j-1], +1 gives a[j+1]"""
    idx = np.clip(np.arange(a.shape[axis]) + shift, 0, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def _up_h(s, r_even, r_odd, sh):
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + _edge(s, 1, -1) + r_even) >> sh
    out[:, 1::2] = (3 * s + _edge(s, 1, +1) + r_odd) >> sh
    return out


def upsample(p, hs, vs, fancy=True):
    """chroma plane of true size -> hs x vs times as large (hs, vs: luma sampling factors)"""
    p = p.astype(np.int64)
    if (hs, vs) == (1, 1):
        return p
    if not fancy:
        return np.repeat(np.repeat(p, vs, 0), hs, 1)
    if (hs, vs) == (2, 1):
        return _up_h(p, 1, 2, 2)
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    rows[0::2] = 3 * p + _edge(p, 0, -1)
    rows[1::2] = 3 * p + _edge(p, 0, +1)
    return _up_h(rows, 8, 7, 4)


def to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def planes_of(info, coef):
    """the component planes at their true sizes"""
    w, h, out = info["width"], info["height"], []
    for c, blocks in enumerate(coef):
        hs, vs = info["sampling"][c]
        cw, ch = -(-w * hs // info["hmax"]), -(-h * vs // info["vmax"])
        out.append(_plane(idct_blocks(blocks, info["quant"][c]))[:ch, :cw])
    return out


def decode(data):
    info, coef = coefficients(data)
    w, h = info["width"], info["height"]
    pl = planes_of(info, coef)
    if info["ncomp"] == 1:
        return pl[0]
    if info["sampling"][1] != (1, 1) or info["sampling"][2] != (1, 1) or info["sampling"][0] not in ((1, 1), (2, 1), (2, 2)):
        raise Unsupported("sampling factors")
    hs, vs = info["sampling"][0]
    # libjpeg takes the triangle filter only for planes wider than 2 samples
    fancy = pl[1].shape[1] > 2
    cb, cr = (upsample(p, hs, vs, fancy)[:h, :w] for p in pl[1:])
    return to_rgb(pl[0], cb, cr)


def gray(rgb, variant):
    """what cv2.cvtColor(BGR2GRAY) makes of an array in R G B order: channel 0 gets the "B" weight"""
    k0, k1, k2, sh = (3735, 19235, 9798, 15) if variant == 4 else (1868, 9617, 4899, 14)
    a = rgb.astype(np.int64)
    return ((a[..., 0] * k0 + a[..., 1] * k1 + a[..., 2] * k2 + (1 << (sh - 1))) >> sh).astype(np.uint8)

"""The PNG writer's filtered rows and the file's frame restated with numpy, zlib and struct, independent of the C code
(csrc/png_enc.h): `filtered(rgb)` is the stream the deflate block must hold, `parse_png(data)` takes a file apart, checks
everything around the compressed stream and inflates it with zlib, which also verifies the Adler-32."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered(rgb):
    """(H, W, 3) uint8 -> bytes: per row the filter type and the filtered row; of the five types the one with the smallest
    sum of absolute values of the bytes taken as signed 8-bit, ties to the lowest type; bpp = 3, zeros above row 0."""
    rgb = np.asarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    rows = rgb.reshape(h, 3 * w).astype(np.int64)
    out = np.empty((h, 1 + 3 * w), np.uint8)
    zero = np.zeros(3 * w, np.int64)
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else zero
        a = np.concatenate([zero[:3], x[:-3]])
        c = np.concatenate([zero[:3], b[:-3]])
        cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, c)]) & 255
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=1)
        t = int(np.argmin(cost))                      # the first of equal minima
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out.tobytes()


def parse_png(data):
    """The file's inflated IDAT; AssertionError for anything but signature, IHDR (8 bit, colour type 2, no interlace), ONE
    IDAT, IEND with right CRCs, a zlib header 78 01 and a single final fixed-Huffman block.  Returns (bytes, w, h)."""
    data = bytes(data)
    assert data[:8] == SIGNATURE
    chunks, pos = [], 8
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0) and chunks[2][1] == b""
    z = chunks[1][1]
    assert z[:2] == b"\x78\x01" and z[2] & 7 == 3      # BFINAL = 1, BTYPE = 01
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b""               # one block, nothing behind the Adler-32
    assert len(raw) == h * (1 + 3 * w)
    return raw, w, h

"""Inputs shared by test_jpeg_encode_host.py and test_gpu_jpeg_encode.py: a reader of a JPEG file's segments, the Huffman
tables of a file Pillow wrote (the standard ones of T.81 Annex K, taken from the file, not from the package), and
hand-made coefficient sets that drive the entropy coder to its edges, with the file tests/jpeg_writer.py makes of them."""
import io

import numpy as np
from PIL import Image

import jpeg_writer as jw

SAMPLING = {(1, 1): [(1, 1)] * 3, (2, 1): [(2, 1), (1, 1), (1, 1)], (2, 2): [(2, 2), (1, 1), (1, 1)]}


def segments(data):
    """[(marker, body)] up to and including SOS, and the entropy-coded bytes between SOS and EOI"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        out.append((m, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if m == 0xDA:
            return out, data[pos:-2]


def bodies(data, marker):
    return [b for m, b in segments(data)[0] if m == marker]


def pillow_file(mode="RGB", size=(40, 24), **kw):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    f = io.BytesIO()
    Image.fromarray(a).convert(mode).save(f, "JPEG", **kw)
    return f.getvalue()


def file_tables(data):
    """({slot: {symbol: length}} DC, the same AC) of a file's DHT segments, symbols in HUFFVAL order"""
    dc, ac = {}, {}
    for body in bodies(data, 0xC4):
        k = 0
        while k < len(body):
            tc, th = body[k] >> 4, body[k] & 15
            bits = body[k + 1:k + 17]
            vals = body[k + 17:k + 17 + sum(bits)]
            lengths, i = {}, 0
            for n in range(16):
                for _ in range(bits[n]):
                    lengths[vals[i]] = n + 1
                    i += 1
            (ac if tc else dc)[th] = lengths
            k += 17 + sum(bits)
    return dc, ac


def descriptor(width, height, quality=75):
    """a 4:2:0 JpegCoefficients of that size, all coefficients 0, with the re-save's tables"""
    from iceberg_tracking_code_amd import resave_coefficients
    j = resave_coefficients(np.zeros((height, width, 3), np.uint8), quality)
    j.coef[:] = 0
    return j


def writer_file(j):
    """tests/jpeg_writer.write of a 3-component JpegCoefficients, with the tables of a file Pillow wrote"""
    dc, ac = file_tables(pillow_file())
    i = j.info
    coef = [j.blocks(c).reshape(i.blocks_y[c], i.blocks_x[c], 64) for c in range(3)]
    return jw.write(coef, i.width, i.height, SAMPLING[(i.hmax, i.vmax)], {0: j.quant(0).reshape(64), 1: j.quant(1).reshape(64)},
                    [0, 1, 1], dc, ac, [0, 1, 1], [0, 1, 1], merge_tables=False)


def _scan_blocks(j):
    """the (component, block as a (64,) view) of a 4:2:0 descriptor in scan order"""
    i = j.info
    for my in range(i.mcus_y):
        for mx in range(i.mcus_x):
            for v in range(2):
                for u in range(2):
                    yield 0, j.blocks(0)[2 * my + v, 2 * mx + u].reshape(64)
            yield 1, j.blocks(1)[my, mx].reshape(64)
            yield 2, j.blocks(2)[my, mx].reshape(64)


def zero_mcu():
    return descriptor(16, 16)


def only_ac63():
    """every block: nothing but coefficient 63 -- a run of 62 (three ZRL, then run 14) and no EOB"""
    j = descriptor(32, 16)
    for k, (_, b) in enumerate(_scan_blocks(j)):
        b[63] = (-1) ** k * (1 + k)
    return j


def longest_blocks():
    """every block: all 63 AC coefficients at +-1023 and a DC difference of category 11 -- 1660 bits in chroma"""
    j = descriptor(48, 32)
    sign = np.where(np.arange(64) % 2, -1, 1)
    last = [0, 0, 0]
    for k, (c, b) in enumerate(_scan_blocks(j)):
        b[:] = 1023 * sign * (-1) ** k
        b[0] = -1024 if last[c] > 0 else 1023
        last[c] = int(b[0])
    return j


def dc_staircase():
    """DC alternating between 1023 and -1024 along every component's scan order: differences of +-2047, category 11"""
    j = descriptor(80, 48)
    last = [0, 0, 0]
    for c, b in _scan_blocks(j):
        b[0] = -1024 if last[c] > 0 else 1023
        last[c] = int(b[0])
    return j


def padded_ff():
    """the last Cr block ends in coefficient 63 = 1023 (ten 1-bits, no EOB) and the first DC is chosen so that the data
    ends inside a byte: the stream's last byte is FF through the 1-bit padding alone, and is stuffed like any other"""
    for dc in range(0, 64):
        j = descriptor(16, 16)
        j.blocks(0)[0, 0, 0, 0] = dc
        j.blocks(2)[0, 0, 7, 7] = 1023
        layout = []
        f = writer_file_layout(j, layout)
        bits, pad = layout[0]
        if 1 <= pad <= 7 and f[-4:] == b"\xff\x00\xff\xd9" and f[-5] != 0xFF:
            return j
    raise AssertionError("no such stream")


def writer_file_layout(j, layout):
    dc, ac = file_tables(pillow_file())
    i = j.info
    coef = [j.blocks(c).reshape(i.blocks_y[c], i.blocks_x[c], 64) for c in range(3)]
    return jw.write(coef, i.width, i.height, SAMPLING[(i.hmax, i.vmax)], {0: j.quant(0).reshape(64), 1: j.quant(1).reshape(64)},
                    [0, 1, 1], dc, ac, [0, 1, 1], [0, 1, 1], merge_tables=False, layout=layout)


def mostly_ff():
    """every block: 1023 behind runs of 15 zeros (symbol FA, sixteen bits of which fifteen are 1, then ten 1-bits) -- the codes
    with the most 1-bits the standard tables have; more than half of the stream's bytes are FF"""
    j = descriptor(64, 64)
    zz = jw.ZIGZAG
    for _, b in _scan_blocks(j):
        for k in (16, 32, 48):
            b[zz[k]] = 1023
        b[zz[63]] = 1023
    return j


CASES = {"zero_mcu": zero_mcu, "only_ac63": only_ac63, "longest_blocks": longest_blocks, "dc_staircase": dc_staircase,
         "padded_ff": padded_ff, "mostly_ff": mostly_ff}


def ac_without_code():
    j = descriptor(16, 16)
    j.blocks(1)[0, 0, 3, 3] = -1024
    return j


def dc_without_code():
    j = descriptor(32, 16)
    j.blocks(0)[0, 1, 0, 0] = 1024
    j.blocks(0)[1, 0, 0, 0] = -1024                         # the next luma block in scan order: a difference of -2048
    return j


def with_restarts():
    j = descriptor(32, 16)
    j.info.restart_interval = 1
    return j

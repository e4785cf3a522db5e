"""The forward half of baseline JPEG as Pillow's `img.save(f, "JPEG")` runs it (libjpeg at its defaults: 4:2:0 chroma,
the Annex K tables scaled by the quality, the "islow" integer DCT), restated in numpy from libjpeg's published description
-- independently of the package and of csrc/jpeg_fwd.h.  Nothing here imports the package; tests compare it with what
Pillow wrote (test_jpeg_resave_host.py) and the package with both.

    tables(quality)            -> (luma, chroma) 8 x 8 int32, natural order
    coefficients(rgb, quality) -> info dict + per-component arrays (blocks_y, blocks_x, 8, 8) int16 over the MCU-padded
                                  grid, in the form of jpeg_restatement.coefficients
    resave(rgb, quality)       -> the pixels of "save, then open" (jpeg_restatement's decoder run on these coefficients)
"""
import numpy as np

# ITU-T T.81 Annex K, tables K.1 and K.2
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61,
               12, 12, 14, 19, 26, 58, 60, 55,
               14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77,
               24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101,
               72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99,
               18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)


def tables(quality=75):
    """libjpeg's quality scaling: scale = 5000 / Q below 50, else 200 - 2 Q; (base * scale + 50) / 100 clamped to 1 .. 255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality 1 .. 100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int32) for t in (K1, K2))


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(a, rows, cols):
    """edge samples repeated down to `rows` rows and right to `cols` columns"""
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def _downsample(c, w, h):
    """full-resolution chroma plane -> its 2x2 downsampled, padded plane"""
    c = _pad(c, h + (h & 1), 16 * -(-w // 16))              # right: to the padded width; down: to an even height only
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)                  # 1, 2, 1, 2 along the output columns, from 1 in every row
    s = (s + bias[None, :]) >> 2
    return _pad(s, 8 * -(-s.shape[0] // 8), s.shape[1])     # then the last downsampled row, to a multiple of 8


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """8-point forward DCT along the last axis; `first`: the row pass"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def _blocks(plane, q):
    """padded plane (a multiple of 8 both ways) -> (by, bx, 8, 8) quantised coefficients"""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _fdct_1d(d, True)                                                     # rows: the last axis
    d = np.swapaxes(_fdct_1d(np.swapaxes(d, -1, -2), False), -1, -2)          # columns
    qv = q.astype(np.int64) << 3
    mag = (np.abs(d) + (qv >> 1)) // qv
    return (np.sign(d) * mag).astype(np.int16)


def coefficients(rgb, quality=75):
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    ql, qc = tables(quality)
    y, cb, cr = ycc(rgb)
    mx, my = -(-w // 16), -(-h // 16)
    rbx, rby = -(-w // 8), -(-h // 8)
    luma = np.zeros((2 * my, 2 * mx, 8, 8), np.int16)
    luma[:rby, :rbx] = _blocks(_pad(y, 8 * rby, 8 * rbx), ql)
    # dummy blocks, in the encoder's order inside an MCU (left to right, top to bottom): AC 0, DC of the block before
    if rbx < 2 * mx:
        luma[:rby, rbx, 0, 0] = luma[:rby, rbx - 1, 0, 0]
    if rby < 2 * my:
        luma[rby, 0::2, 0, 0] = luma[rby - 1, 1::2, 0, 0]                     # bottom left: the MCU's top right
        luma[rby, 1::2, 0, 0] = luma[rby - 1, 1::2, 0, 0]
    planes = [luma, _blocks(_downsample(cb, w, h), qc), _blocks(_downsample(cr, w, h), qc)]
    info = dict(width=w, height=h, ncomp=3, hmax=2, vmax=2, mcus_x=mx, mcus_y=my, restart_interval=0,
                sampling=[(2, 2), (1, 1), (1, 1)], quant=[ql, qc, qc])
    return info, planes


def resave(rgb, quality=75):
    """np.array(Image.open(f)) after Image.fromarray(rgb).save(f, "JPEG", quality=quality)"""
    import jpeg_restatement as jr
    info, coef = coefficients(rgb, quality)
    w, h = info["width"], info["height"]
    pl = jr.planes_of(info, coef)
    fancy = pl[1].shape[1] > 2
    cb, cr = (jr.upsample(p, 2, 2, fancy)[:h, :w] for p in pl[1:])
    return jr.to_rgb(pl[0], cb, cr)

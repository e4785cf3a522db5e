"""JPEG files for the decoder tests, made with Pillow from seeded pixels (shared by test_jpeg_host.py and
test_gpu_jpeg.py).  Every case is (label, bytes)."""
import io

import numpy as np
from PIL import Image


def photo(w, h, seed=0, channels=3):
    """smooth colour ramps + a few hard edges + a little noise: every frequency gets coefficients"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3), np.float64)
    img[..., 0] = 128 + 100 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0)
    img[..., 1] = (x * 255.0 / max(w - 1, 1) + y * 3) % 256
    img[..., 2] = 255.0 * (((x // 6) + (y // 5)) % 2)
    img += rng.normal(0, 12, img.shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img if channels == 3 else img[..., 0].copy()


def edges(w, h, seed=5):
    """hard black / white edges and full-range noise in one channel: with quality 100 both clamps (inverse DCT and
    colour conversion) have work to do"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3), np.uint8)
    bw = (255 * (((x // 3) + (y // 4)) % 2)).astype(np.uint8)
    img[..., 0] = bw
    img[..., 1] = 255 - bw
    img[..., 2] = rng.integers(0, 2, (h, w)) * 255
    return img


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.array(Image.open(io.BytesIO(data)))


SIZES = [(16, 16), (37, 29), (33, 17), (8, 8), (50, 47), (1, 1), (17, 1)]   # (w, h)


def matrix(min_width=1, heights=range(1, 36)):
    """The matrix the arithmetic was pinned on: widths 16 and 23 at every height 1..35, the sizes above, subsampling
    4:4:4 / 4:2:2 / 4:2:0, quality 30 / 75 / 95 / 100 with optimize on and off, restart markers, a comment, gray files."""
    out = []
    for sub in (0, 1, 2):
        for w in (16, 23):
            for h in heights:
                out.append(("%dx%d s%d" % (w, h, sub), encode(photo(w, h), quality=75, subsampling=sub)))
        for w, h in SIZES:
            if w >= min_width:
                out.append(("%dx%d s%d" % (w, h, sub), encode(photo(w, h, 1), quality=75, subsampling=sub)))
        for q in (30, 75, 95, 100):
            for opt in (False, True):
                out.append(("37x29 s%d q%d opt%d" % (sub, q, opt),
                            encode(photo(37, 29, 2), quality=q, subsampling=sub, optimize=opt)))
        out.append(("37x29 s%d rst-blocks" % sub, encode(photo(37, 29, 3), quality=90, subsampling=sub, restart_marker_blocks=3)))
        out.append(("50x47 s%d rst-rows" % sub, encode(photo(50, 47, 3), quality=90, subsampling=sub, restart_marker_rows=1)))
        out.append(("33x17 s%d comment" % sub, encode(photo(33, 17, 4), quality=85, subsampling=sub, comment=b"time lapse")))
    for w, h in SIZES + [(23, 35)]:
        if w >= min_width:
            out.append(("%dx%d gray" % (w, h), encode(photo(w, h, 6, channels=1), quality=80)))
    return out

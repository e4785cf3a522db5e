"""Inputs and the Pillow oracle shared by test_jpeg_resave_host.py and test_gpu_jpeg_resave.py."""
import io

import numpy as np
from PIL import Image

# (width, height): a single pixel, less than a block, exact blocks and MCUs, one row / column more than an MCU, heights
# with h mod 16 in 2..8 and 10..15 (where chroma is NOT padded to 16 rows before downsampling), odd sizes, more than one
# strip of 16 MCUs across (250 > 256 - 16 is still one; 333 rows make 21 MCU rows)
SIZES = ((1, 1), (3, 3), (8, 8), (16, 16), (16, 17), (17, 33), (24, 24), (33, 16), (40, 56), (41, 7), (64, 50), (99, 131), (250, 333))
# the device's: width >= 3; 640 x 480 has three strips across, the last one partial (40 = 16 + 16 + 8 MCUs)
GPU_SIZES = ((3, 3), (8, 8), (16, 17), (17, 33), (33, 16), (40, 56), (41, 7), (99, 131), (250, 333), (640, 480))
CONTENTS = ("noise", "ramp", "smooth", "zeros", "full", "stripes")
CROP = (3, 5, 6, 7)            # left, top, right, bottom: odd, no multiples of 8
PHOTO_SIZE = (131, 99)         # width, height


def content(kind, w, h, seed=0):
    """h x w x 3 uint8"""
    rng = np.random.default_rng([seed, w, h, CONTENTS.index(kind)])
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        return np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, (7 * x + 2 * y) % 256], -1).astype(np.uint8)
    if kind == "smooth":
        f = [127 + 100 * np.sin(x / (5.0 + c) + c) * np.cos(y / (7.0 - c)) for c in range(3)]
        return np.clip(np.stack(f, -1) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "stripes":                                  # saturated primaries (and their complements) in 8-pixel stripes
        colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 255, 255], [255, 0, 255], [255, 255, 0]], np.uint8)
        return colours[((x // 8) + 2 * (y // 8)) % 6]
    raise ValueError(kind)


def pillow_save(rgb, quality=None):
    """the bytes Image.fromarray(rgb).save(f, "JPEG"[, quality=quality]) writes"""
    f = io.BytesIO()
    if quality is None:
        Image.fromarray(rgb).save(f, "JPEG")
    else:
        Image.fromarray(rgb).save(f, "JPEG", quality=quality)
    return f.getvalue()


def pillow_open(data):
    return np.array(Image.open(io.BytesIO(data)))


def photo_file(seed=3, size=PHOTO_SIZE, quality=90):
    """a camera photo as a file: smooth content with noise, 4:2:0, as the cameras write it"""
    w, h = size
    f = io.BytesIO()
    Image.fromarray(content("smooth", w, h, seed)).save(f, "JPEG", quality=quality, subsampling=2)
    return f.getvalue()


def reference_crop_resave(inpath, outpath, crop):
    """crop_image_standalone of the reference (camtools.py:64-104), call for call, for a file that is not truncated"""
    left, top, right, bottom = crop
    img = Image.open(inpath)
    width, height = img.size                               # pic['width'], pic['height'] of the calibration workbook
    img_crop = img.crop((left, top, width - right, height - bottom))
    img_crop.save(outpath)

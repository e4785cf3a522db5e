"""Sources, crop boxes and the Pillow oracle shared by test_jpeg_crop_fwd_host.py and test_gpu_jpeg_crop_fwd.py: the fused
crop-and-forward kernel (csrc/k_jpeg_fwd.hip: k_jpeg_crop_fwd) and its host statement (csrc/jpeg_crop_fwd_host.h)."""
import functools
import io

import numpy as np
from PIL import Image

import jpeg_resave_cases as rc

W, H = 667, 501                                            # neither a multiple of 16: true plane edges inside the last MCU
SUBSAMPLING = {"420": 2, "422": 1, "444": 0}               # Pillow's `subsampling=`
NARROW = (4, 9)                                            # chroma planes 2 samples wide: libjpeg replicates (modes 3 / 4)

# (left, top, width, height) in a W x H source
BOXES = (
    # the four parities of the origin, the smallest crop the device takes
    (1, 1, 3, 3), (2, 1, 3, 3), (1, 2, 3, 3), (2, 2, 3, 3),
    # the sizes: 200 x 9, 176 x 16 (exact MCUs), 272 x 33 (a second strip of one MCU across, one row into a third MCU row),
    # 640 x 480 (three strips, the last one partial), strictly inside
    (5, 7, 200, 9), (8, 16, 176, 16), (3, 4, 272, 33), (13, 11, 640, 480),
    # heights with h mod 16 = 3, 7, 8, 13 (0, 1 and 9 are above)
    (21, 30, 33, 19), (10, 3, 41, 23), (6, 9, 64, 24), (17, 12, 99, 29),
    # flush with the true image edges: left + top, right + bottom, each edge alone, the whole image
    (0, 0, 272, 33), (W - 200, H - 9, 200, 9), (W - 176, 40, 176, 16), (20, H - 33, 272, 33), (0, 9, 200, 9), (9, 0, 176, 16),
    (0, 0, W, H),
)
QUALITY_BOX = (3, 4, 272, 33)                              # also at quality 50 and 100
NARROW_BOXES = ((0, 0, 3, 9), (1, 2, 3, 5), (1, 0, 3, 8))


def _pixels(w, h):
    """smooth content with noise; the right third saturated primaries, where the colour matrix clamps"""
    a = rc.content("smooth", w, h, seed=11)
    b = rc.content("stripes", w, h, seed=11)
    x = np.arange(w)[None, :, None]
    return np.where(x >= 2 * w // 3, b, a).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def source(sampling, narrow=False):
    """the bytes of a source photo"""
    w, h = NARROW if narrow else (W, H)
    f = io.BytesIO()
    Image.fromarray(_pixels(w, h)).save(f, "JPEG", quality=90, subsampling=SUBSAMPLING[sampling])
    return f.getvalue()


def crop4(data_size, box):
    """(left, top, width, height) -> the library's (left, top, right, bottom)"""
    (w, h), (left, top, bw, bh) = data_size, box
    return (left, top, w - left - bw, h - top - bh)


def pillow_crop_file(data, box, quality=None):
    """the bytes Image.open(f).crop(box).save(out) writes -- the reference's crop step (camtools.py:64-104)"""
    left, top, bw, bh = box
    im = Image.open(io.BytesIO(data)).crop((left, top, left + bw, top + bh))
    f = io.BytesIO()
    if quality is None:
        im.save(f, "JPEG")
    else:
        im.save(f, "JPEG", quality=quality)
    return f.getvalue()


def cases():
    """(label, source bytes, source size, box, quality or None) of every case of the issue"""
    out = []
    for s in SUBSAMPLING:
        for box in BOXES:
            out.append(("%s-%d_%d_%dx%d" % ((s,) + box), source(s), (W, H), box, None))
    for q in (50, 100):
        out.append(("420-q%d" % q, source("420"), (W, H), QUALITY_BOX, q))
    for s in ("420", "422"):
        for box in NARROW_BOXES:
            out.append(("narrow%s-%d_%d_%dx%d" % ((s,) + box), source(s, True), NARROW, box, None))
    return out

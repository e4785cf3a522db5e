"""Frames just large enough to hold every arm of the strip corner kernel (k_eig_strip, csrc/k_corners.hip) -- TEST HARNESS.

A workgroup takes one of three bodies: FRESH (the strip touches the top or bottom of the frame), rolling, and -- where all
output columns of the strip are inside the frame and no mask and no map is asked for -- rolling with the row phase that tests
nothing per pixel.  Inside every body a wave takes the square root in its band or, if one radicand of the wave is outside it
(0 over flat ground), sqrtf.

  760 x 130          four strips in x (three whole, with the reflected left edge among them, and the narrower last one), three
                     in y (top and bottom FRESH, one rolling)
  247 / 248 x 130    one strip, around TW
  40 x 40            smaller than a strip
  rounding(...)      box_sum_frames.frame content (kinds whose box sums round), stacked to the height asked for
  dots(bs)           isolated bright pixels whose windows straddle covariance columns 63/64, 127/128 and 191/192 of the first
                     interior strip (the seams between the four waves of a workgroup), in the rolling strip
  half_flat(bs)      the dots above, constant ground below: radicand 0 in the lower strips
  flat()             one value everywhere
  stripes()          random columns, constant down the frame: dy is exactly 0, so every eigenvalue is a - sqrt(a * a) = +0 while
                     every radicand is an ordinary positive number: the maximum is +0 and every wave takes the root in its band
  stripes_dots(bs)   the dots on the stripes: positive eigenvalues, no zero radicand, every box sum still exact
The flat ground of flat(), dots() and half_flat() has radicand 0 in every 256-column row, so on those every wave takes sqrtf;
the band's arm runs on stripes(), stripes_dots() and the rounding frames.
Numpy only.  References are computed once per session and are read-only (box_sum_frames.references does the same)."""
import numpy as np

import box_sum_frames as B
import np_restatement as R

W, H = 760, 130
# (label, seed, kind, width, height, block sizes)
ROUNDING = [
    ("wide-pm1", 18, "pm1", W, H, (3, 5, 7, 10)),
    ("tw-247", 48, "pm1", 247, H, (10,)),
    ("tw-248", 121, "pm3", 248, H, (10,)),
    ("small", 180, "pm3", 40, 40, (3, 10)),
]


def rounding(seed, kind, w, h):
    """texture / near-flat bands of box_sum_frames.frame, repeated with following seeds until h rows are there"""
    parts, rows, k = [], 0, 0
    while rows < h:
        parts.append(B.frame(seed + 7 * k, kind, w=w, above=bool(k % 2)))
        rows += parts[-1].shape[0]
        k += 1
    return np.ascontiguousarray(np.concatenate(parts)[:h])


def seam_columns(bs):
    """image x of covariance columns 63/64, 127/128, 191/192 of strip 1 in x"""
    c = B.strip_cfg(bs)
    xs = c["TW"] - 1 - bs // 2
    return [xs + j for j in (63, 64, 127, 128, 191, 192)]


def dots(bs, h=H, lower_flat=False):
    c = B.strip_cfg(bs)
    img = np.full((h, W), 17, np.uint8)
    ys = [c["SH"] + 6 + 9 * k for k in range(6)]          # rows of the rolling strip (strip 1 in y), windows apart
    for k, x in enumerate(seam_columns(bs)):
        img[ys[k % len(ys)] if not lower_flat else 8 + 9 * k, x] = 255
        img[(ys[(k + 3) % len(ys)] if not lower_flat else 8 + 9 * ((k + 3) % 6)), x + 2 * bs + 3] = 200 + k
    if lower_flat:
        img[h // 2:] = 17
    return img


def half_flat(bs):
    return dots(bs, lower_flat=True)


def flat():
    return np.full((H, W), 93, np.uint8)


def stripes():
    return np.ascontiguousarray(np.repeat(np.random.RandomState(3).randint(0, 256, (1, W)), H, axis=0).astype(np.uint8))


def stripes_dots(bs):
    img, d = stripes(), dots(bs)
    img[d != 17] = d[d != 17]
    return img


def ordered_key(v):
    """corner_keys.h's order-preserving key of a float32"""
    b = int(np.array([v], np.float32).view(np.uint32)[0])
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


_refs = {}


def references(label, bs):
    """img, exact, bound, term, running of a ROUNDING frame at one block size"""
    key = (label, bs)
    if key not in _refs:
        _, seed, kind, w, h, _ = next(e for e in ROUNDING if e[0] == label)
        img = rounding(seed, kind, w, h)
        r = dict(img=img, bs=bs, exact=B.exact_map(img, bs), bound=B.bound(img, bs), term=R.min_eig_map(img, bs),
                 running=B.running_map(img, bs))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = r
    return _refs[key]


CASES = [(label, bs) for label, _, _, _, _, sizes in ROUNDING for bs in sizes]

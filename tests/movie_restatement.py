"""The movie's scaler restated in numpy, written from DESIGN.md 7.11 and not from csrc/resize.h: Pillow's
`Image.resize(size, Image.BICUBIC)` on an 8-bit R G B image, and the size rule of the movie.  Whole-array arithmetic: the
weights of an axis as one (out, taps) matrix in float64, the fixed-point sums as one int32 matrix product per pass.  The
cases of the host and the GPU tests are listed here so that both run the same ones."""
import numpy as np

# (w, h) -> (ow, oh): one tap, 1025 taps, enlargement and reduction, a skipped pass on either axis, widths that are no
# multiples of 4, and thin slices of the real sizes (1200 and 1400 wide pictures, the movie 2000 wide)
CASES = [((1, 1), (16, 16)), ((2, 3), (16, 16)), ((5, 7), (3, 16)), ((37, 23), (64, 48)), ((64, 48), (37, 23)), ((33, 17), (33, 32)),
         ((257, 130), (31, 16)), ((1200, 13), (2000, 16)), ((1400, 40), (2000, 64)), ((4099, 5), (16, 16))]
FILLS = ("random", "extremes", "zeros", "ones")


def pixels(size, fill, seed=0):
    """The (h, w, 3) uint8 test picture of a case: random, random 0 / 255 (the overshoot then clips at both ends), all 0, all 255"""
    w, h = size
    rng = np.random.default_rng([seed, w, h, FILLS.index(fill)])
    if fill == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if fill == "extremes":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return np.full((h, w, 3), 0 if fill == "zeros" else 255, np.uint8)


def movie_size(w, h, width=2000):
    mw = int(width) if width > 0 else int(w)
    return mw, max(16, (mw * int(h) // int(w) + 8) // 16 * 16)


def _cubic(x):
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def axis_table(n_in, n_out):
    """(first (out,), K (out, in) int32): output o is sum K[o, s] source[s]; K is zero outside an output's taps"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    center = (np.arange(n_out) + 0.5) * scale
    first = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    end = np.minimum(n_in, np.trunc(center + support + 0.5).astype(np.int64))
    taps = int((end - first).max())
    j = np.arange(taps)[None, :]
    live = j < (end - first)[:, None]
    w = np.where(live, _cubic((j + first[:, None] - center[:, None] + 0.5) * (1.0 / fs)), 0.0)
    ww = np.zeros(n_out)
    for t in range(taps):                      # the sum in index order
        ww = ww + w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.trunc(w * float(1 << 22) + np.where(w < 0, -0.5, 0.5)).astype(np.int64)
    K = np.zeros((n_out, n_in), np.int64)
    rows = np.repeat(np.arange(n_out), taps).reshape(n_out, taps)
    cols = np.minimum(first[:, None] + j, n_in - 1)
    np.add.at(K, (rows[live], cols[live]), k[live])
    return first, end, K


def _pass(K, a):
    """K (out, in) over axis 0 of a (in, ...) uint8 -> (out, ...) uint8; the sums stay below 2^31 as the C code's do"""
    acc = np.tensordot(K, a.astype(np.int64), axes=(1, 0)) + (1 << 21)
    assert np.abs(acc).max() < 1 << 31
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize(rgb, size):
    """(h, w, 3) uint8 -> (oh, ow, 3) uint8 for size = (ow, oh)"""
    a = np.asarray(rgb)
    h, w = a.shape[:2]
    ow, oh = size
    if w != ow:
        a = _pass(axis_table(w, ow)[2], a.transpose(1, 0, 2)).transpose(1, 0, 2)
    if h != oh:
        a = _pass(axis_table(h, oh)[2], a)
    return np.ascontiguousarray(a)

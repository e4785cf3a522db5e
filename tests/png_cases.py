"""The pictures the PNG tests share (tests/test_png_host.py on the CPU, tests/test_gpu_png.py on the device), all built by
seeded numpy: name -> (H, W, 3) uint8.  SEGMENT is the coder's segment size (csrc/png_enc.h: kSegment); a filtered
stream has N = H (1 + 3 W) bytes."""
import functools

import numpy as np

SEGMENT = 4096
ZERO_RUNS = (2, 3, 257, 258, 259, 516)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _zero_run(length):
    """One row whose bytes alternate 30 and 226 -- filter None costs 30 a byte, Sub and Paeth 60, Average more, Up ties with
    None and loses: the filtered row is the row -- with `length` zero bytes from byte 31 on."""
    row = np.where(np.arange(600) % 2 == 0, 30, 226).astype(np.uint8)
    row[31:31 + length] = 0
    return row.reshape(1, 200, 3)


def _row_pair(w, seed):
    """Two rows whose Sub residuals are small signed noise r (1 .. 8 and -8 .. -1): row 0 the running sums of r, row 1 row 0
    plus 100.  Both rows take Sub (None, Up and Average cost far more, Paeth predicts the left neighbour and loses the tie),
    so from its second pixel on a filtered byte of row 1 equals the byte one row pitch before it, while distances 1 and 3
    match rarely."""
    rng = np.random.default_rng(seed)
    r = rng.integers(1, 9, (w, 3)) * rng.choice([-1, 1], (w, 3))
    row = np.cumsum(r, axis=0)
    return np.stack([row & 255, (row + 100) & 255]).astype(np.uint8)


def _map():
    import map_cases as mc
    import thumb_cases as tc
    import thumb_restatement as T
    pic, base = mc.case(64, 2, 0)
    return np.ascontiguousarray(T.paste(base, tc.inset_cases(64, pic["height"])["corners"]))


def _ramp(h, w, axis):
    i = np.arange(h)[:, None, None] if axis == 0 else np.arange(w)[None, :, None]
    return np.broadcast_to((i * np.array([1, 2, 3]) + np.array([0, 50, 100])) & 255, (h, w, 3)).astype(np.uint8)


def _checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    on = ((y // 2 + x // 2) % 2).astype(bool)
    return np.where(on[..., None], np.array([200, 60, 10]), np.array([20, 130, 250])).astype(np.uint8)


BUILDERS = {
    "1x1": lambda: _noise(1, 1, 1), "1x7": lambda: _noise(7, 1, 2), "7x1": lambda: _noise(1, 7, 3),
    "zero 512x64": lambda: np.zeros((64, 512, 3), np.uint8),
    "colour 512x64": lambda: np.broadcast_to(np.array([17, 200, 93], np.uint8), (64, 512, 3)).copy(),
    "noise 64x48": lambda: _noise(48, 64, 4),
    "horizontal ramp": lambda: _ramp(37, 101, 1), "vertical ramp": lambda: _ramp(101, 37, 0),
    "checkerboard": lambda: _checker(33, 47),
    "N = segment": lambda: _noise(16, 85, 5),               # 16 * 256
    "N = segment - 1": lambda: _noise(45, 30, 6),            # 45 * 91
    "N = segment + 1": lambda: _noise(17, 80, 7),            # 17 * 241
    "N = 2 segments": lambda: _checker(32, 85),              # 32 * 256
    "rows straddle segments": lambda: _ramp(5, 1366, 1),     # pitch 4099: every row holds a segment start
    "pitch 32767": lambda: _row_pair(10922, 8),
    "pitch 32770": lambda: _row_pair(10923, 8),
    "map": _map,
}
BUILDERS.update({"zero run %d" % n: functools.partial(_zero_run, n) for n in ZERO_RUNS})
NAMES = list(BUILDERS)
LARGEST = "zero 512x64"      # the most filtered bytes but for the two long-row pictures; "pitch 32767" has the longest rows


@functools.lru_cache(maxsize=None)
def case(name):
    a = np.ascontiguousarray(BUILDERS[name](), dtype=np.uint8)
    a.setflags(write=False)
    return a


def stream_bytes(a):
    return a.shape[0] * (1 + 3 * a.shape[1])

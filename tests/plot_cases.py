"""Frames and the hand-built track table that tests/test_plot_host.py and tests/test_gpu_plot.py share: every shape is
drawn by the code under test and by tests/plot_restatement.py, and the two must agree in every byte."""
import functools

import numpy as np

# (w, h, width asked for)
SHAPES = [(64, 48, 24),       # a non-integer ratio, 2.67
          (37, 29, 16),       # both dimensions prime
          (50, 37, 50),       # scale 1: the background is the frame itself
          (4000, 8, 1200)]    # wide and flat: Ho = 2, many background chunks per row
VERTICES = (2, 3, 5)
STAMPS = {2: "2019-07-14 12:30:05 120/60 ....",   # runs off the right edge of the small pictures
          3: "",
          5: "12:30"}


def frame(w, h, seed=7):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8)


def _polyline(p, q, vertices, reverse=False):
    """p .. q in `vertices` vertices: the interior ones lie on the chord, pushed 1.3 px off it to alternate sides; reverse:
    out to q and back to p (needs 3 vertices, else it is the chord)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if reverse and vertices >= 3:
        half = vertices // 2
        return [tuple(p + (q - p) * min(k, vertices - 1 - k) / half) for k in range(vertices)]
    d = q - p
    n = np.array([-d[1], d[0]]) / (np.hypot(*d) or 1.0)
    pts = []
    for k in range(vertices):
        off = 0.0 if k in (0, vertices - 1) else (1.3 if k % 2 else -1.3)
        pts.append(tuple(p + d * k / (vertices - 1) + n * off))
    return pts


def track_table(w, h, width, vertices):
    """(n, vertices, 2) float32 in frame pixels"""
    wo = min(width, w)
    T = []

    def both(p, q):
        T.append(_polyline(p, q, vertices))
        T.append(_polyline(q, p, vertices))

    both((0.1 * w, 0.2 * h), (0.8 * w, 0.2 * h))                     # horizontal
    both((0.7 * w, 0.1 * h), (0.7 * w, 0.9 * h))                     # vertical
    d = 0.4 * min(w, h)
    both((0.2 * w, 0.3 * h), (0.2 * w + d, 0.3 * h + d))             # 45 degrees, down
    both((0.2 * w, 0.9 * h), (0.2 * w + d, 0.9 * h - d))             # 45 degrees, up
    both((0.15 * w, 0.4 * h), (0.75 * w, 0.5 * h))                   # shallow
    both((0.4 * w, 0.15 * h), (0.5 * w, 0.75 * h))                   # steep
    T.append([(0.5 * w, 0.5 * h)] * vertices)                        # zero length
    T.append([(0.3 * w + 0.2 * k / (vertices - 1), 0.6 * h + 0.1 * k / (vertices - 1)) for k in range(vertices)])   # < 1 output pixel
    T.append(_polyline((0.25 * w, 0.7 * h), (0.6 * w, 0.8 * h), vertices, reverse=True))   # reverses
    inside = (0.45 * w, 0.45 * h)
    for start in ((-0.3 * w, 0.5 * h), (1.3 * w, 0.35 * h), (0.55 * w, -0.4 * h - 3), (0.35 * w, 1.5 * h + 3)):
        T.append(_polyline(start, inside, vertices))                 # from outside in, every side
    T.append(_polyline((-0.2 * w, 0.3 * h), (1.2 * w, 0.7 * h), vertices))     # through the picture, both ends outside
    T.append(_polyline((-50.0, -50.0), (-10.0, -20.0), vertices))    # wholly outside
    T.append(_polyline((w + 5.0, h + 5.0), (w + 40.0, h + 90.0), vertices))
    T.append(_polyline((-30.0, 0.5 * h), (-30.0, 2.0 * h), vertices))
    # vertices whose coordinate is exactly a pixel centre, 256 c + 128: (x + 0.5) wo / w = c + 0.5
    cx = 1.5 * w / wo - 0.5
    T.append(_polyline((cx, 2.0), (cx + 4.0 * w / wo, 2.0), vertices))
    T.append(_polyline((5.0, 3.0), (11.0, 3.0), vertices))           # integers: centres at scale 1
    # left out whole: a vertex that is not finite, or 2^20; drawn: one just below 2^20
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20):
        t = _polyline((0.1 * w, 0.1 * h), (0.9 * w, 0.85 * h), vertices)
        t[-1] = (bad, t[-1][1])
        T.append(t)
        t = _polyline((0.9 * w, 0.1 * h), (0.1 * w, 0.85 * h), vertices)
        t[vertices // 2] = (t[vertices // 2][0], bad)
        T.append(t)
    t = _polyline((0.1 * w, 0.3 * h), (0.5 * w, 0.35 * h), vertices)
    t[-1] = (2.0 ** 20 - 1.0, -(2.0 ** 20) + 1.0)
    T.append(t)
    # 40 tracks ending in one pixel: counts beyond 31
    end = (0.6 * w + 0.25, 0.3 * h + 0.25)
    for k in range(40):
        a = 2 * np.pi * k / 40
        T.append(_polyline((end[0] + 0.3 * w * np.cos(a), end[1] + 0.3 * h * np.sin(a)), end, vertices))
    return np.array(T, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(w, h, width, vertices):
    """(gray, tracks, stamp, the restatement's picture): computed once, shared, never written to"""
    import plot_restatement as R
    g, t, s = frame(w, h), track_table(w, h, width, vertices), STAMPS[vertices]
    ref = R.overlay(g, t, width, s)
    for a in (g, t, ref):
        a.setflags(write=False)
    return g, t, s, ref

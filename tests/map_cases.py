"""The pictures the map tests share (tests/test_map_host.py on the CPU, tests/test_gpu_map.py on the device): small
pictures with one view and with two, holding every kind of item at and beyond the edges of the rules of DESIGN.md 7.7.
`case(width, views, variant)` gives (picture dict, the restatement's R G B); the restatement runs once per case."""
import functools

import numpy as np

import map_restatement as R

WIDTHS = (64, 96, 160)
VIEWS = (1, 2)
# per variant, per panel: (arrow width in metres, pivot, alpha).  A pixel is 10 m: widths of 10, 20 and 100 m give shafts
# 1, 2 and 7 pixels thick (100 m: 10 pixels, clamped), and 100 m a head that the 48-pixel cap cuts (5 x 10 pixels)
VARIANTS = (((10.0, "tail", 1.0), (20.0, "mid", 0.75)), ((20.0, "mid", 0.75), (100.0, "tail", 1.0)), ((100.0, "tail", 1.0), (10.0, "mid", 1.0)))
VMAX = 0.5
M = 10.0                       # metres per pixel
X0, Y0 = 500000.0, 7000000.0   # UTM-sized numbers


def table():
    """a colour table of the test's own: no two entries alike"""
    k = np.arange(256)
    return np.stack([k, 255 - k, (k * 7) % 256], 1).astype(np.uint8)


def views_of(width, n):
    """rectangles of the test's own: n views side by side, a bar 4 wide right of each"""
    height = (3 * width) // 4
    pw = width // n
    out = []
    for i in range(n):
        vw, vh = pw - 12, height - 9
        out.append(dict(view=(i * pw + 2, 5, vw, vh), bar=(i * pw + 4 + vw, 4), limits=(X0, X0 + M * vw, Y0, Y0 + M * vh)))
    return height, out


def arrows_of(vw, vh):
    """(n, 5): x, y, dx, dy, speed in the world of a view of vw x vh pixels"""
    cx, cy = X0 + M * vw / 2, Y0 + M * vh / 2
    a = []
    # eight octants and the four axis directions, 14 pixels long, round the centre
    for k, (dx, dy) in enumerate([(140, 0), (0, 140), (-140, 0), (0, -140), (130, 50), (50, 130), (-50, 130), (-130, 50), (-130, -50),
                                  (-50, -130), (50, -130), (130, -50)]):
        ang = 2 * np.pi * k / 12
        a.append((cx + 90 * np.cos(ang) + 0.37, cy + 90 * np.sin(ang) - 0.21, dx, dy, VMAX * k / 12))
    a.append((cx + 31.0, cy + 17.0, 2.0, 1.0, 0.3))                 # shorter than a pixel
    a.append((cx - 33.0, cy + 12.0, 0.0, 0.0, 0.2))                 # zero length
    a.append((X0 + 20.0, Y0 + 30.0, 600.0, 350.0, 0.45))            # long: the head's cap, and it leaves the view
    a.append((X0 - 40.0, cy, 300.0, 10.0, 0.1))                     # partly outside
    a.append((X0 + M * vw + 70.0, cy, -400.0, 30.0, 0.15))          # comes in from the right
    a.append((X0 - 500.0, Y0 - 500.0, 100.0, 100.0, 0.2))           # wholly outside
    a.append((np.nan, cy, 10.0, 10.0, 0.2))
    a.append((cx, np.inf, 10.0, 10.0, 0.2))
    a.append((cx, cy, -np.inf, 10.0, 0.2))
    a.append((X0 + M * 2.0 ** 20, cy, 30.0, 0.0, 0.2))              # exactly 2^20 pixels: left out
    a.append((X0 - M * (2.0 ** 20 - 1), cy, 300.0, 0.0, 0.2))       # just inside the limit: walked, nothing to see
    a.append((cx, cy, 1e300, 1e300, 0.2))                           # a tip beyond everything
    for speed in (0.05, 0.48, 0.25):                                # three arrows stacked on the same pixels
        a.append((cx - 60.0, cy - 80.0, 90.0, 40.0, speed))
    # speeds: 0, just below vmax, vmax, above, negative, NaN, infinite
    for k, speed in enumerate((0.0, np.nextafter(VMAX, 0), VMAX, 0.7, -0.1, np.nan, np.inf, 1e300)):
        a.append((X0 + 15.0 + 23.0 * k, Y0 + M * vh - 25.0, 14.0, -60.0, speed))
    return np.array(a, np.float64)


def panel_of(base, width, pivot, alpha):
    _, _, vw, vh = base["view"]
    cells = [(X0 + 50.0 + 100.0 * i, Y0 + M * vh - 30.0 - 100.0 * j, 100.0) for i in range(3) for j in range(2)]
    cells += [(X0 - 60.0, Y0 + 90.0, 100.0), (np.nan, Y0, 100.0), (X0 + 120.0, Y0 + 230.0, -40.0)]   # over the edge, left out, negative size
    measured = [1, 0, 0, 1, 0, 1, 0, 0, 0]
    outline = [(X0 - 80.0, Y0 + 40.0), (X0 + 60.0, Y0 + 55.0), (X0 + M * vw * 0.7, Y0 + M * vh + 90.0), (X0 + M * vw + 50.0, Y0 + 100.0),
               (np.nan, Y0), (X0 + 200.0, Y0 + 20.0), (X0 + 30.0, Y0 + 21.0)]
    cams = [(X0 + 100.0, Y0 + 100.0), (X0 + 5.0, Y0 + 5.0), (X0 - 25.0, Y0 + 200.0), (X0 + M * vw, Y0 + M * vh), (np.nan, 0.0),
            (X0 + 300.0, Y0 + 150.0), (X0 + 1e9, Y0), (X0 + 222.2, Y0 + 33.3)]
    return dict(base, cells=np.array(cells), measured=np.array(measured, np.uint8), outline=np.array(outline), arrows=arrows_of(vw, vh),
                pivot=pivot, width=width, alpha=alpha, vmax=VMAX, cameras=np.array(cams))


def texts_of(width, height):
    t = [(1, 1, "Date: 2019-07-24"), (2, 9, "Time: 10:00-10:30 UTC"), (width // 2, height // 2, "Cameras: UAS7, UAS8"),
         (3, height - 8, "Grid spacing: 250 m"), (width - 20, 3, "Speed (m/s)"), (-7, height // 3, "left edge"), (5, -3, "TOP EDGE"),
         (width - 4, height - 4, "corner"), (0, 0, ""), (10, 20, "0.0"), (10, 28, "0.5"), (width, 5, "outside"), (5, height, "below"),
         (12, 40, "abcdefghijklmnopqrstuvwxyz"), (1, 33, "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-:./ ,()ABCD"), (-400, -400, "far away")]
    assert len(t) == 16 and max(len(s) for _, _, s in t) == 48
    return t


def picture(width, views, variant, quality=90):
    height, base = views_of(width, views)
    panels = [panel_of(b, *v) for b, v in zip(base, VARIANTS[variant])]
    return dict(width=width, height=height, quality=quality, table=table(), texts=texts_of(width, height), panels=panels)


@functools.lru_cache(maxsize=None)
def _want(width, views, variant):
    rgb = R.render(picture(width, views, variant))
    rgb.setflags(write=False)
    return rgb


def case(width, views, variant):
    return picture(width, views, variant), _want(width, views, variant)


CASES = [(w, v, k) for w in WIDTHS for v in VIEWS for k in range(len(VARIANTS))]

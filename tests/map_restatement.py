"""The velocity map restated in numpy, independently of csrc/map_raster.h: plain loops over Python integers
and floats (one rounding per operation, as the rules say), no call into the library.  The letters are written out below as
rows of '#' and '.', so the library's table (icelk_map_glyph) is compared with something a person can read; the digits and
signs are plot_restatement's.

    render(picture, resident=None, group=None) -> (height, width, 3) uint8
    planes(picture, resident=None, group=None) -> base, top, count: int64 (height, width)
    arrow_hits(view, limits, width, pivot, arrow) -> [(p, q)] in view pixels, one entry per hit
"""
import math

import numpy as np

import plot_restatement as PR

GLYPHS = dict(PR.GLYPHS)
GLYPHS.update({
    "A": [".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"],
    "B": ["####.", "#...#", "#...#", "####.", "#...#", "#...#", "####."],
    "C": [".###.", "#...#", "#....", "#....", "#....", "#...#", ".###."],
    "D": ["####.", "#...#", "#...#", "#...#", "#...#", "#...#", "####."],
    "E": ["#####", "#....", "#....", "####.", "#....", "#....", "#####"],
    "F": ["#####", "#....", "#....", "####.", "#....", "#....", "#...."],
    "G": [".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".####"],
    "H": ["#...#", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"],
    "I": [".###.", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."],
    "J": ["..###", "...#.", "...#.", "...#.", "...#.", "#..#.", ".##.."],
    "K": ["#...#", "#..#.", "#.#..", "##...", "#.#..", "#..#.", "#...#"],
    "L": ["#....", "#....", "#....", "#....", "#....", "#....", "#####"],
    "M": ["#...#", "##.##", "#.#.#", "#.#.#", "#...#", "#...#", "#...#"],
    "N": ["#...#", "#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#"],
    "O": [".###.", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."],
    "P": ["####.", "#...#", "#...#", "####.", "#....", "#....", "#...."],
    "Q": [".###.", "#...#", "#...#", "#...#", "#.#.#", "#..#.", ".##.#"],
    "R": ["####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#"],
    "S": [".####", "#....", "#....", ".###.", "....#", "....#", "####."],
    "T": ["#####", "..#..", "..#..", "..#..", "..#..", "..#..", "..#.."],
    "U": ["#...#", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."],
    "V": ["#...#", "#...#", "#...#", "#...#", "#...#", ".#.#.", "..#.."],
    "W": ["#...#", "#...#", "#...#", "#.#.#", "#.#.#", "#.#.#", ".#.#."],
    "X": ["#...#", "#...#", ".#.#.", "..#..", ".#.#.", "#...#", "#...#"],
    "Y": ["#...#", "#...#", "#...#", ".#.#.", "..#..", "..#..", "..#.."],
    "Z": ["#####", "....#", "...#.", "..#..", ".#...", "#....", "#####"],
    ",": [".....", ".....", ".....", ".....", ".##..", "..#..", ".#..."],
    "(": ["...#.", "..#..", ".#...", ".#...", ".#...", "..#..", "...#."],
    ")": [".#...", "..#..", "...#.", "...#.", "...#.", "..#..", ".#..."],
})
BASE_COLOUR = {0: 255, 1: 211, 2: 169, 3: 0}      # white, lightgray, darkgray, black
LIMIT = 2.0 ** 20


def fixed(view, limits, x, y):
    """(X, Y) in 1/256 pixel relative to the view's corner, or None: the coordinate rule"""
    _, _, w, h = view
    xmin, xmax, ymin, ymax = (float(v) for v in limits)
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    try:
        cx = ((x - xmin) * float(w)) / (xmax - xmin)
        cy = ((ymax - y) * float(h)) / (ymax - ymin)
    except OverflowError:
        return None
    if not (abs(cx) < LIMIT and abs(cy) < LIMIT):     # false for inf and NaN
        return None
    return math.floor(cx * 256.0), math.floor(cy * 256.0)


def line(a, b, w, h, shift=0, thick=1):
    """[(p, q)] of a line between two fixed points inside a w x h view: the major-axis rule of DESIGN.md 7.6, the minor
    coordinate moved by -shift, every step marking its pixel and the thick - 1 after it along the minor axis"""
    (x0, y0), (x1, y1) = a, b
    xmajor = abs(x1 - x0) >= abs(y1 - y0)
    (ma, na), (mb, nb) = sorted([(x0, y0), (x1, y1)] if xmajor else [(y0, x0), (y1, x1)])
    n_major, n_minor = (w, h) if xmajor else (h, w)
    out = []
    if ma == mb:
        return out
    lo, hi = -((128 - ma) // 256), -((128 - mb) // 256)     # ceil((m - 128) / 256)
    for c in range(max(lo, 0), min(hi, n_major)):
        r = (na - shift + ((nb - na) * (256 * c + 128 - ma)) // (mb - ma)) >> 8
        for k in range(thick):
            if 0 <= r + k < n_minor:
                out.append((c, r + k) if xmajor else (r + k, c))
    return out


def arrow_width(view, limits, width):
    return max(256, math.floor(((float(width) * float(view[2])) / (float(limits[1]) - float(limits[0]))) * 256.0))


def arrow_hits(view, limits, width, pivot, arrow):
    x, y, dx, dy, speed = (float(v) for v in arrow)
    _, _, vw, vh = view
    if not (speed >= 0.0 and speed < math.inf):
        return []
    tx, ty = (x - dx * 0.5, y - dy * 0.5) if pivot in ("mid", 1) else (x, y)
    pos, tail, tip = fixed(view, limits, x, y), fixed(view, limits, tx, ty), fixed(view, limits, tx + dx, ty + dy)
    if pos is None or tail is None or tip is None:
        return []
    fx, fy = float(tip[0] - tail[0]), float(tip[1] - tail[1])
    length = math.sqrt(fx * fx + fy * fy)
    if length < 256.0:
        p, q = pos[0] >> 8, pos[1] >> 8
        return [(p, q)] if 0 <= p < vw and 0 <= q < vh else []
    w = arrow_width(view, limits, width)
    hl = min(5.0 * float(w), length, 48.0 * 256.0)
    ux, uy = fx / length, fy / length
    bx, by = float(tip[0]) - hl * ux, float(tip[1]) - hl * uy
    hb = (3.0 * hl) / 10.0
    thick = min(7, max(1, (w + 128) >> 8))
    out = line(tail, (math.floor(bx), math.floor(by)), vw, vh, shift=(thick - 1) * 128, thick=thick)
    tri = [tip, (math.floor(bx - hb * uy), math.floor(by + hb * ux)), (math.floor(bx + hb * uy), math.floor(by - hb * ux))]

    def cross(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    area = cross(*tri)
    if area == 0:
        return out
    if area < 0:
        tri = [tri[0], tri[2], tri[1]]
    p0, p1 = max(0, min(v[0] for v in tri) >> 8), min(vw - 1, max(v[0] for v in tri) >> 8)
    q0, q1 = max(0, min(v[1] for v in tri) >> 8), min(vh - 1, max(v[1] for v in tri) >> 8)
    for q in range(q0, q1 + 1):
        for p in range(p0, p1 + 1):
            c = (256 * p + 128, 256 * q + 128)
            if cross(tri[0], tri[1], c) >= 0 and cross(tri[1], tri[2], c) >= 0 and cross(tri[2], tri[0], c) >= 0:
                out.append((p, q))
    return out


def _cell(base, view, limits, left, top, size, measured):
    x0, y0, vw, vh = view
    a, b = fixed(view, limits, left, top), fixed(view, limits, float(left) + float(size), float(top) - float(size))
    if a is None or b is None:
        return
    sub = base[y0:y0 + vh, x0:x0 + vw]
    if not measured:
        p0, p1 = max(0, -((128 - a[0]) // 256)), min(vw, -((128 - b[0]) // 256))
        q0, q1 = max(0, -((128 - a[1]) // 256)), min(vh, -((128 - b[1]) // 256))
        if p1 > p0 and q1 > q0:
            sub[q0:q1, p0:p1] = np.maximum(sub[q0:q1, p0:p1], 1)
    for s, e in (((a[0], a[1]), (b[0], a[1])), ((a[0], b[1]), (b[0], b[1])), ((a[0], a[1]), (a[0], b[1])), ((b[0], a[1]), (b[0], b[1]))):
        for p, q in line(s, e, vw, vh):
            sub[q, p] = max(sub[q, p], 2)


def _panel_arrows(panel, resident, group):
    """[(index, arrow)] a panel draws"""
    if panel.get("resident"):
        a = np.asarray(resident, np.float64).reshape(-1, 5)
        want = int(panel.get("group", -1))
        keep = np.ones(len(a), bool) if want < 0 else np.asarray(group) == want
        return [(int(k), a[k]) for k in np.nonzero(keep)[0]]
    return list(enumerate(np.asarray(panel.get("arrows", np.zeros((0, 5))), np.float64).reshape(-1, 5)))


def planes(picture, resident=None, group=None):
    W, H = picture["width"], picture["height"]
    base, top, count = (np.zeros((H, W), np.int64) for _ in range(3))
    for panel in picture["panels"]:
        view, limits = tuple(panel["view"]), panel["limits"]
        x0, y0, vw, vh = view
        cells = np.asarray(panel.get("cells", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        for (left, t, size), m in zip(cells, np.asarray(panel.get("measured", ())).ravel()):
            _cell(base, view, limits, left, t, size, bool(m))
        xy = np.asarray(panel.get("outline", np.zeros((0, 2))), np.float64).reshape(-1, 2)
        for k in range(len(xy) - 1):
            a, b = fixed(view, limits, *xy[k]), fixed(view, limits, *xy[k + 1])
            if a is not None and b is not None:
                for p, q in line(a, b, vw, vh):
                    base[y0 + q, x0 + p] = 3
        ys, xs, ids = [], [], []
        for index, arrow in _panel_arrows(panel, resident, group):
            hits = arrow_hits(view, limits, panel.get("width", 4.0), panel.get("pivot", "tail"), arrow)
            xs += [x0 + p for p, _ in hits]
            ys += [y0 + q for _, q in hits]
            ids += [index + 1] * len(hits)
        at = (np.array(ys, np.int64), np.array(xs, np.int64))
        np.maximum.at(top, at, np.array(ids, np.int64))
        np.add.at(count, at, 1)
    return base, top, count


def text_mask(texts, W, H):
    m = np.zeros((H, W), bool)
    k = max(1, W // 400)
    for px, py, s in texts:
        for n, ch in enumerate(s):
            for r, row in enumerate(GLYPHS[ch.upper()]):
                for col, bit in enumerate(row):
                    if bit == "#":
                        ys, xs = py + r * k, px + (6 * n + col) * k
                        m[max(ys, 0):max(ys + k, 0), max(xs, 0):max(xs + k, 0)] = True      # slices drop what falls outside
    return m


def colour_index(speed, vmax):
    return int(min(255.0, math.floor((float(speed) / float(vmax)) * 256.0)))


def render(picture, resident=None, group=None):
    W, H = picture["width"], picture["height"]
    table = np.asarray(picture["table"], np.uint8).reshape(256, 3).astype(np.int64)
    base, top, count = planes(picture, resident, group)
    gray = np.vectorize(BASE_COLOUR.get)(base).astype(np.int64)
    out = np.repeat(gray[..., None], 3, axis=2)
    r = max(2, (3 * W) // 1000)
    for panel in picture["panels"]:
        x0, y0, vw, vh = view = tuple(panel["view"])
        arrows = dict(_panel_arrows(panel, resident, group))
        alpha = float(panel.get("alpha", 1.0))
        T = [int(math.floor((1.0 - alpha) ** k * 65536 + 0.5)) for k in range(32)]
        for q in range(vh):
            for p in range(vw):
                t = top[y0 + q, x0 + p]
                if t:
                    over = table[colour_index(arrows[t - 1][4], panel.get("vmax", 0.5))]
                    tt = T[min(int(count[y0 + q, x0 + p]), 31)]
                    out[y0 + q, x0 + p] = (gray[y0 + q, x0 + p] * tt + over * (65536 - tt) + 32768) >> 16
        qq, pp = np.mgrid[0:vh, 0:vw]
        for cam in np.asarray(panel.get("cameras", np.zeros((0, 2))), np.float64).reshape(-1, 2):
            c = fixed(view, panel["limits"], *cam)
            if c is not None:
                disc = (256 * pp + 128 - c[0]) ** 2 + (256 * qq + 128 - c[1]) ** 2 <= (256 * r) ** 2
                out[y0:y0 + vh, x0:x0 + vw][disc] = (255, 0, 0)
    for panel in picture["panels"]:
        x0, y0, vw, vh = panel["view"]
        bx, bw = panel.get("bar", (0, 0))
        if bw > 0:
            for row in range(vh):
                idx = 255 - (255 * row) // (vh - 1) if vh > 1 else 255
                out[y0 + row, bx:bx + bw] = table[idx]
            out[y0, bx:bx + bw] = 0
            out[y0 + vh - 1, bx:bx + bw] = 0
            out[y0:y0 + vh, bx] = 0
            out[y0:y0 + vh, bx + bw - 1] = 0
    out[text_mask(picture.get("texts", ()), W, H)] = 0
    return out.astype(np.uint8)

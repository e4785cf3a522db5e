"""Frames on which double addition of the detector's box sums ROUNDS, with references to tell orders apart -- TEST HARNESS.

cornerMinEigenVal box-filters three planes of float32 products (dx*dx, dx*dy, dy*dy) into double sums.
tests/test_oracle_kat.py proves such sums exact for derivatives of the form integer * scale.  Real planes are not that:
dy = rdy[down] - rdy[up] is the difference of two row smooths that were each rounded three times, so where two pixel
rows nearly cancel dy is a rounding residue (|dy| down to 2^-28 against k1 ~ 1e-4).  A product with such a dy has
its low bit near 2^-63; beside ordinary products (up to ~2^-3) in one window the sum needs more than 53 bits, and the ORDER
of the additions shows in the result.  The oracle, np_restatement and the generic kernel add term by term (each window row
left to right, then the row sums top to bottom); the strip kernel keeps a running column sum down the strip and slides a
window along the row (k_corners.hip).  The running sum keeps the rounding error of a tiny term that entered while the sum
was large and left when it was small: texture -> near-flat within blockSize rows.  These frames have that transition.

Numpy and the standard library only; nothing compiled, not the oracle, not the package.

  frame(seed, kind, ...)    the generator
  products(img, bs)         the three float32 product planes, as np_restatement.min_eig_map forms them
  exact_sums(img, bs)       the box sums with no rounding at all (Python integers), each rounded ONCE to double
  exact_map(img, bs)        the restatement's float32 eigenvalue formula on those -- the high-precision reference
  sequential_sums(img, bs)  the term-by-term double sums (window row-major)
  running_map(img, bs)      a column running sum down the frame, then a sliding row sum: another legal double summation
                            (NOT the kernel instruction for instruction: no strips, no batches of four outputs)
  chain_length(bs), bound(img, bs)   the derived bound of DESIGN.md section 4.2
  FRAMES, RESIDUE_FRAMES    the chosen frames
  references(entry)         image, exact map, bound and the two CPU maps of one of them, computed once per session
"""
import numpy as np

import np_restatement as R

F = np.float32
KINDS = ("const", "pm1", "pm3", "stripes", "flecks")
FUSED = (3, 5, 7, 10)


# ---------------------------------------------------------------------------------------------- frames
def band(rng, kind, rows, w):
    """A near-flat band: the residues of dy live where two pixel rows (nearly) cancel."""
    if kind == "const":
        return np.full((rows, w), rng.randint(0, 256), np.int64)
    if kind == "pm1":
        return np.clip(rng.randint(1, 255) + rng.randint(-1, 2, (rows, w)), 0, 255)
    if kind == "pm3":
        return np.clip(128 + rng.randint(-3, 4, (rows, w)), 0, 255)
    if kind == "stripes":
        return np.repeat(rng.randint(0, 256, (1, w)), rows, axis=0)
    if kind == "flecks":
        b = np.repeat(rng.randint(0, 256, (1, w)), rows, axis=0)
        return np.clip(b + (rng.rand(rows, w) < 0.05) * rng.choice([-1, 1], (rows, w)), 0, 255)
    raise ValueError(kind)


def frame(seed, kind, w=48, above=False, lead=0):
    """Random 8-bit texture (8-29 rows) over a near-flat band (12-29 rows) of `kind`.

    above   a second band of the same kind above the texture (flat -> texture -> flat)
    lead    rows of one more band put on top of everything: moves the transitions down the frame, e.g. to just above the
            seam between two strips of the kernel
    The draws of the basic frame come first, so (seed, kind) means the same texture and band whatever the options."""
    rng = np.random.RandomState(seed)
    h1, h2 = rng.randint(8, 30), rng.randint(12, 30)
    parts = [rng.randint(0, 256, (h1, w)), band(rng, kind, h2, w)]
    if above:
        parts.insert(0, band(rng, kind, rng.randint(12, 30), w))
    if lead:
        parts.insert(0, band(rng, kind, lead, w))
    return np.concatenate(parts).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- planes and windows
def products(img, bs):
    """(dx*dx, dx*dy, dy*dy) in float32: the operation order of np_restatement.min_eig_map (A.7), restated so that the planes
    can be had; tests/test_box_sums_host.py holds the term-by-term sums of these against R.min_eig_map."""
    s = np.asarray(img).astype(np.float32)
    h, w = s.shape
    scale = 1.0 / (4.0 * int(bs) * 255.0)
    k1, k0 = F(scale), F(2.0 * scale)
    lf, rt = R._ridx(-1, w, w), R._ridx(1, w, w)
    up, dn = R._ridx(-1, h, h), R._ridx(1, h, h)
    rdx = s[:, rt] - s[:, lf]
    dx = (rdx[up] + rdx[dn]) * k1 + rdx * k0
    rdy = k1 * s[:, lf]
    rdy = rdy + k0 * s
    rdy = rdy + k1 * s[:, rt]
    dy = rdy[dn] - rdy[up]
    out = (dx * dx, dx * dy, dy * dy)
    assert all(p.dtype == np.float32 for p in out)
    return out


def window_index(n, bs):
    """Row (or column) indices of the window's k-th line for every output position: anchor bs // 2, reflect-101."""
    an = int(bs) // 2
    return [R._ridx(k - an, n, n) for k in range(int(bs))]


SHIFT = 149   # every finite float32 is an integer multiple of 2^-149


def _as_integers(plane):
    """float32 -> Python integers, value * 2^149, exactly (a float32 times a power of two is exact in double)."""
    scaled = plane.astype(np.float64) * 2.0 ** SHIFT
    return np.array([int(v) for v in scaled.ravel()], dtype=object).reshape(plane.shape)


def exact_sums(img, bs, drop=None, shift_rows=0):
    """The three box sums per pixel, formed in integers (no rounding, so no order) and rounded once to double.

    The two planted errors of the bound's own test:
      drop = (y, x, k)   leaves the k-th term (row-major) out of the window of pixel (y, x)
      shift_rows = d     takes every window d rows lower"""
    h, w = np.asarray(img).shape
    by, bx = window_index(h, bs), window_index(w, bs)
    if shift_rows:
        by = [np.array([R.reflect101(i + shift_rows, h) for i in c], np.intp) for c in by]
    out = []
    for p in products(img, bs):
        z = _as_integers(p)
        rows = sum(z[:, c] for c in bx)
        s = sum(rows[c] for c in by)
        if drop is not None:
            y, x, k = drop
            s[y, x] -= z[by[k // int(bs)][y], bx[k % int(bs)][x]]
        # int / int is correctly rounded in Python: one rounding, to double
        out.append(np.array([v / (1 << SHIFT) for v in s.ravel()], np.float64).reshape(h, w))
    return out


def eig_of_sums(s0, s1, s2):
    """The float32 formula of np_restatement.min_eig_map (calcMinEigenVal) on double sums; also returns a, c."""
    a, b, c = s0.astype(np.float32) * F(0.5), s1.astype(np.float32), s2.astype(np.float32) * F(0.5)
    t = a - c
    eig = (a + c) - np.sqrt(t * t + b * b)
    assert eig.dtype == np.float32
    return eig, a, c


def exact_map(img, bs, **planted):
    return eig_of_sums(*exact_sums(img, bs, **planted))[0]


def sequential_sums(img, bs):
    """One double accumulator per window, the bs*bs terms added row-major."""
    h, w = np.asarray(img).shape
    by, bx = window_index(h, bs), window_index(w, bs)
    out = []
    for p in products(img, bs):
        d = p.astype(np.float64)
        acc = np.zeros((h, w))
        for ry in by:
            for cx in bx:
                acc = acc + d[np.ix_(ry, cx)]
        out.append(acc)
    return out


def rows_first_sums(img, bs):
    """The oracle's and the restatement's order: each window row left to right, then the row sums top to bottom."""
    h, w = np.asarray(img).shape
    by, bx = window_index(h, bs), window_index(w, bs)
    out = []
    for p in products(img, bs):
        d = p.astype(np.float64)
        r = sum(d[:, c] for c in bx)
        out.append(sum(r[c] for c in by))
    return out


def running_sums(img, bs):
    """Column sums first, as ONE running double sum per column carried down the whole frame, V = (V + new) - oldest; then a
    window slid along each row, s = (s - oldest) + next, carried across the whole row."""
    bs = int(bs)
    h, w = np.asarray(img).shape
    an = bs // 2
    ry = R._ridx(-an, h + bs - 1, h)          # covariance rows the columns walk through, reflected
    rx = R._ridx(-an, w + bs - 1, w)
    out = []
    for p in products(img, bs):
        d = p.astype(np.float64)[np.ix_(ry, rx)]            # (h + bs - 1, w + bs - 1)
        V = np.zeros(w + bs - 1)
        for r in range(bs - 1):
            V = V + d[r]
        col = np.empty((h, w + bs - 1))
        for y in range(h):
            V = V + d[y + bs - 1]
            if y:
                V = V - d[y - 1]
            col[y] = V
        s = col[:, 0].copy()
        for k in range(1, bs):
            s = s + col[:, k]
        res = np.empty((h, w))
        res[:, 0] = s
        for x in range(1, w):
            s = (s - col[:, x - 1]) + col[:, x + bs - 1]
            res[:, x] = s
        out.append(res)
    return out


def running_map(img, bs):
    return eig_of_sums(*running_sums(img, bs))[0]


# ---------------------------------------------------------------------------------------------- the bound
def strip_cfg(bs):
    """StripCfg<BS> of k_corners.hip, restated; tests/test_box_sums_host.py reads the constants back out of the source."""
    from math import gcd
    nt, r, rx = 256, 4, 4
    unroll = bs * r // gcd(bs, r)
    eh = (64 // unroll) * unroll
    return dict(NT=nt, R=r, RX=rx, UNROLL=unroll, EH=eh, SH=eh - 2, NROWS=eh + bs - 1, TW=nt - (bs - 1) - 2)


def chain_length(bs):
    """N: the double additions on the strip kernel's longest chain into one box sum.

    column running sum   bs - 1 additions fill the window, then 2 (one +, one -) for each of the EH eigenvalue rows of a strip
    row window           bs - 1 additions form the first of a task's RX outputs, 2 for each of the RX - 1 slides
    blockSize 3 adds its three terms afresh per output (2 additions): counted as the longer sliding form."""
    c = strip_cfg(int(bs))
    return (int(bs) - 1) + 2 * c["EH"] + (int(bs) - 1) + 2 * (c["RX"] - 1)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


def bound(img, bs, n=None):
    """Per pixel: 4 * ulp32(a + c) + 4 * N * 2^-53 * Smax, a and c from the exact reference, Smax = bs^2 * the largest
    product magnitude of the frame.  No margin."""
    n = chain_length(bs) if n is None else n
    _, a, c = eig_of_sums(*exact_sums(img, bs))
    smax = float(int(bs) ** 2) * max(float(np.abs(p).max()) for p in products(img, bs))
    return 4.0 * ulp32(a + c).astype(np.float64) + 4.0 * n * 2.0 ** -53 * smax


def within_bound(got, img, bs, ref=None, bnd=None):
    ref = exact_map(img, bs) if ref is None else ref
    bnd = bound(img, bs) if bnd is None else bnd
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bnd


# ---------------------------------------------------------------------------------------------- the chosen frames
# (seed, kind, blockSize, options of frame(), map_differs); map_differs: running_map != R.min_eig_map in some pixel.
#
# How they were found: seeds 0 .. 1999 x the five kinds x blockSize 3 / 5 / 7 / 10, running_map against R.min_eig_map.  856
# of the 40 000 differ: 130 / 547 / 53 / 126 at blockSize 3 / 5 / 7 / 10, so every fused blockSize has frames of its own;
# 790 are "pm1", 57 "pm3", 9 "const" (RESIDUE_FRAMES below), none "stripes" or "flecks" (rows of a striped band are equal, so
# dy is exactly 0 there, not a residue; the two such frames kept here have their one inexact window in the texture).
# Each differs in 1 - 6 pixels by 2e-13 .. 4e-12.  Kept: those that ALSO have a window whose sequential double sum is
# not the exact sum (a running sum can round where no single window's own sum does: (26, "pm1", 3) is such a frame).
#   w = 300         crosses the strip seam in x (a strip is 252 / 250 / 248 / 245 outputs wide); the chosen ones differ at
#                   x = 240 .. 281, at or just past the seam
#   lead            puts the texture -> band transition 3 rows above the strip seam in y (output row 58; 54 at blockSize 7);
#                   the frame is then taller than one strip
#   above           flat -> texture -> flat
FRAMES = [
    (50, "pm1", 3, {}, True), (51, "pm1", 3, {}, True), (54, "pm1", 3, {}, True),
    (13, "pm1", 5, {}, True), (31, "pm1", 5, {}, True), (166, "pm3", 5, {}, True), (399, "pm3", 5, {}, True),
    (121, "pm1", 7, {}, True), (124, "pm1", 7, {}, True), (238, "pm1", 7, {}, True),
    (18, "pm1", 10, {}, True), (48, "pm1", 10, {}, True), (180, "pm3", 10, {}, True), (900, "pm3", 10, {}, True),
    (5, "stripes", 10, {}, False), (5, "flecks", 10, {}, False),
    (50, "pm1", 3, {"above": True}, True), (51, "pm3", 5, {"above": True}, True), (124, "pm1", 7, {"above": True}, True),
    (141, "pm1", 7, {"above": True}, True), (18, "pm1", 10, {"above": True}, True), (48, "pm1", 10, {"above": True}, True),
    (149, "pm1", 3, {"w": 300}, True), (21, "pm1", 5, {"w": 300}, True), (55, "pm3", 5, {"w": 300}, True),
    (10, "pm1", 7, {"w": 300}, True), (10, "pm3", 7, {"w": 300}, True), (121, "pm1", 10, {"w": 300}, True),
    (19, "pm1", 10, {"w": 300}, True),
    (50, "pm1", 3, {"lead": 31}, True), (56, "pm1", 5, {"lead": 26}, True), (161, "pm3", 5, {"lead": 33}, True),
    (124, "pm1", 7, {"lead": 29}, True), (121, "pm1", 7, {"lead": 41}, True), (18, "pm1", 10, {"lead": 37}, True),
    (48, "pm1", 10, {"lead": 47}, True), (180, "pm3", 10, {"lead": 30}, True),
]

# A band that is exactly constant below the texture: every product of the band is 0, so each exact box sum there is 0 and
# the map exactly 0 -- and a running column sum that took a rounding error in the texture keeps it for as long as it runs,
# blockSize columns wide: 39 - 200 pixels of a frame read 2e-19 .. 3e-18 where the term-by-term sum reads 0.  Far inside the
# bound, but many pixels: these frames are held to the bound, NOT to the 1 % share (the share is a property of bands that keep
# feeding terms which bury the residue below a float32 ulp).  Same layout as FRAMES; map_differs is True for all.
RESIDUE_FRAMES = [
    (1740, "const", 3, {}, True), (642, "const", 7, {}, True), (642, "const", 10, {}, True),
    (147, "const", 10, {"w": 300}, True),
]


def build(entry):
    seed, kind, bs, opts, _ = entry
    return frame(seed, kind, **opts)


def tag(entry):
    seed, kind, bs, opts, _ = entry
    return "%s%d-bs%d%s" % (kind, seed, bs, "".join("-%s%s" % (k, "" if v is True else v) for k, v in sorted(opts.items())))


_references = {}


def references(entry):
    """Per chosen frame, once per session and read-only: img, bs, exact (exact_map), bound, term (R.min_eig_map), running."""
    key = tag(entry)
    if key not in _references:
        img, bs = build(entry), entry[2]
        r = dict(img=img, bs=bs, exact=exact_map(img, bs), bound=bound(img, bs), term=R.min_eig_map(img, bs),
                 running=running_map(img, bs))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _references[key] = r
    return _references[key]

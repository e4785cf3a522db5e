"""The Harris response and the corner selection on it, in numpy alone -- TEST HARNESS.

The C oracle does not know the Harris detector; this module pins it, the way tests/np_restatement.py pins the default
path.  `harris_map` is written as np_restatement.min_eig_map is -- the same Sobel pair in OpenCV's operation order, the
same term-by-term box sums in double -- and ends in one of the two forms of DESIGN.md 4.2 on a = (float)S dx^2,
b = (float)S dx dy, c = (float)S dy^2, which are NOT halved as calcMinEigenVal halves them:

    tail = 0   calcHarris' float lanes: every operation rounded to float32, nothing fused
               t = a + c;  R = (a c - b b) - (kf t) t;   kf = (float)k
    tail = 1   its scalar tail, where k stays a double
               R = (float)((double)(fl(a c) - fl(b b)) - (k (double)fl(a + c)) (double)fl(a + c))

Both forms are written from knowledge of upstream OpenCV; this is still not OpenCV ("parity unpinned").
`good_features` is the selection of np_restatement.good_features, restated on a map that is handed in: a map whose
masked maximum is <= 0 yields None (THRESH_TOZERO at max * qualityLevel leaves no masked pixel above zero).

It imports numpy, the standard library and np_restatement's index helpers: not the oracle, not the package.
"""
import numpy as np

from np_restatement import F, _ridx, _u8image


def cov_sums(img, blockSize=3):
    """(a, b, c): the un-normalised blockSize x blockSize box sums of dx^2, dx dy, dy^2 as float32 planes (anchor
    blockSize / 2, BORDER_REFLECT_101), summed term by term in double."""
    s = _u8image(img).astype(np.float32)
    h, w = s.shape
    bs = int(blockSize)
    scale = 1.0 / (4.0 * bs * 255.0)
    k1, k0 = F(scale), F(2.0 * scale)
    lf, rt = _ridx(-1, w, w), _ridx(1, w, w)
    up, dn = _ridx(-1, h, h), _ridx(1, h, h)
    # Dx: row pass [-1 0 1] (exact), scaled symmetric column pass (r0 + r2)*k1 + r1*k0
    rdx = s[:, rt] - s[:, lf]
    dx = (rdx[up] + rdx[dn]) * k1 + rdx * k0
    # Dy: scaled row pass k1*l + k0*c + k1*r left to right, column pass [-1 0 1]
    rdy = k1 * s[:, lf]
    rdy = rdy + k0 * s
    rdy = rdy + k1 * s[:, rt]
    dy = rdy[dn] - rdy[up]
    assert dx.dtype == np.float32 and dy.dtype == np.float32
    an = bs // 2
    bx = [_ridx(k - an, w, w) for k in range(bs)]
    by = [_ridx(k - an, h, h) for k in range(bs)]

    def box(plane):
        p = plane.astype(np.float64)
        r = sum(p[:, c] for c in bx)
        return sum(r[c] for c in by).astype(np.float32)

    return box(dx * dx), box(dx * dy), box(dy * dy)


def harris_map(img, blockSize=3, k=0.04, tail=0):
    a, b, c = cov_sums(img, blockSize)
    t = a + c
    det = a * c - b * b
    assert t.dtype == np.float32 and det.dtype == np.float32
    if tail:
        t64 = t.astype(np.float64)
        r = (det.astype(np.float64) - (float(k) * t64) * t64).astype(np.float32)
    else:
        r = det - (F(k) * t) * t
    assert r.dtype == np.float32
    return r


def select(resp, maxCorners, qualityLevel, minDistance, mask=None):
    """goodFeaturesToTrack behind its response map: (M,1,2) float32 in response order, or None."""
    h, w = resp.shape
    ok = np.ones((h, w), bool) if mask is None else (_u8image(mask) != 0)
    max_val = float(resp[ok].max()) if ok.any() else 0.0
    thresh = F(max_val * float(qualityLevel))
    t = np.where(resp > thresh, resp, F(0))                   # THRESH_TOZERO keeps strictly greater
    big = np.full((h + 2, w + 2), -np.inf, np.float32)
    big[1:-1, 1:-1] = t
    dil = np.max([big[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    keep = (t != 0) & (t == dil) & ok
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    idx = np.nonzero(keep.ravel())[0]
    vals = t.ravel()[idx]
    order = sorted(range(len(idx)), key=lambda j: (-float(vals[j]), -int(idx[j])))   # higher address first among equals
    out = []
    cell = int(np.rint(float(minDistance))) if minDistance >= 1 else 0   # cvRound
    grid = {}
    md2 = float(minDistance) * float(minDistance)
    for j in order:
        y, x = divmod(int(idx[j]), w)
        if cell:
            xc, yc = x // cell, y // cell
            near = (q for yy in range(yc - 1, yc + 2) for xx in range(xc - 1, xc + 2) for q in grid.get((xx, yy), ()))
            if any((x - qx) * (x - qx) + (y - qy) * (y - qy) < md2 for qx, qy in near):
                continue
            grid.setdefault((xc, yc), []).append((x, y))
        out.append((x, y))
        if maxCorners > 0 and len(out) == maxCorners:
            break
    if not out:
        return None
    return np.array(out, np.float32).reshape(-1, 1, 2)


def ties(resp, qualityLevel, mask=None):
    """how many pairs of candidates of `select` have the same response (their order is then by address)"""
    p = select(resp, 0, qualityLevel, 0, mask)
    if p is None:
        return 0
    v = np.sort(np.array([resp[int(y), int(x)] for x, y in p.reshape(-1, 2)]))
    return int((v[1:] == v[:-1]).sum())


def good_features(img, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3, useHarrisDetector=False, k=0.04,
                  tail=0):
    """cv2.goodFeaturesToTrack-shaped.  useHarrisDetector=False: np_restatement's own statement of the default path."""
    if not useHarrisDetector:
        import np_restatement
        return np_restatement.good_features(img, maxCorners, qualityLevel, minDistance, mask, blockSize)
    return select(harris_map(_u8image(img), blockSize, k, tail), maxCorners, qualityLevel, minDistance, mask)


class HarrisRestatementCv:
    """cv2-shaped facade for tests/reference_loops.run_reference_loop: np_restatement's tracker, this module's detector."""

    @staticmethod
    def calcOpticalFlowPyrLK(a, b, p0, p1, **kw):
        import np_restatement
        return np_restatement.pyrlk(a, b, p0, p1, **kw)

    @staticmethod
    def goodFeaturesToTrack(img, mask=None, **kw):
        return good_features(img, kw["maxCorners"], kw["qualityLevel"], kw["minDistance"], mask, kw.get("blockSize", 3),
                             kw.get("useHarrisDetector", False), kw.get("k", 0.04))


# ---------------------------------------------------------------------------------------------- frames
def blob_frame(w, h, seed, shift=(0.0, 0.0)):
    """Seeded Gaussian blobs, about one per 250 px^2: centres anywhere (the frame's edges included), sigma 1.2 .. 3.5 px,
    amplitudes 40 .. 215, on a dark ground of fine noise (17 .. 26).  `shift` moves every blob and leaves the ground (a
    sequence for the frame loop).  The ground is not flat on purpose: where a dy is a rounding residue the strip kernel's
    running sums differ from term-by-term sums by ~2^-53 of the sum (k_corners.hip, window_sums' note), which a float32 map
    shows only where everything else in the window is exactly zero -- over flat ground."""
    rng = np.random.RandomState(seed)
    n = max(4, w * h // 250)
    cx, cy = rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)
    sg, am = rng.uniform(1.2, 3.5, n), rng.uniform(40, 215, n)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 17.0 + rng.randint(0, 10, (h, w))
    for x0, y0, s, a in zip(cx, cy, sg, am):
        r = int(4 * s) + 2
        ya, yb = max(0, int(y0 + shift[1]) - r), min(h, int(y0 + shift[1]) + r + 1)
        xa, xb = max(0, int(x0 + shift[0]) - r), min(w, int(x0 + shift[0]) + r + 1)
        if ya >= yb or xa >= xb:
            continue
        d2 = (xx[ya:yb, xa:xb] - x0 - shift[0]) ** 2 + (yy[ya:yb, xa:xb] - y0 - shift[1]) ** 2
        img[ya:yb, xa:xb] += a * np.exp(-d2 / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def lattice_frame(w=120, h=90, pitch=20, sigma=2.0, amp=180.0):
    """isolated blobs at the integer lattice positions (pitch/2 + i pitch, pitch/2 + j pitch); -> (frame, positions)"""
    pos = [(x, y) for y in range(pitch // 2, h - pitch // 4, pitch) for x in range(pitch // 2, w - pitch // 4, pitch)]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 20.0)
    for k, (x0, y0) in enumerate(pos):
        img += (amp - 3 * k) * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * sigma * sigma))   # no two alike: no ties
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), pos


def ramp_frame():
    return np.tile((np.arange(60, dtype=np.uint8) * 4), (40, 1))

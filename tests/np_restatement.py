"""A third statement of the tracking path, in numpy alone -- TEST HARNESS.

Gray, pyrDown, the pyramid stop rule, Scharr, pyramidal Lucas-Kanade with the forward-backward filter, the
Shi-Tomasi eigenvalue map and corner selection, written from SURVEY.md Appendix A (A.1 - A.7, with A.9 for what those leave open) and the bullets of
DESIGN.md section 2 (np.hypot on float32, Sobel operation order, box sums exact in double).  It imports numpy and the
standard library only: not the oracle, not the package, nothing compiled.  The oracle (oracle/icelk_oracle.c) and
the HIP kernels were written by one hand from one reading of those texts; this module is held against both, bit for
bit (tests/test_restatement_oracle.py, tests/test_gpu_restatement.py), so that an error the two share has a third
witness.  It is still not OpenCV: "parity unpinned" keeps its meaning with respect to cv2.

Structure: vectorised over the window, a Python loop over points (point-major: all levels of one point, then the
next point -- the oracle is level-major), reflected borders by explicit index arrays.

The call shapes are those of oracle/cpu.py, so a test can swap one for the other.

Default variant only.  The named variants (`lk_sums` 1 / 2, `sobel_fma`, `eig_fma`) are out of scope: numpy has no
fused multiply-add, and emulating one through float64 rounds twice; the float-lane sums would need a Python loop per
pixel.  They stay pinned oracle-to-kernel (test_named_variants_equal_the_oracles).

What keeps it exact: every float constant and every intermediate is an np.float32 (never a bare Python float next
to one); window sums are exact Python / int64 integers converted once; cvRound is np.rint of the float32 product
evaluated left to right; the epsilon test is formed in double; box sums go through float64 and back.
"""
import numpy as np

F = np.float32
CRIT_COUNT = 1
CRIT_EPS = 2
FLAG_INITIAL_FLOW = 4
FLAG_MIN_EIGENVALS = 8
W_BITS = 14
FLT_EPSILON = F(2.0 ** -23)
FLT_SCALE = F(2.0 ** -20)


# ---------------------------------------------------------------------------------------------- borders
def reflect101(i, n):
    """BORDER_REFLECT_101 (A.3): ... 2 1 | 0 1 2 ... n-2 n-1 | n-2 n-3 ..., by iterated reflection; n == 1 -> 0."""
    i, n = int(i), int(n)
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def _ridx(start, count, n):
    return np.array([reflect101(i, n) for i in range(start, start + count)], np.intp)


def _u8image(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("expected HxW uint8 image")
    return a


# ---------------------------------------------------------------------------------------------- A.1
def bgr2gray(img, variant=3):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected HxWx3 uint8 image")
    k0, k1, k2, s = {3: (1868, 9617, 4899, 14), 4: (3735, 19235, 9798, 15)}[variant]
    c = a.astype(np.int64)
    return ((c[..., 0] * k0 + c[..., 1] * k1 + c[..., 2] * k2 + (1 << (s - 1))) >> s).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- A.3
def pyrdown(img):
    s = _u8image(img).astype(np.int64)
    h, w = s.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    cx = [np.array([reflect101(2 * x + k, w) for x in range(dw)], np.intp) for k in (-2, -1, 0, 1, 2)]
    r = s[:, cx[0]] + s[:, cx[4]] + 4 * (s[:, cx[1]] + s[:, cx[3]]) + 6 * s[:, cx[2]]
    cy = [np.array([reflect101(2 * y + k, h) for y in range(dh)], np.intp) for k in (-2, -1, 0, 1, 2)]
    d = r[cy[0]] + r[cy[4]] + 4 * (r[cy[1]] + r[cy[3]]) + 6 * r[cy[2]]
    return ((d + 128) >> 8).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- A.2
def pyramid_levels(w, h, win, max_level):
    """The effective maxLevel: after level l exists the NEXT size decides."""
    for level in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win[0] or h <= win[1]:
            return level
    return max_level


def build_pyramid(img, win=(21, 21), max_level=3):
    """The level images buildOpticalFlowPyramid holds, unpadded."""
    img = _u8image(img)
    levels = [img.copy()]
    for _ in range(pyramid_levels(img.shape[1], img.shape[0], win, max_level)):
        levels.append(pyrdown(levels[-1]))
    return levels


# ---------------------------------------------------------------------------------------------- A.4
def scharr(img):
    s = _u8image(img).astype(np.int64)
    h, w = s.shape
    up, dn = s[_ridx(-1, h, h)], s[_ridx(1, h, h)]
    t0 = (up + dn) * 3 + s * 10
    t1 = dn - up
    lf, rt = _ridx(-1, w, w), _ridx(1, w, w)
    ix = t0[:, rt] - t0[:, lf]
    iy = (t1[:, rt] + t1[:, lf]) * 3 + t1 * 10
    return np.stack([ix, iy], -1).astype(np.int16)


# ---------------------------------------------------------------------------------------------- A.5 / A.6
def _weights(a, b):
    """14-bit bilinear weights of the fractions (a, b); the last flag says whether a product was an exact half."""
    one, s = F(1), F(1 << W_BITS)
    p = ((one - a) * (one - b) * s, a * (one - b) * s, (one - a) * b * s)
    iw = [int(np.rint(v)) for v in p]                     # cvRound: half to even
    half = any(v - np.floor(v) == F(0.5) for v in p)
    return iw[0], iw[1], iw[2], (1 << W_BITS) - iw[0] - iw[1] - iw[2], half


def _bilinear(patch, wt, shift):
    """DESCALE(s00*iw00 + s01*iw01 + s10*iw10 + s11*iw11, shift) over a (h+1, w+1) integer patch."""
    v = patch[:-1, :-1] * wt[0] + patch[:-1, 1:] * wt[1] + patch[1:, :-1] * wt[2] + patch[1:, 1:] * wt[3]
    return (v + (1 << (shift - 1))) >> shift


class _Level:
    """One pyramid level of both frames, as A.2 / A.4 keep it: the images with a winSize border of reflected
    pixels, the derivative planes of the first image with a winSize border of zeros."""

    def __init__(self, I, J, win):
        ww, wh = win
        self.rows, self.cols = I.shape
        ry, rx = _ridx(-wh, self.rows + 2 * wh, self.rows), _ridx(-ww, self.cols + 2 * ww, self.cols)
        self.I = I.astype(np.int64)[np.ix_(ry, rx)]
        self.J = J.astype(np.int64)[np.ix_(ry, rx)]
        d = scharr(I).astype(np.int64)
        self.dx = np.pad(d[..., 0], ((wh, wh), (ww, ww)))
        self.dy = np.pad(d[..., 1], ((wh, wh), (ww, ww)))
        self.win = win

    def outside(self, ix, iy):
        ww, wh = self.win
        return ix < -ww or ix >= self.cols or iy < -wh or iy >= self.rows

    def patch(self, plane, ix, iy):
        ww, wh = self.win
        return plane[iy + wh:iy + 2 * wh + 1, ix + ww:ix + 2 * ww + 1]


def _criteria(criteria):
    t, count, eps = int(criteria[0]), int(criteria[1]), float(criteria[2])
    count = min(max(count, 0), 100) if t & CRIT_COUNT else 30
    eps = min(max(eps, 0.0), 10.0) if t & CRIT_EPS else 0.01
    return count, eps * eps


def _floor(v):
    return int(np.floor(v))


def pyrlk(prev, nxt, prev_pts, next_pts=None, winSize=(21, 21), maxLevel=3,
          criteria=(CRIT_COUNT | CRIT_EPS, 30, 0.01), flags=0, minEigThreshold=1e-4, trace=None):
    """cv2.calcOpticalFlowPyrLK-shaped: (nextPts (N,1,2) f32, status (N,1) u8, err (N,1) f32).

    `trace`, if a list, receives (point, level, tag) for the way each point left each level:
      "outside"       the template window lies outside the level (first bounds test)
      "mineig"        minEig below the threshold
      "det"           minEig test passed, D < FLT_EPSILON
      "zero_iter"     maxCount is 0: no iteration
      "outside_first" the search window lay outside the level before the first iteration (an initial guess)
      "outside_iter"  the search window left the level during the iterations
      "eps"           delta . delta <= eps^2
      "oscillation"   the j > 0 rule with the half step back
      "count"         maxCount iterations done
    and, beside those, the squared length of every step taken (a float in place of the tag, in double as the epsilon
    test forms it), "eps_tie" where a step of non-zero length met eps^2 with equality, "half_weight" where a weight
    product was an exact half before rounding and "err_outside" where the window of the final error lay outside
    level 0."""
    prev, nxt = _u8image(prev), _u8image(nxt)
    if prev.shape != nxt.shape:
        raise ValueError("frames differ in size")
    ww, wh = int(winSize[0]), int(winSize[1])
    p0 = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
    n = len(p0)
    if flags & FLAG_INITIAL_FLOW:
        p1 = np.ascontiguousarray(next_pts, dtype=np.float32).reshape(-1, 2).copy()
    else:
        p1 = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)                          # 0 where OpenCV leaves stale memory (A.5)
    max_count, eps2 = _criteria(criteria)
    thr = F(minEigThreshold)
    win = (ww, wh)
    levels = [_Level(a, b, win) for a, b in zip(build_pyramid(prev, win, maxLevel), build_pyramid(nxt, win, maxLevel))]
    top = len(levels) - 1
    half_x, half_y = F(ww - 1) * F(0.5), F(wh - 1) * F(0.5)
    area2 = F(2 * ww * wh)
    area32 = F(32 * ww * wh)

    def note(i, level, tag):
        if trace is not None:
            trace.append((i, level, tag))

    for i in range(n):
        nx = ny = F(0)
        for level in range(top, -1, -1):
            L = levels[level]
            scale = F(2.0 ** -level)
            px, py = p0[i, 0] * scale, p0[i, 1] * scale
            if level == top:
                if flags & FLAG_INITIAL_FLOW:
                    nx, ny = p1[i, 0] * scale, p1[i, 1] * scale
                else:
                    nx, ny = px, py
            else:
                nx, ny = p1[i, 0] * F(2), p1[i, 1] * F(2)
            p1[i] = (nx, ny)
            px, py = px - half_x, py - half_y
            if not (np.isfinite(px) and np.isfinite(py)):
                raise ValueError("point %d is not finite" % i)
            ix, iy = _floor(px), _floor(py)
            if L.outside(ix, iy):
                if level == 0:
                    status[i] = 0
                    err[i] = F(0)
                note(i, level, "outside")
                continue
            wt = _weights(px - F(ix), py - F(iy))
            if wt[4]:
                note(i, level, "half_weight")
            Iw = _bilinear(L.patch(L.I, ix, iy), wt, W_BITS - 5)
            Ix = _bilinear(L.patch(L.dx, ix, iy), wt, W_BITS)
            Iy = _bilinear(L.patch(L.dy, ix, iy), wt, W_BITS)
            A11 = F(int((Ix * Ix).sum())) * FLT_SCALE
            A12 = F(int((Ix * Iy).sum())) * FLT_SCALE
            A22 = F(int((Iy * Iy).sum())) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / area2
            if flags & FLAG_MIN_EIGENVALS:
                err[i] = min_eig
            if min_eig < thr or D < FLT_EPSILON:
                if level == 0:
                    status[i] = 0
                note(i, level, "mineig" if min_eig < thr else "det")
                continue
            D = F(1) / D
            nx, ny = nx - half_x, ny - half_y
            pdx = pdy = F(0)
            how = "count" if max_count > 0 else "zero_iter"
            for j in range(max_count):
                jx, jy = _floor(nx), _floor(ny)
                if L.outside(jx, jy):
                    if level == 0:
                        status[i] = 0
                    how = "outside_iter" if j > 0 else "outside_first"
                    break
                wj = _weights(nx - F(jx), ny - F(jy))
                if wj[4]:
                    note(i, level, "half_weight")
                diff = _bilinear(L.patch(L.J, jx, jy), wj, W_BITS - 5) - Iw
                b1 = F(int((diff * Ix).sum())) * FLT_SCALE
                b2 = F(int((diff * Iy).sum())) * FLT_SCALE
                dx = (A12 * b2 - A22 * b1) * D
                dy = (A12 * b1 - A11 * b2) * D
                nx, ny = nx + dx, ny + dy
                p1[i] = (nx + half_x, ny + half_y)
                step2 = float(dx) * float(dx) + float(dy) * float(dy)
                note(i, level, step2)
                if step2 <= eps2:
                    if step2 == eps2 and step2 > 0:
                        note(i, level, "eps_tie")
                    how = "eps"
                    break
                if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                    p1[i] = (p1[i, 0] - dx * F(0.5), p1[i, 1] - dy * F(0.5))
                    how = "oscillation"
                    break
                pdx, pdy = dx, dy
            note(i, level, how)
            if status[i] and level == 0 and not flags & FLAG_MIN_EIGENVALS:
                qx, qy = p1[i, 0] - half_x, p1[i, 1] - half_y
                jx, jy = _floor(qx), _floor(qy)
                if L.outside(jx, jy):
                    status[i] = 0
                    note(i, level, "err_outside")
                    continue
                wq = _weights(qx - F(jx), qy - F(jy))
                diff = _bilinear(L.patch(L.J, jx, jy), wq, W_BITS - 5) - Iw
                err[i] = F(int(np.abs(diff).sum())) / area32
    return p1.reshape(-1, 1, 2), status.reshape(-1, 1), err.reshape(-1, 1)


def track_fb(img0, img1, p0, winSize=(21, 21), maxLevel=3, criteria=(CRIT_COUNT | CRIT_EPS, 30, 0.01),
             minEigThreshold=1e-4, fb_threshold=1.0, trace=None):
    """Forward + backward + distance test of the reference loop: dist = np.hypot(|p0 - p0r|) on float32."""
    p0 = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 2)
    p1, st_f, er_f = pyrlk(img0, img1, p0, None, winSize, maxLevel, criteria, 0, minEigThreshold, trace)
    p0r, st_b, er_b = pyrlk(img1, img0, p1, None, winSize, maxLevel, criteria, 0, minEigThreshold, trace)
    p1, p0r = p1.reshape(-1, 2), p0r.reshape(-1, 2)
    d = np.abs(p0 - p0r)
    dist = np.hypot(d[:, 0], d[:, 1])
    assert dist.dtype == np.float32
    return dict(p1=p1, p0r=p0r, st_fwd=st_f.ravel(), st_bwd=st_b.ravel(), err_fwd=er_f.ravel(), err_bwd=er_b.ravel(),
                dist=dist, valid=(dist < F(fb_threshold)).astype(np.uint8))


# ---------------------------------------------------------------------------------------------- A.7
def min_eig_map(img, blockSize=3):
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

    a, b, c = box(dx * dx) * F(0.5), box(dx * dy), box(dy * dy) * F(0.5)
    t = a - c
    eig = (a + c) - np.sqrt(t * t + b * b)
    assert eig.dtype == np.float32
    return eig


def good_features(img, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3, trace=None):
    """cv2.goodFeaturesToTrack-shaped: (M,1,2) float32, or None when nothing is found.

    `trace`, if a list, receives tags: "tie" (two candidates of equal response, ordered by address), "reject_own_cell" /
    "reject_adjacent_cell" (minDistance refusal, by where the neighbour was found), "border_refused" (a pixel of the
    1-px frame border that met every other condition) and "maxcorners_stop"."""
    img = _u8image(img)
    h, w = img.shape
    eig = min_eig_map(img, blockSize)
    ok = np.ones((h, w), bool) if mask is None else (_u8image(mask) != 0)
    max_val = float(eig[ok].max()) if ok.any() else 0.0
    thresh = F(max_val * float(qualityLevel))
    t = np.where(eig > thresh, eig, F(0))                      # THRESH_TOZERO keeps strictly greater
    big = np.full((h + 2, w + 2), -np.inf, np.float32)
    big[1:-1, 1:-1] = t
    dil = np.max([big[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    keep = (t != 0) & (t == dil) & ok
    if trace is not None:
        edge = keep.copy()
        edge[1:-1, 1:-1] = False
        trace.extend(["border_refused"] * int(edge.sum()))
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    idx = np.nonzero(keep.ravel())[0]
    vals = t.ravel()[idx]
    order = sorted(range(len(idx)), key=lambda k: (-float(vals[k]), -int(idx[k])))   # higher address first among equals
    if trace is not None:
        trace.extend(["tie"] * sum(1 for a, b in zip(order, order[1:]) if vals[a] == vals[b]))
    out = []
    if minDistance >= 1:
        cell = int(np.rint(float(minDistance)))                 # cvRound
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = {}
        md2 = float(minDistance) * float(minDistance)
        for k in order:
            y, x = divmod(int(idx[k]), w)
            xc, yc = x // cell, y // cell
            found = None
            for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
                for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                    for (qx, qy) in grid.get((xx, yy), ()):
                        if (x - qx) * (x - qx) + (y - qy) * (y - qy) < md2:
                            found = (xx, yy)
                            break
                    if found:
                        break
                if found:
                    break
            if found:
                if trace is not None:
                    trace.append("reject_own_cell" if found == (xc, yc) else "reject_adjacent_cell")
                continue
            grid.setdefault((xc, yc), []).append((x, y))
            out.append((x, y))
            if maxCorners > 0 and len(out) == maxCorners:
                if trace is not None:
                    trace.append("maxcorners_stop")
                break
    else:
        for k in order:
            y, x = divmod(int(idx[k]), w)
            out.append((x, y))
            if maxCorners > 0 and len(out) == maxCorners:
                if trace is not None:
                    trace.append("maxcorners_stop")
                break
    if not out:
        return None
    return np.array(out, np.float32).reshape(-1, 1, 2)


class RestatementCv:
    """cv2-shaped facade over this module, to drive tests/reference_loops.run_reference_loop."""

    @staticmethod
    def calcOpticalFlowPyrLK(a, b, p0, p1, **kw):
        return pyrlk(a, b, p0, p1, **kw)

    @staticmethod
    def goodFeaturesToTrack(img, mask=None, **kw):
        return good_features(img, kw["maxCorners"], kw["qualityLevel"], kw["minDistance"], mask, kw.get("blockSize", 3))

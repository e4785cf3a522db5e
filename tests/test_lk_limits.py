"""The LK tracker's integer arithmetic at its limits, on the host (no GPU).

- The content families of extreme_frames.py reach the regimes the GPU tests (test_gpu_extremes.py) claim to exercise:
  window sums above 2^31 and 2^32 (the high word of lk_common.h's 64-bit sums), lane partials of the generic kernel
  within a few per cent of 2^31.
- An independent numpy statement of one LK level (maxLevel 0) -- reflect-101 padding, Scharr, float32 bilinear weights,
  exact int64 sums, OpenCV's float32 solve, float64 convergence test, oscillation back-off, err -- gives the oracle's
  result bit for bit on every family, so the oracle itself is checked where the GPU tests lean on it.
- sum_to_float (k_lk_fast.hip) is the correctly rounded int64 -> float conversion over the whole range of its sums.
"""
import numpy as np
import pytest

import extreme_frames as xf
from test_oracle_kat import np_scharr

FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
FLT_SCALE = np.float32(1.0 / (1 << 20))
MAX_IX = 16 * 255                   # |Scharr| of 8-bit content
MAX_DIFF = 32 * 255                 # |J - I| in the 5-bit fixed point of the tracker


# -- regime ------------------------------------------------------------------------------------------------------------

def _corner_points(w, h, win, step):
    """Points whose windows have integer top-left corners, on a grid over the frame."""
    half = ((win[0] - 1) * 0.5, (win[1] - 1) * 0.5)
    xs = np.arange(0, w - win[0], step) + half[0]
    ys = np.arange(0, h - win[1], step) + half[1]
    return np.float32([(x, y) for y in ys for x in xs])


@pytest.mark.parametrize("family", list(xf.FAMILIES))
def test_families_reach_the_regimes_the_gpu_tests_claim(family):
    w, h = 320, 240
    I, J, _ = xf.FAMILIES[family](w, h, 7)
    assert I.dtype == J.dtype == np.uint8 and I.shape == J.shape == (h, w)
    d = np.abs(np_scharr(I).astype(np.int64))
    s21 = xf.window_sums(I, J, _corner_points(w, h, (21, 21), 7), (21, 21))
    s35 = xf.window_sums(I, J, _corner_points(w, h, (35, 35), 9), (35, 35))
    a21 = max(max(s["a11"], s["a22"]) for s in s21)
    a35 = max(max(s["a11"], s["a22"]) for s in s35)
    b21 = max(abs(s["b1"]) for s in s21)
    if family in ("blocks2", "blocks3", "mondrian", "stripes", "inverted"):
        assert d.max() == MAX_IX
        assert a21 > 2 ** 31, "no 21x21 sum beyond 2^31 (%g x 2^31)" % (a21 / 2 ** 31)
        assert a35 > 2 ** 32, "no 35x35 sum beyond 2^32 (%g x 2^32)" % (a35 / 2 ** 32)
    if family == "blocks4":
        assert d.max() == MAX_IX and a21 > 2 ** 30 and a35 > 2 ** 31
    if family == "stretched16":
        assert d.max() == MAX_IX and a35 > 2 ** 31
        assert ((I == 0) | (I == 255)).mean() > 0.5
    if family == "stretched4":
        assert d.max() > 3000 and ((I == 0) | (I == 255)).mean() > 0.1
    if family == "stripes":
        assert b21 > 2 ** 31, "first-iteration b1 stays below 2^31 (%g)" % (b21 / 2 ** 31)
    if family == "saturated":
        assert (I == 255).sum() >= 60 * 80 and (I == 0).sum() >= 70 * 90
    if family == "inverted":
        diff = 32 * (J.astype(np.int64) - I)
        assert np.abs(diff).max() == MAX_DIFF


def test_stripes_put_generic_lanes_at_the_int32_bound():
    """k_lk at 64x64: lane l holds window pixels l, l + 64, ... (column l of every row).  Some lane's first-iteration
    b1 partial is within 10 % of 2^31, and none passes it; the 21/35/41 windows see sums of half their group bound."""
    w, h = 480, 200
    I, J, _ = xf.stripes(w, h)
    for win in ((64, 64), (21, 21), (35, 35), (41, 41)):
        pts = xf.stripe_points(w, h, win)
        assert len(pts) >= 10
        sums = xf.window_sums(I, J, pts, win)
        assert len(sums) == len(pts)
        if win == (64, 64):
            lanes = np.stack([s["b1_px"].reshape(-1, 64).sum(0) for s in sums])
            assert lanes.max() > 0.9 * 2 ** 31, lanes.max() / 2 ** 31
            assert np.abs(lanes).max() <= xf.INT32_MAX
        # every second column carries the full product +8 160 * 4 080 on the rows outside the band
        px = np.stack([s["b1_px"] for s in sums])
        assert px.max() == MAX_DIFF * MAX_IX and px.min() >= 0
        assert max(s["b1"] for s in sums) > 2 ** 31 if win != (21, 21) else True


def test_sub_ulp_points_give_negative_w11_and_ties():
    pts, wts = xf.sub_ulp_points((21, 21))
    assert any(w[3] == -1 for w in wts), "no point with iw11 = -1"
    # the issue's example: (110 + 6 * 2^-17, 110 + 5 * 2^-17) with a 21x21 window
    a = np.float32(110 + 6 * 2.0 ** -17) - np.float32(10)
    b = np.float32(110 + 5 * 2.0 ** -17) - np.float32(10)
    assert xf.bilinear_weights(a - np.float32(100), b - np.float32(100)) == (16383, 1, 1, -1)
    assert len(pts) > 10


# -- one LK level, restated in numpy -----------------------------------------------------------------------------------

def _reflect101(p, n):
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo]
        p[hi] = 2 * n - 2 - p[hi]


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def np_lk_level0(I, J, prev_pts, next_pts=None, win=(21, 21), criteria=(3, 30, 0.01), flags=0, min_eig=1e-4):
    """cv2.calcOpticalFlowPyrLK at maxLevel 0 in the oracle's named variant (exact int64 sums)."""
    h, w = I.shape
    ww, wh = win
    # images padded by the window with reflect-101, derivatives of the unpadded image zero-padded by the window
    ry, rx = _reflect101(np.arange(-wh, h + wh), h), _reflect101(np.arange(-ww, w + ww), w)
    Ip = I.astype(np.int64)[np.ix_(ry, rx)]
    Jp = J.astype(np.int64)[np.ix_(ry, rx)]
    dI = np.zeros((h + 2 * wh, w + 2 * ww, 2), np.int64)
    dI[wh:wh + h, ww:ww + w] = np_scharr(I)

    ctype, count, eps = criteria
    count = 30 if not ctype & 1 else min(max(int(count), 0), 100)
    eps = 0.01 if not ctype & 2 else min(max(float(eps), 0.0), 10.0)
    eps *= eps
    half_x, half_y = np.float32((ww - 1) * 0.5), np.float32((wh - 1) * 0.5)
    thr = np.float32(min_eig)
    npx = len(prev_pts)
    p0 = np.asarray(prev_pts, np.float32).reshape(-1, 2)
    p1 = (np.asarray(next_pts, np.float32).reshape(-1, 2) if flags & 4 else p0).copy()
    st = np.ones(npx, np.uint8)
    err = np.zeros(npx, np.float32)
    f32 = np.float32

    def inside(ix, iy):
        return -ww <= ix < w and -wh <= iy < h

    def patch(img, ix, iy, wts):
        y, x = iy + wh, ix + ww
        a = img[y:y + wh + 1, x:x + ww + 1]
        return a[:-1, :-1] * wts[0] + a[:-1, 1:] * wts[1] + a[1:, :-1] * wts[2] + a[1:, 1:] * wts[3]

    for i in range(npx):
        px, py = p0[i, 0] - half_x, p0[i, 1] - half_y
        ipx, ipy = int(np.floor(px)), int(np.floor(py))
        if not inside(ipx, ipy):
            st[i] = 0
            continue
        wts = xf.bilinear_weights(px - f32(ipx), py - f32(ipy))
        Iw = _descale(patch(Ip, ipx, ipy, wts), xf.W_BITS - 5)
        ixw = _descale(patch(dI[..., 0], ipx, ipy, wts), xf.W_BITS)
        iyw = _descale(patch(dI[..., 1], ipx, ipy, wts), xf.W_BITS)
        A11 = f32(int((ixw * ixw).sum())) * FLT_SCALE
        A12 = f32(int((ixw * iyw).sum())) * FLT_SCALE
        A22 = f32(int((iyw * iyw).sum())) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        me = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + f32(4) * A12 * A12)) / f32(2 * ww * wh)
        if flags & 8:
            err[i] = me
        if me < thr or D < FLT_EPSILON:
            st[i] = 0
            continue
        D = f32(1) / D
        nx, ny = p1[i, 0] - half_x, p1[i, 1] - half_y
        pdx = pdy = f32(0)
        for j in range(count):
            inx, iny = int(np.floor(nx)), int(np.floor(ny))
            if not inside(inx, iny):
                st[i] = 0
                break
            wj = xf.bilinear_weights(nx - f32(inx), ny - f32(iny))
            diff = _descale(patch(Jp, inx, iny, wj), xf.W_BITS - 5) - Iw
            b1 = f32(int((diff * ixw).sum())) * FLT_SCALE
            b2 = f32(int((diff * iyw).sum())) * FLT_SCALE
            dx = (A12 * b2 - A22 * b1) * D
            dy = (A12 * b1 - A11 * b2) * D
            nx, ny = nx + dx, ny + dy
            p1[i] = (nx + half_x, ny + half_y)
            if float(dx) * float(dx) + float(dy) * float(dy) <= eps:
                break
            if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                p1[i] = (p1[i, 0] - dx * f32(0.5), p1[i, 1] - dy * f32(0.5))
                break
            pdx, pdy = dx, dy
        if st[i] and not flags & 8:
            qx, qy = p1[i, 0] - half_x, p1[i, 1] - half_y
            iqx, iqy = int(np.floor(qx)), int(np.floor(qy))
            if not inside(iqx, iqy):
                st[i] = 0
                continue
            wq = xf.bilinear_weights(qx - f32(iqx), qy - f32(iqy))
            diff = _descale(patch(Jp, iqx, iqy, wq), xf.W_BITS - 5) - Iw
            err[i] = f32(int(np.abs(diff).sum())) * f32(1) / f32(32 * ww * wh)
    return p1.reshape(-1, 1, 2), st.reshape(-1, 1), err.reshape(-1, 1)


def _same(orc_out, np_out):
    (q1, qs, qe), (p1, st, er) = orc_out, np_out
    assert np.array_equal(qs, st), "status differs at %s" % np.nonzero(qs != st)[0][:10]
    bad = np.nonzero((q1.view(np.uint32) != p1.view(np.uint32)).any(axis=-1).ravel())[0]
    assert len(bad) == 0, "nextPts differ at %s: %s vs %s" % (bad[:5], q1.reshape(-1, 2)[bad[:3]], p1.reshape(-1, 2)[bad[:3]])
    assert np.array_equal(qe.view(np.uint32), er.view(np.uint32)), "err differs"


CRITERIA = [(3, 30, 0.01), (1, 7, 0.0), (2, 0, 0.05), (3, 25, 0.03)]


@pytest.mark.parametrize("family", list(xf.FAMILIES))
def test_numpy_lk_level_equals_the_oracle(orc, family):
    w, h = 160, 120
    I, J, _ = xf.FAMILIES[family](w, h, 11)
    rng = np.random.RandomState(len(family))
    if family == "saturated":
        pts = np.concatenate([xf.saturated_points(w, h), xf.points(rng, 30, w, h)])
    elif family == "stripes":
        pts = np.concatenate([xf.stripe_points(w, h, (21, 21), n=12), xf.points(rng, 20, w, h)])
    else:
        pts = xf.points(rng, 40, w, h)
    for k, (win, crit) in enumerate(zip(((21, 21), (35, 35), (15, 9), (31, 31)), CRITERIA)):
        ref = orc.pyrlk(I, J, pts, None, win, 0, crit)
        _same(ref, np_lk_level0(I, J, pts, None, win, crit))
        live = ref[1][:12] if family == "stripes" else ref[1]     # off the band rows, stripes alone are singular
        assert live.sum() >= 0.4 * len(live), (win, live.sum())


def test_numpy_lk_level_with_flags_and_sub_ulp_points(orc):
    w, h = 240, 220
    for family in ("stretched16", "blocks2"):
        I, J, _ = xf.FAMILIES[family](w, h, 5)
        for win in ((21, 21), (35, 35)):
            pts, wts = xf.sub_ulp_points(win)
            pts = pts[:40]
            assert any(t[3] == -1 for t in wts[:40])
            guess = pts + np.float32([0.75, -0.5])
            for flags in (0, 4, 8, 12):
                for crit in ((1, 1, 0.0), (3, 30, 0.01), (2, 0, 0.02)):
                    g = guess if flags & 4 else None
                    ref = orc.pyrlk(I, J, pts, g, win, 0, crit, flags)
                    _same(ref, np_lk_level0(I, J, pts, g, win, crit, flags))
            # the same positions as the iteration's guess (COUNT 1): the weights of J's patch
            ref = orc.pyrlk(I, J, pts + np.float32([2.25, 1.5]), pts, win, 0, (1, 1, 0.0), 4)
            _same(ref, np_lk_level0(I, J, pts + np.float32([2.25, 1.5]), pts, win, (1, 1, 0.0), 4))


# -- sum_to_float ------------------------------------------------------------------------------------------------------

def sum_to_float(t):
    """k_lk_fast.hip's sum_to_float in numpy float32: float(t >> 16) * 65536 + float(t & 0xffff), each op rounded."""
    t = np.asarray(t, np.int64)
    hi = (t >> 16).astype(np.int32)
    lo = (t & 0xffff).astype(np.int32)
    return (hi.astype(np.float32) * np.float32(65536)) + lo.astype(np.float32)


def test_sum_to_float_is_the_rounded_conversion():
    rng = np.random.RandomState(3)
    top = 35 * 35 * MAX_DIFF * MAX_IX            # the largest |sum| of k_lk_fast (35x35 is its widest window)
    assert top < 2 ** 36
    edges = []
    for e in (24, 25, 31, 32, 33, 35, 36, 39):
        c = 1 << e
        edges.append(np.arange(c - 70000, c + 70000))
    lots = rng.randint(-top, top + 1, 2_000_000)
    # halfway cases: values with exactly one bit beyond float's 24 below the leading bit
    ties = np.int64(rng.randint(1 << 23, 1 << 24, 20000)) << np.int64(12) | np.int64(1 << 11)
    t = np.concatenate(edges + [lots, ties, -ties, np.int64([0, 1, -1, top, -top, 2 ** 40 - 1, -(2 ** 40) + 1])])
    t = np.concatenate([t, -t])
    got = sum_to_float(t)
    want = t.astype(np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, "sum_to_float(%d) = %r, float(t) = %r" % (t[bad[0]], got[bad[0]], want[bad[0]])


def test_sum_to_float_bound_in_its_comment_is_tight():
    """Above 2^40 float(t >> 16) itself rounds and the sum is rounded twice: the bound in the comment is not loose."""
    t = np.int64((1 << 41) + (1 << 17) + 1)
    assert sum_to_float(t) != np.float32(t)
